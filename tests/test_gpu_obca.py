"""GPU parity of the OBCA local subproblem: the batched SQP of
csrc/piadmm_obca.hip through the C-ABI (piadmm_obca_solve) against oracle/obca_oracle.py on the
two-vehicle overtaking scenario (decentralized_overtaking_ADMM.py:22-42; every MPC step 0..41,
both vehicles, three bar_state variants, both halfspace models).

Bar: same status; for converged problems X, U, Lambda within ATOL = 1e-7 (rel. 1e-9 of the state
scale) and the cost within RTOL = 1e-9; and the GPU answer, with the GPU's multipliers, is a KKT
point of the reference's NLP (optimizer.py:84-168) -- stationarity <= 1e-9 of the gradient
scale, feasibility and complementarity <= 1e-8.  Agreement with IPOPT is unpinned (CasADi absent).

Off the defaults (second half of the file, case sets of tests/_obca_cases.py): runs truncated at
max_iter = 1..4 and six off-default parameter sets plus the exchanged-plan set, held to the oracle
with exact iteration counts and all seven multiplier blocks; the longest-first schedule of a
resident batch (the path bench.py --obca times); independence of the blocks of one launch; one
handle across batch sizes; and the state / argument errors of the resident-batch calls.
"""
import numpy as np
import pytest

import _obca_cases as C
from oracle import obca_oracle as O
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

ATOL = 1e-7


@pytest.fixture(scope="module")
def batch():
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    b = obca.OBCABatch(0)
    yield b
    b.close()


def _oracle(recs):
    out = []
    for rec in recs:
        p, opt = O.from_record(rec)
        out.append((p, O.solve_local(p, opt)))
    return out


def _check(recs, res, orc, kkt=True):
    n_conv = 0
    for k, (p, r) in enumerate(orc):
        assert res.status[k] == r.status, (k, res.status[k], r.status)
        if r.status != O.CONVERGED:
            continue
        n_conv += 1
        assert abs(int(res.iters[k]) - r.iters) <= 1, (k, res.iters[k], r.iters)
        np.testing.assert_allclose(res.X[k], r.X, rtol=1e-9, atol=ATOL, err_msg=f"X {k}")
        np.testing.assert_allclose(res.U[k], r.U, rtol=1e-9, atol=ATOL, err_msg=f"U {k}")
        np.testing.assert_allclose(res.Lam[k], r.Lam, rtol=1e-9, atol=ATOL, err_msg=f"Lambda {k}")
        assert abs(res.cost[k] - r.cost) <= 1e-9 * max(1.0, abs(r.cost)), (k, res.cost[k], r.cost)
        if kkt:
            _check_kkt(p, res, k)
    return n_conv


def _check_kkt(p, res, k):
    """The GPU's answer to problem k, with the GPU's multipliers, is a KKT point of p."""
    kk = O.kkt_residual(p, res.X[k], res.U[k], res.Lam[k], res.y_a[k], res.y_b[k], res.y_n[k], res.y_x[k],
                        res.pi[k], res.y_u[k], res.y_l[k])
    gscale = 1.0 + 2 * p.q * np.abs(res.X[k][1:] - p.ref[1:]).max()
    assert max(kk["stat_x"], kk["stat_u"], kk["stat_l"]) <= 1e-9 * gscale, (k, kk)
    assert kk["feas"] <= 1e-8 and kk["comp"] <= 1e-8, (k, kk)


@pytest.mark.parametrize("prob", [1, 0])
def test_gpu_equals_oracle_on_the_overtaking_scenario(batch, prob):
    recs = np.stack([obca.overtaking_problem(ts, v, var, prob=prob)
                     for ts in range(0, 42, 1 if prob else 3) for v in (0, 1)
                     for var in ("initial", "consensus", "perturbed")])
    res = batch.solve(recs)
    orc = _oracle(recs)
    n_conv = _check(recs, res, orc)
    assert n_conv >= 0.95 * len(recs)
    # the window where (5a) binds is covered
    assert np.sum(np.max(res.y_a, axis=1) > 1.0) >= 10


def test_reference_as_written_is_reported_infeasible(batch):
    recs = np.stack([obca.as_written_problem(ts, v) for ts in (0, 5) for v in (0, 1)])
    res = batch.solve(recs)
    assert np.all(res.status == obca_status("qp_infeasible"))
    assert np.all(res.iters == 1)


def obca_status(name):
    return {v: k for k, v in obca.STATUS.items()}[name]


def test_resident_batch_and_timing_equal_one_shot_solve(batch):
    recs = obca.scenario_batch(300, seed=2)
    a = batch.solve(recs)
    batch.upload(recs)
    ms = batch.time(3)
    assert ms > 0
    b = batch.download(len(recs))
    np.testing.assert_array_equal(a.raw, b.raw)
    np.testing.assert_array_equal(a.status, b.status)


def test_errors_are_reported_before_any_launch(batch):
    rec = obca.overtaking_problem(3, 0)
    bad = rec.copy()
    bad[283 + 6] = 2.0          # prob must be 0 / 1
    with pytest.raises(_lib.PiadmmError, match="bad parameters"):
        batch.solve(bad[None])
    bad = rec.copy()
    bad[283 + 7] = 0.0          # max_iter >= 1
    with pytest.raises(_lib.PiadmmError):
        batch.solve(bad[None])
    # the handle still works
    r = batch.solve(rec[None])
    assert r.status[0] == 0


# ---------------------------------------------------------------------------------------------
# The case sets of tests/_obca_cases.py (proved sound on the CPU by tests/test_obca_cases.py):
# status and SQP iteration count equal the oracle's EXACTLY, and X, U, Lambda, the cost and all
# seven multiplier blocks are compared for every status that writes an iterate -- converged or
# stopped at max_iter alike -- so a truncated run compares the SQP step itself (line search,
# merit parameter, multiplier blend, warm start), not only the fixed point.
#
# Problems whose iteration count may differ from the oracle's: none.  One may be added only with
# the evidence from the oracle's Options.trace that its step or violation at that iteration lies
# within 10 x tol_step / tol_feas, and at most 2 % of a set.
# ---------------------------------------------------------------------------------------------
EXEMPT = {}


def _compare_set(batch, name, recs, kkt):
    res = batch.solve(recs)
    orc = C.oracle(recs)
    exempt = EXEMPT.get(name, ())
    assert len(exempt) <= 0.02 * len(recs)
    worst = C.compare(res, orc, exempt=exempt)
    C.report(f"GPU vs oracle, {name} ({len(recs)} problems)", worst)
    if kkt:
        for k, (p, r) in enumerate(orc):
            if r.status == O.CONVERGED and res.status[k] == O.CONVERGED:
                _check_kkt(p, res, k)
    return res


@pytest.mark.parametrize("k", [1, 2, 3, 4])
def test_truncated_sqp_iterates_equal_oracle(batch, k):
    res = _compare_set(batch, f"truncated_{k}", C.truncated(k), kkt=False)
    # the runs do stop inside the SQP (tests/test_obca_cases.py holds the oracle to the same)
    assert np.sum(res.status == obca_status("max_iter")) >= 5
    assert np.all(res.iters[res.status == obca_status("max_iter")] == k)


@pytest.mark.parametrize("name", C.OFF_DEFAULT_NAMES + ("exchanged",))
def test_off_default_parameters_equal_oracle(batch, name):
    recs = C.exchanged() if name == "exchanged" else C.off_default()[name]
    res = _compare_set(batch, name, recs, kkt=True)
    if name == "r_q_1":
        assert np.sum(np.max(np.abs(res.y_u), axis=1) > 1e-6) >= 5        # control-bound rows active
    if name == "state_box":
        assert np.sum(np.min(res.y_x[:, :, 0], axis=1) < -1e-6) >= 5      # the upper x row binds
    if name == "infeasible":
        assert np.sum(res.status == obca_status("qp_infeasible")) >= 5


def _fresh_solve(recs):
    b = obca.OBCABatch(0)
    try:
        return b.solve(recs)
    finally:
        b.close()


def _bits(raw):
    return np.ascontiguousarray(raw).view(np.uint64)


def _same(a, b):
    """Two OBCAResults are bit-identical: the outputs and the status / iterations / QP steps."""
    np.testing.assert_array_equal(_bits(a.raw), _bits(b.raw))
    np.testing.assert_array_equal(np.stack([a.status, a.iters, a.qp_steps]), np.stack([b.status, b.iters, b.qp_steps]))


def test_longest_first_schedule_keeps_answers():
    """After a run on the same upload, block b solves problem order[b] (longest first by the last
    run's QP steps and SQP iterations): what bench.py --obca times and dumps.  The answers do not
    depend on the order, and the order of one batch is not carried over to the next."""
    recs = obca.scenario_batch(300, seed=2)
    n = len(recs)
    b = obca.OBCABatch(0)
    try:
        b.upload(recs)
        b.run_async(1)                    # index order (no run on this upload yet)
        a = b.download(n)
        assert b.time(2) > 0              # both launches in the order from a's work
        r2 = b.download(n)
        assert b.time(1) > 0              # rescheduled from the permuted run's work
        r3 = b.download(n)
        _same(a, r2)
        _same(a, r3)
        _same(a, _fresh_solve(recs))
        # the schedule() of the second and third run, rebuilt here: not the identity, so the
        # indirect addressing was exercised
        order = sorted(range(n), key=lambda i: (-int(a.qp_steps[i]), -int(a.iters[i])))
        assert sorted(order) == list(range(n))
        moved = sum(order[i] != i for i in range(n))
        assert moved >= n // 4, moved
        # another batch of the same size: the old batch's order does not apply to it
        other = obca.scenario_batch(n, seed=3)
        assert not np.array_equal(other, recs)
        b.upload(other)
        b.run_async(1)
        _same(b.download(n), _fresh_solve(other))
    finally:
        b.close()


def test_blocks_do_not_share_state(batch):
    """64 copies of one record between 66 different ones (converged, stopped at max_iter and
    qp_infeasible among them): every copy's rows are those of the record solved alone."""
    rep = C.BASE[C.KEYS.index((1, 14, 0, "perturbed"))]
    pool = (list(C.off_default()["infeasible"][0::3][:22]) + list(C.truncated(2)[1::3][:22])
            + list(C.off_default()["r_q_1"][2::3][:22]))
    assert len(pool) == 66
    recs, copies = [], []
    for i, rec in enumerate(pool):
        recs.append(rec)
        if i < 64:
            copies.append(len(recs))
            recs.append(rep)
    recs = np.ascontiguousarray(np.stack(recs))
    assert len(recs) == 130 and len(copies) == 64
    alone = batch.solve(rep[None])
    assert alone.status[0] == obca_status("converged") and alone.iters[0] >= 3
    others = batch.solve(np.ascontiguousarray(np.stack(pool)))
    for name in ("converged", "max_iter", "qp_infeasible"):
        assert np.sum(others.status == obca_status(name)) >= 5, name
    res = batch.solve(recs)
    for k in copies:
        np.testing.assert_array_equal(_bits(res.raw[k]), _bits(alone.raw[0]), err_msg=f"copy at {k}")
        assert (res.status[k], res.iters[k], res.qp_steps[k]) == (alone.status[0], alone.iters[0], alone.qp_steps[0])
    # and the different ones are not disturbed by the copies
    rest = [k for k in range(len(recs)) if k not in copies]
    np.testing.assert_array_equal(_bits(res.raw[rest]), _bits(others.raw))
    np.testing.assert_array_equal(res.status[rest], others.status)
    np.testing.assert_array_equal(res.iters[rest], others.iters)
    np.testing.assert_array_equal(res.qp_steps[rest], others.qp_steps)


def test_handle_survives_batch_size_changes():
    """One handle through batches of 4, 300, 4 and 1 problems (the buffers grow once and are then
    reused above the batch; the schedule restarts with every upload)."""
    big = obca.scenario_batch(300, seed=2)
    b = obca.OBCABatch(0)
    try:
        for recs in (big[:4], big, big[:4], big[7:8]):
            recs = np.ascontiguousarray(recs)
            _same(b.solve(recs), _fresh_solve(recs))
    finally:
        b.close()


def test_state_and_argument_errors():
    recs = obca.scenario_batch(4, seed=2)
    b = obca.OBCABatch(0)
    try:
        with pytest.raises(_lib.PiadmmError, match="before obca_upload"):
            b.run_async(1)
        with pytest.raises(_lib.PiadmmError, match="before obca_upload"):
            b.time(1)
        b.upload(recs)
        with pytest.raises(_lib.PiadmmError):
            b.time(0)
        b.run_async(1)
        with pytest.raises(_lib.PiadmmError, match="uploaded batch"):
            b.download(3)
        with pytest.raises(_lib.PiadmmError, match="uploaded batch"):
            b.download(5)
        good = b.download(4)
        bad = recs.copy()
        bad[2, 283 + 0] = 0.0             # rho > 0
        with pytest.raises(_lib.PiadmmError, match="record 2: bad parameters"):
            b.upload(bad)
        # the rejected upload changed nothing: the good batch is still resident
        b.run_async(1)
        _same(b.download(4), good)
        _same(good, _fresh_solve(recs))
    finally:
        b.close()
