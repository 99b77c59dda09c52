"""GPU parity of the OBCA-ADMM edge step: csrc/piadmm_obca_edge.hip through the C-ABI
(piadmm_obca_edge_solve) against the NumPy restatement tests/_obca_edge_ref.py on the case sets
proved sound by tests/test_obca_edge_ref.py and on the hard-branch sets of tests/_obca_edge_cases.py
(proved by tests/test_obca_edge_cases.py), and the planner loop (piadmm.obca.OBCAPlanner)
teacher-forced stage by stage.

Bars (those of tests/test_gpu_obca.py): status, SQP iteration count and QP step count equal the
restatement's exactly; Z, multipliers and cost within ATOL 1e-7 / rtol 1e-9; the GPU's own answer, with the
GPU's multipliers, is a KKT point of the slot NLP -- stationarity <= 1e-9 of the gradient scale,
feasibility and complementarity <= 1e-8.
"""
import numpy as np
import pytest

import _obca_cases as C
import _obca_edge_cases as K
import _obca_edge_ref as E
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

ATOL, RTOL = 1e-7, 1e-9
MULT_TOL = 1e-7

# Slots (set name -> [(record, slot)]) whose iteration count may differ from the restatement's:
# none.  One may be added only with the evidence that its step or violation at that iteration
# lies within 10 x tol_step / tol_feas, and at most 2 % of a set.
EXEMPT = {}


@pytest.fixture(scope="module")
def batch():
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    b = obca.OBCABatch(0)
    yield b
    b.close()


def _compare(res, recs, name="", kkt=True, keep=None):
    """An OBCAEdgeResult against the restatement, slot by slot (`keep`: the (record, slot) pairs
    to compare, all by default)."""
    exempt = EXEMPT.get(name, ())
    assert len(exempt) <= 0.02 * len(recs) * obca.NT
    worst = dict(z=0.0, mult=0.0, cost=0.0, stat=0.0, feas=0.0, comp=0.0)
    for k, rec in enumerate(recs):
        for t, (p, r) in enumerate(E.solve_record(rec)):
            if keep is not None and (k, t) not in keep:
                continue
            same = res.status[k, t] == r.status and int(res.iters[k, t]) == r.iters
            if not same and (k, t) in exempt:
                continue
            assert same, (name, k, t, int(res.status[k, t]), r.status, int(res.iters[k, t]), r.iters)
            # the QP step count: a difference at equal status and iterations is a finding, not an exemption
            assert int(res.qp_steps[k, t]) == r.qp_steps, (name, k, t, int(res.qp_steps[k, t]), r.qp_steps)
            if r.status not in E.WRITES_ITERATE:
                continue
            z = res.z(k, t)
            worst["z"] = max(worst["z"], float(np.abs(z - r.z).max()))
            np.testing.assert_allclose(z, r.z, rtol=RTOL, atol=ATOL, err_msg=f"{name} Z {k} {t}")
            dev = abs(res.cost[k, t] - r.cost) / max(1.0, abs(r.cost))
            worst["cost"] = max(worst["cost"], float(dev))
            assert dev <= RTOL, (name, k, t, res.cost[k, t], r.cost)
            for got, ref in ((res.y_eq[k, t], r.y_eq), (res.y_in[k, t], r.y_in), (res.y_bnd[k, t], r.y_bnd)):
                got, ref = np.atleast_1d(got), np.atleast_1d(ref)
                dev = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
                worst["mult"] = max(worst["mult"], dev)
                assert dev <= MULT_TOL, (name, k, t, dev)
            if kkt and res.status[k, t] == E.CONVERGED:
                kk = E.kkt_residual_edge(p, z, res.y_eq[k, t], res.y_in[k, t], res.y_bnd[k, t])
                worst["stat"] = max(worst["stat"], kk["stat"] / kk["gscale"])
                worst["feas"], worst["comp"] = max(worst["feas"], kk["feas"]), max(worst["comp"], kk["comp"])
                assert kk["stat"] <= 1e-9 * kk["gscale"], (name, k, t, kk)
                assert kk["feas"] <= 1e-8 and kk["comp"] <= 1e-8, (name, k, t, kk)
    print(f"{name}: worst " + "  ".join(f"{a} {b:.1e}" for a, b in worst.items()))
    return worst


@pytest.mark.parametrize("name", E.SET_NAMES)
def test_gpu_equals_restatement(batch, name):
    recs = E.case_set(name)
    res = batch.solve_edge(recs)
    _compare(res, recs, name)


def test_rounding(batch):
    recs = np.concatenate([E.case_set("exchanged"), E.case_set("pressed")])
    res = batch.solve_edge(recs)
    n, skipped = 0, 0
    for k, rec in enumerate(recs):
        for t, (p, r) in enumerate(E.solve_record(rec)):
            assert res.status[k, t] == r.status
            x = r.z * 1e4
            tie = np.abs(np.abs(x - np.floor(x)) - 0.5) < 1e-6 * 1e4      # within 1e-6 of a rounding tie
            want = np.round(r.z, 4)
            got = np.concatenate([res.Z_bar[k, 0, t], res.Z_bar[k, 1, t]])
            n += x.size
            skipped += int(tie.sum())
            np.testing.assert_array_equal(got[~tie], want[~tie])
    print(f"rounding: {skipped} of {n} values within 1e-6 of a tie")
    assert skipped <= 0.05 * n
    off = recs.copy()
    off[:, obca._E_PAR + 4] = -1.0
    r2 = batch.solve_edge(off)
    np.testing.assert_array_equal(r2.Z_bar, r2.Z)
    np.testing.assert_array_equal(r2.Z, res.Z)


def _check_dual_update(res, recs):
    """lamb_bar_new and the dual-residual partials against the host form on the GPU's own Z_bar;
    returns the number of slots that wrote no iterate."""
    n_kept = 0
    for k, rec in enumerate(recs):
        d = obca.edge_unpack(rec)
        w = np.concatenate([d["local_x"], d["lamb_ij"]], axis=2)
        total = 0.0
        for t in range(obca.NT):
            if res.status[k, t] in obca.EDGE_WRITES_ITERATE:
                want = d["lamb_bar"][:, t] + d["rho"] * (w[:, t] - res.Z_bar[k, :, t])
                np.testing.assert_allclose(res.lamb_bar[k, :, t], want, rtol=0, atol=1e-12)
            else:
                n_kept += 1
                np.testing.assert_array_equal(res.lamb_bar[k, :, t], d["lamb_bar"][:, t])
                assert res.dres[k, t] == 0.0
            total += np.abs(res.lamb_bar[k, :, t] - d["lamb_bar"][:, t]).sum()
        assert abs(res.dual_residual()[k] - total) <= 1e-12 * max(1.0, total)
    return n_kept


def test_fused_dual_update(batch):
    recs = np.concatenate([E.case_set("exchanged"), E.case_set("zero_start")])
    assert _check_dual_update(batch.solve_edge(recs), recs) >= 1          # zero_start: slots that wrote no iterate


@pytest.mark.parametrize("n_pairs", [1, 3, 65])
def test_batch_shapes(batch, n_pairs):
    pool = np.concatenate([E.case_set("exchanged"), E.case_set("pressed"), E.case_set("bounds")])
    recs = np.ascontiguousarray(pool[np.arange(n_pairs) % len(pool)])
    res = batch.solve_edge(recs)
    # every record equals itself solved alone (first occurrence), bit for bit
    for k in range(min(n_pairs, len(pool))):
        one = batch.solve_edge(recs[k:k + 1]) if k < 3 else None
        if one is not None:
            np.testing.assert_array_equal(one.raw[0], res.raw[k])
            np.testing.assert_array_equal(one.status[0], res.status[k])
    for k in range(len(pool), n_pairs):
        np.testing.assert_array_equal(res.raw[k], res.raw[k % len(pool)])
    _compare(res, recs[:min(n_pairs, 4)], f"shape{n_pairs}", kkt=False)


def test_position_in_batch_and_workgroup_does_not_matter(batch):
    pool = np.concatenate([E.case_set("exchanged"), E.case_set("pressed")])
    alone = batch.solve_edge(pool[:1])
    recs = []
    for k in range(64):
        recs.append(pool[0])
        if k % 3 != 2:          # irregular spacing: the copies land on every wave slot of a workgroup
            recs.append(pool[1 + k % (len(pool) - 1)])
    recs = np.ascontiguousarray(np.stack(recs))
    res = batch.solve_edge(recs)
    n = 0
    for k, rec in enumerate(recs):
        if np.array_equal(rec, pool[0]):
            n += 1
            np.testing.assert_array_equal(res.raw[k], alone.raw[0])
            np.testing.assert_array_equal(res.status[k], alone.status[0])
            np.testing.assert_array_equal(res.iters[k], alone.iters[0])
    assert n == 64


def test_edge_call_leaves_the_resident_local_batch_alone(batch):
    recs = obca.scenario_batch(40, seed=3)
    want = batch.solve(recs)
    batch.upload(recs)
    batch.run_async(1)
    batch.solve_edge(E.case_set("pressed"))
    got = batch.download(len(recs))
    np.testing.assert_array_equal(got.raw, want.raw)
    np.testing.assert_array_equal(got.status, want.status)
    # and between upload and the run
    batch.upload(recs)
    batch.solve_edge(E.case_set("bounds"))
    batch.run_async(1)
    got = batch.download(len(recs))
    np.testing.assert_array_equal(got.raw, want.raw)


def test_errors_are_reported_before_any_launch(batch):
    rec = E.case_set("consistent")[:2]
    # rho, prob, max_iter, start; min_dis and g_max not finite
    for off, val in ((0, 0.0), (2, 2.0), (3, 0.0), (5, 2.0), (1, np.nan), (1, np.inf), (8, np.nan), (8, -np.inf)):
        bad = rec.copy()
        bad[1, obca._E_PAR + off] = val
        with pytest.raises(_lib.PiadmmError, match="record 1: bad parameters"):
            batch.solve_edge(bad)
    r = batch.solve_edge(rec)
    assert np.all(r.status == 0)


# ---------------------------------------------------------------------------------------------
# the hard branches (tests/_obca_edge_cases.py, proved on the CPU by tests/test_obca_edge_cases.py):
# the Hessian modification with its two ladders, the QP's drops, the upper range row, solves from
# zeros, rho / min_dis / round_decimals off their defaults -- on the slots the stability filter keeps
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", K.SET_NAMES)
def test_gpu_equals_restatement_on_the_hard_branches(batch, name):
    recs = K.case_set(name)
    res = batch.solve_edge(recs)
    _compare(res, recs, name, keep=set(K.kept(name)))


def test_rounding_at_other_decimals(batch):
    recs = K.case_set("decimals")
    res = batch.solve_edge(recs)
    n, skipped, seen, keep = 0, 0, set(), set(K.kept("decimals"))
    for k, rec in enumerate(recs):
        for t, (p, r) in enumerate(E.solve_record(rec)):
            if (k, t) not in keep:
                continue
            assert res.status[k, t] == r.status
            d = p.round_decimals
            seen.add(d)
            x = r.z * 10.0 ** d
            # within 1e-2 of the decimal's grid spacing of a rounding tie (test_rounding's window at d = 4)
            tie = np.abs(np.abs(x - np.floor(x)) - 0.5) < 1e-2
            want = np.round(r.z, d)
            got = np.concatenate([res.Z_bar[k, 0, t], res.Z_bar[k, 1, t]])
            n += x.size
            skipped += int(tie.sum())
            np.testing.assert_array_equal(got[~tie], want[~tie], err_msg=f"decimals {d}: record {k} slot {t}")
    assert seen == set(K.DECIMALS)
    print(f"rounding at {sorted(seen)} decimals: {skipped} of {n} values within 1e-2 grid steps of a tie")
    assert skipped <= 0.05 * n
    # the solve does not see the field
    for j in range(0, len(recs), len(K.DECIMALS)):
        for i in range(1, len(K.DECIMALS)):
            np.testing.assert_array_equal(res.Z[j + i], res.Z[j])


@pytest.mark.parametrize("name", ["soft_rho", "stiff_rho"])
def test_fused_dual_update_off_unit_rho(batch, name):
    recs = K.case_set(name)
    assert np.all(recs[:, obca._E_PAR] != 1.0)
    _check_dual_update(batch.solve_edge(recs), recs)


def _long_and_short():
    """soft_rho records with a slot that runs all 60 SQP iterations, consistent records (2 each)."""
    long_ = [rec for rec in K.case_set("soft_rho") if any(r.iters == 60 for _, r in E.solve_record(rec))]
    short = list(E.case_set("consistent")[:5])
    assert len(long_) >= 3 and all(r.iters == 2 for rec in short for _, r in E.solve_record(rec))
    recs, who = [], []
    for k in range(36):
        recs.append(long_[k % len(long_)])
        who.append(("long", k % len(long_)))
        if k % 3 != 2:          # irregular spacing: long and short solves share workgroups in every arrangement
            recs.append(short[k % len(short)])
            who.append(("short", k % len(short)))
    return long_, short, np.ascontiguousarray(np.stack(recs)), who


def test_long_and_short_solves_interleaved(batch):
    long_, short, recs, who = _long_and_short()
    alone = {("long", i): batch.solve_edge(np.ascontiguousarray(rec[None])) for i, rec in enumerate(long_)}
    alone.update({("short", i): batch.solve_edge(np.ascontiguousarray(rec[None])) for i, rec in enumerate(short)})
    assert all(alone["long", i].iters.max() == 60 for i in range(len(long_)))
    assert all(alone["short", i].iters.max() == 2 for i in range(len(short)))
    res = batch.solve_edge(recs)
    for k, key in enumerate(who):
        np.testing.assert_array_equal(res.raw[k], alone[key].raw[0], err_msg=f"{k} {key}")
        np.testing.assert_array_equal(res.status[k], alone[key].status[0])
        np.testing.assert_array_equal(res.iters[k], alone[key].iters[0])
        np.testing.assert_array_equal(res.qp_steps[k], alone[key].qp_steps[0])


def test_hard_branches_repeat_bit_for_bit(batch):
    recs = np.concatenate([_long_and_short()[2], K.case_set("tight_mu"), K.case_set("cold_start")])
    a, b = batch.solve_edge(recs), batch.solve_edge(recs)
    np.testing.assert_array_equal(a.raw, b.raw)
    for x, y in ((a.status, b.status), (a.iters, b.iters), (a.qp_steps, b.qp_steps)):
        np.testing.assert_array_equal(x, y)


# ---------------------------------------------------------------------------------------------
# the planner, teacher-forced: every stage's GPU output against the restatement applied to that
# stage's GPU inputs (a free-running comparison of a nonconvex loop would test chaos, not code)
# ---------------------------------------------------------------------------------------------
def test_planner_teacher_forced(batch):
    # the issue's two scenarios (prob 1 and 0) and a third whose thresholds let it stop at its first
    # iterate: the scenarios provably stop at different iterates, and both cases of the :87 shift
    # (the start-of-step state, the previous iterate's state) occur
    stages = []
    pl = obca.OBCAPlanner(batch, n_scenarios=3, prob=[1, 0, 1], t_step0=12, max_admm_iter=2, round_decimals=-1,
                          primal_thres=[0.01, 0.01, np.inf], dual_thres=[0.01, 0.01, np.inf],
                          on_stage=lambda name, inp, outp: stages.append((name, inp, outp)))
    rec = pl.run(2)
    names = [s[0] for s in stages]
    assert set(names) == {"local", "exchange", "converge", "edge", "residual", "shift"}
    for name, inp, outp in stages:
        if name == "local":
            C.compare(outp["result"], C.oracle(inp["recs"]))
        elif name == "exchange":
            for k, s in enumerate(inp["scenarios"]):
                want = obca.bar_state_update(inp["bar"][k], inp["fullx"][k], prob=pl.prob[s])
                for key in ("A", "b", "local_x", "lamb_ij"):
                    np.testing.assert_array_equal(outp["bar"][k][key], want[key])
        elif name == "converge":
            for k in range(len(inp["bar"])):
                assert outp["if_converge"][k] == obca.check_converge(inp["bar"][k], 0.1, pl.min_dis)
        elif name == "edge":
            _compare(outp["result"], inp["recs"], "planner", kkt=False)
            for k, r in enumerate(inp["recs"]):
                ref = E.edge_step(r)
                np.testing.assert_array_equal(outp["result"].status[k], ref["status"])
                np.testing.assert_allclose(outp["result"].lamb_bar[k], ref["lamb_bar"], rtol=RTOL, atol=ATOL)
        elif name == "residual":
            for k, s in enumerate(inp["scenarios"]):
                want_p = np.abs(inp["ctrl"][k] - inp["ctrl_prev"][k]).sum()
                want_d = np.abs(inp["lamb_bar"][k] - inp["lamb_bar_prev"][k]).sum()
                assert abs(outp["primal"][k] - want_p) <= 1e-12 * max(1.0, want_p)
                assert abs(outp["dual"][k] - want_d) <= 1e-12 * max(1.0, want_d)
                stop = (want_p <= pl.primal_thres[s] and want_d <= pl.dual_thres[s]) or inp["i_iter"] > pl.max_admm_iter
                assert bool(outp["stop"][k]) == bool(stop)
    # the :87 shift (B16), no resubmission of a stopped scenario, init_state = X[1], the hand-over
    iters = E.check_planner_structure(pl, stages, rec, 12)
    assert np.all(iters[:, 2] == 1) and np.all(iters[:, :2] >= 2)      # they stop at different iterates
    for name, inp, outp in stages:
        if name == "local" and inp["i_iter"] > 1:
            assert 2 not in inp["scenarios"]
    # the run record
    assert np.asarray(rec.state_record).shape == (3, 3, 2, 5)
    assert np.asarray(rec.iter_num_record).shape == (2, 3)
    assert np.asarray(rec.lambda_record).shape == (2, 3, 2, obca.NT, 9)
    assert np.all(np.asarray(rec.iter_num_record) <= 3)
    assert len(rec.status_record) == names.count("local")


def test_planner_update_lamb_ij_takes_the_local_lambda(batch):
    stages = []
    pl = obca.OBCAPlanner(batch, n_scenarios=2, prob=[1, 0], t_step0=12, max_admm_iter=0, update_lamb_ij=1,
                          on_stage=lambda name, inp, outp: stages.append((name, inp, outp)))
    pl.run(1)
    exch = [s for s in stages if s[0] == "exchange"]
    assert len(exch) == 1
    _, inp, outp = exch[0]
    for k in range(2):
        for v in (0, 1):
            np.testing.assert_array_equal(outp["bar"][k]["lamb_ij"][v], inp["fullx"][k][v][:, 5:])
        assert not np.array_equal(outp["bar"][k]["lamb_ij"], inp["bar"][k]["lamb_ij"])
    # and the edge stage read it
    edge = [s for s in stages if s[0] == "edge"][0]
    for k in range(2):
        np.testing.assert_array_equal(obca.edge_unpack(edge[1]["recs"][k])["lamb_ij"], outp["bar"][k]["lamb_ij"])
