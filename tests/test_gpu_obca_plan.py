"""The device-resident OBCA-ADMM consensus loop (csrc/piadmm_obca_plan.hip behind
piadmm_obca_plan_*, piadmm.obca.OBCADevicePlanner), teacher-forced: every stage's device output
against the repository's own host function applied to that stage's device input, both read with
piadmm_obca_plan_get.  A free-running comparison of this nonconvex loop would test chaos, not
code (tests/test_gpu_obca_edge.py); the two solves are replayed on a second handle.

Bars.  Copies (records, local_x, lamb_ij, Z_bar, lamb_bar, the shift) and the replayed solves:
bit-equal.  A: 1e-15 absolute (host and device sin / cos each within a few ulp of a value <= 1).
b: 1e-12 absolute (|db| <= 2 (|x| + |y|) |dA| + rounding, |x| + |y| <= max_x + max_y = 170).
The dual residual: bit-equal (the 7 partials added in index order); the primal one:
1e-12 max(1, value).  Flags (check_converge, stop) are compared where the host value stands at
least 1e-9 from its threshold; closer ones are counted and the count must be 0."""
import ctypes

import numpy as np
import pytest

import _obca_edge_ref as E
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

MARGIN = 1e-9
SETUP = dict(prob=[1, 0, 1], t_step0=12, max_admm_iter=2, round_decimals=-1,
             primal_thres=[0.01, 0.01, np.inf], dual_thres=[0.01, 0.01, np.inf])


@pytest.fixture(scope="module")
def batches():
    """(the handle under test, a second handle that replays the solves)."""
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    b, ref = obca.OBCABatch(0), obca.OBCABatch(0)
    yield b, ref
    b.close()
    ref.close()


def _bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (msg, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), (msg, float(np.nanmax(np.abs(a.astype(float) - b.astype(float)))))


def _converge_margin(bar, thres, min_dis):
    eq = np.einsum("tij,ti->tj", bar["A"][0], bar["lamb_ij"][0]) + np.einsum("tij,ti->tj", bar["A"][1], bar["lamb_ij"][1])
    ueq = -np.einsum("ti,ti->t", bar["b"][0], bar["lamb_ij"][0]) - np.einsum("ti,ti->t", bar["b"][1], bar["lamb_ij"][1])
    return min(float(np.abs(np.abs(eq) - thres).min()), float(np.abs(ueq - min_dis).min()))


def teacher_forced_step(pl, ref, stats):
    """One MPC step of `pl` iterate by iterate, every stage checked; returns the stop iterates."""
    n, t_step = pl.n, pl.t_step
    assert int(pl.get("T_STEP")[0]) == t_step
    expect_active = list(range(n))
    stopped = set()
    i_iter = 0
    while expect_active:
        i_iter += 1
        before, prev_before = pl.get("STATE"), pl.get("STATE_PREV")
        ctrlp_before = pl.get("CTRL_PREV")
        if i_iter == 1:
            _bits(before, prev_before, "a step starts with both states equal")
            assert not ctrlp_before.any()
        left = pl.iterate()
        act = [int(s) for s in pl.get("ACTIVE")]
        assert act == expect_active and not stopped & set(act)
        assert pl.counts()[0] == len(act) and pl.counts()[2] == i_iter
        after, prev_after = pl.get("STATE"), pl.get("STATE_PREV")
        bar_in = [obca.unpack_state(before[s]) for s in act]
        # ---- pack-local ----
        recs = pl.get("LOCAL_REC")
        want = np.stack([obca.local_record(bar_in[k][0], v, t_step, bar_in[k][1][v], pl.ref_traj, rho=pl.rho,
                                           min_dis=pl.min_dis, prob=pl.prob[s], max_iter=pl.max_iter)
                         for k, s in enumerate(act) for v in (0, 1)])
        _bits(recs, want, "LOCAL_REC")
        # ---- local solve, replayed on the second handle ----
        res = ref.solve(recs)
        _bits(pl.get("LOCAL_OUT"), res.raw, "LOCAL_OUT")
        _bits(pl.get("LOCAL_IST"), np.stack([res.status, res.iters, res.qp_steps], axis=1), "LOCAL_IST")
        # ---- exchange ----
        bar_ex = []
        for k, s in enumerate(act):
            fullx = [res.bar_fullx(2 * k + v) for v in (0, 1)]
            host = obca.bar_state_update(bar_in[k][0], fullx, prob=pl.prob[s])
            if pl.update_lamb_ij:
                host["lamb_ij"] = np.stack([fullx[v][:, 5:] for v in (0, 1)])
            dev, init = obca.unpack_state(after[s])
            _bits(dev["local_x"], host["local_x"], "local_x")
            _bits(dev["lamb_ij"], host["lamb_ij"], "lamb_ij")
            _bits(init, bar_in[k][1], "init_state stays")
            dA, db = float(np.abs(dev["A"] - host["A"]).max()), float(np.abs(dev["b"] - host["b"]).max())
            stats["dA"], stats["db"] = max(stats["dA"], dA), max(stats["db"], db)
            assert dA <= 1e-15 and db <= 1e-12, (s, i_iter, dA, db)
            dev["Z_bar"], dev["lamb_bar"] = bar_in[k][0]["Z_bar"], bar_in[k][0]["lamb_bar"]
            bar_ex.append(dev)
        ctrl, X = pl.get("CTRL"), pl.get("X")
        for k, s in enumerate(act):
            for v in (0, 1):
                _bits(ctrl[s, v], np.append(res.U[2 * k + v][:, 0], res.U[2 * k + v][:, 1]), "ctrl")
                _bits(X[s, v], res.X[2 * k + v], "X")
        # ---- check_converge of the device's own bar ----
        conv = pl.get("CONVERGE")
        for k, s in enumerate(act):
            if _converge_margin(bar_ex[k], pl.conv_thres, pl.min_dis) < MARGIN:
                stats["near"] += 1
                continue
            assert bool(conv[s]) == obca.check_converge(bar_ex[k], pl.conv_thres, pl.min_dis), (s, i_iter)
            stats["conv_checked"] += 1
        # ---- the edge record and the edge solve ----
        erecs = pl.get("EDGE_REC")
        want = np.stack([obca.edge_record(bar_ex[k], rho=pl.rho, min_dis=pl.min_dis, prob=pl.prob[s],
                                          max_iter=pl.max_iter, round_decimals=pl.round_decimals, start=pl.start)
                         for k, s in enumerate(act)])
        _bits(erecs, want, "EDGE_REC")
        eres = ref.solve_edge(erecs)
        _bits(pl.get("EDGE_OUT"), eres.raw, "EDGE_OUT")
        _bits(pl.get("EDGE_IST"), np.stack([eres.status, eres.iters, eres.qp_steps], axis=2), "EDGE_IST")
        # ---- residual ----
        primal, dual, stop, iters = pl.get("PRIMAL"), pl.get("DUAL"), pl.get("STOP"), pl.get("ITERS")
        _bits(dual[act], eres.dual_residual(), "DUAL")
        nxt = []
        for k, s in enumerate(act):
            dev = obca.unpack_state(after[s])[0]
            _bits(dev["Z_bar"], eres.Z_bar[k], "Z_bar")
            _bits(dev["lamb_bar"], eres.lamb_bar[k], "lamb_bar")
            want_p = float(np.abs(ctrl[s] - ctrlp_before[s]).sum())
            assert abs(primal[s] - want_p) <= 1e-12 * max(1.0, want_p), (s, primal[s], want_p)
            forced = i_iter > pl.max_admm_iter
            if not forced and min(abs(primal[s] - pl.primal_thres[s]), abs(dual[s] - pl.dual_thres[s])) < MARGIN:
                stats["near"] += 1
                want_stop = bool(stop[s])
            else:
                want_stop = bool((primal[s] <= pl.primal_thres[s] and dual[s] <= pl.dual_thres[s]) or forced)
                assert bool(stop[s]) == want_stop, (s, i_iter, primal[s], dual[s])
                stats["stop_checked"] += 1
            if want_stop:
                assert iters[s] == i_iter
                stopped.add(s)
                _bits(prev_after[s], prev_before[s], "a stopped scenario's previous state is frozen (B16)")
                assert prev_after[s].tobytes() != after[s].tobytes()
            else:
                assert iters[s] == 0
                _bits(prev_after[s], after[s], "a continuing scenario's state becomes the previous one")
                _bits(pl.get("CTRL_PREV")[s], ctrl[s], "ctrl_prev")
                nxt.append(s)
        for s in set(range(n)) - set(act):          # not submitted: untouched
            _bits(after[s], before[s], "STATE of a stopped scenario")
            _bits(prev_after[s], prev_before[s], "STATE_PREV of a stopped scenario")
        assert left == len(nxt) == pl.counts()[1]
        expect_active = nxt
    assert stopped == set(range(n))
    # ---- shift ----
    iters, frozen, X, last = pl.get("ITERS").copy(), pl.get("STATE_PREV"), pl.get("X"), pl.get("STATE")
    pl.shift()
    now, prev = pl.get("STATE"), pl.get("STATE_PREV")
    _bits(now, prev, "the shift fills both states")
    for s in range(n):
        want = obca.pack_state(obca.iterate_next_state(obca.unpack_state(frozen[s])[0]), X[s, :, 1])
        _bits(now[s], want, f"shift {s}")
        _bits(pl.get("LAMBDA")[s], obca.unpack_state(last[s])[0]["lamb_bar"], "LAMBDA")
    assert int(pl.get("T_STEP")[0]) == t_step + 1 and pl.counts() == (0, n, 0)
    assert not pl.get("CTRL_PREV").any()
    pl.t_step += 1
    return iters


def test_stage_parity(batches):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, n_scenarios=3, **SETUP)
    stats = dict(dA=0.0, db=0.0, near=0, conv_checked=0, stop_checked=0)
    iters = np.stack([teacher_forced_step(pl, ref, stats) for _ in range(2)])
    print(f"stage parity: max |dA| {stats['dA']:.2e}  max |db| {stats['db']:.2e}  flags checked "
          f"{stats['conv_checked']} + {stats['stop_checked']}, within 1e-9 of a threshold {stats['near']}")
    assert stats["near"] == 0
    assert stats["conv_checked"] > 0 and stats["stop_checked"] > 0
    # the scenarios stop at different iterates: both cases of the :87 shift occurred
    assert np.all(iters[:, 2] == 1) and np.all(iters[:, :2] >= 2)
    pl.close()


def test_first_iterate_equals_the_host_planner(batches):
    b, ref = batches
    host_stages, dev_stages = [], []
    hp = obca.OBCAPlanner(ref, n_scenarios=3, on_stage=lambda *a: host_stages.append(a), **SETUP)
    dp = obca.OBCADevicePlanner(b, n_scenarios=3, on_stage=lambda *a: dev_stages.append(a), **SETUP)
    hrec, drec = hp.run(2), dp.run(2)
    h0 = [s for s in host_stages if s[0] == "local"][0]
    d0 = [s for s in dev_stages if s[0] == "local"][0]
    assert h0[1]["i_iter"] == d0[1]["i_iter"] == 1 and h0[1]["scenarios"] == d0[1]["scenarios"]
    _bits(d0[1]["recs"], h0[1]["recs"], "first local records")
    _bits(d0[2]["result"].raw, h0[2]["result"].raw, "first local outputs")
    _bits(d0[2]["result"].status, h0[2]["result"].status, "first local status")
    # from here the runs part in the last bits of A: information only
    dev = float(np.abs(np.asarray(drec.state_record) - np.asarray(hrec.state_record)).max())
    print(f"free-running: max |state_record(device) - state_record(host)| after 2 steps {dev:.3e}; "
          f"iterates host {np.asarray(hrec.iter_num_record).tolist()} device {np.asarray(drec.iter_num_record).tolist()}")
    dp.close()


# scenario k of a run = combination k % 6 of (prob, thresholds): a third stops at its first iterate
def _cycle(n):
    prob = [k % 2 for k in range(n)]
    thres = [np.inf if k % 3 == 2 else 0.01 for k in range(n)]
    return dict(prob=prob, primal_thres=thres, dual_thres=thres, t_step0=12, max_admm_iter=1, round_decimals=-1)


def _final(pl):
    return dict(STATE=pl.get("STATE"), X=pl.get("X"), ITERS=pl.get("ITERS"),
                state_record=np.asarray(pl.record.state_record), iter_num_record=np.asarray(pl.record.iter_num_record),
                lambda_record=np.asarray(pl.record.lambda_record))


@pytest.fixture(scope="module")
def alone(batches):
    """Each of the 6 scenario kinds run alone for 2 MPC steps (computed once, never changed)."""
    b, _ = batches
    out = []
    for c in range(6):
        kw = _cycle(6)
        kw = {k: ([v[c]] if isinstance(v, list) else v) for k, v in kw.items()}
        pl = obca.OBCADevicePlanner(b, n_scenarios=1, **kw)
        pl.run(2)
        out.append(_final(pl))
        pl.close()
    return out


@pytest.mark.parametrize("n", [1, 3, 70])
def test_shapes_and_position_independence(batches, alone, n):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, n_scenarios=n, **_cycle(n))
    pl.run(2)
    got = _final(pl)
    pl.close()
    assert got["state_record"].shape == (3, n, 2, 5) and got["iter_num_record"].shape == (2, n)
    assert got["lambda_record"].shape == (2, n, 2, obca.NT, 9)
    for k in range(n):
        one = alone[k % 6]
        for key in ("STATE", "X", "ITERS"):
            _bits(got[key][k], one[key][0], f"{key} of scenario {k}")
        for key in ("state_record", "iter_num_record", "lambda_record"):
            _bits(got[key][:, k], one[key][:, 0], f"{key} of scenario {k}")
    it = got["iter_num_record"]
    stop_first = [k for k in range(n) if k % 3 == 2]
    assert np.all(it[:, stop_first] == 1)                      # the compaction had gaps
    assert np.all(it[:, [k for k in range(n) if k % 3 != 2]] == 2)


def test_plan_step_equals_stepping_by_hand(batches):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, n_scenarios=3, **SETUP)
    seen = []
    for _ in range(2):
        n_it = 0
        while True:
            n_it += 1
            if pl.iterate() == 0:
                break
        assert n_it <= SETUP["max_admm_iter"] + 1
        seen.append(pl.get("ITERS"))
        pl.shift()
    hand = dict(STATE=pl.get("STATE"), X=pl.get("X"), ITERS=np.stack(seen))
    pl.close()
    pl = obca.OBCADevicePlanner(b, n_scenarios=3, **SETUP)
    rec = pl.run(2)
    _bits(pl.get("STATE"), hand["STATE"], "STATE")
    _bits(pl.get("X"), hand["X"], "X")
    _bits(np.asarray(rec.iter_num_record, np.int32), hand["ITERS"], "ITERS")
    _bits(pl.get("ITERS"), hand["ITERS"][1], "ITERS of the last step")
    assert len(rec.status_record) == 2 and np.all(rec.status_record[0]["local_status_mask"] >= 1)
    pl.close()


def test_on_stage_and_the_record(batches):
    b, _ = batches
    stages = []
    pl = obca.OBCADevicePlanner(b, n_scenarios=3, on_stage=lambda *a: stages.append(a), **SETUP)
    rec = pl.run(2)
    names = [s[0] for s in stages]
    assert set(names) == {"local", "exchange", "converge", "edge", "residual", "shift"}
    assert np.asarray(rec.state_record).shape == (3, 3, 2, 5)
    assert np.asarray(rec.iter_num_record).shape == (2, 3)
    assert np.asarray(rec.lambda_record).shape == (2, 3, 2, obca.NT, 9)
    assert len(rec.status_record) == names.count("local")
    # the structure of the loop from the recorded stages alone: B16's shift, no resubmission,
    # init_state = X[1], the hand-over to the next step (the check the host planner passes)
    iters = E.check_planner_structure(pl, stages, rec, 12)
    assert np.all(iters[:, 2] == 1) and np.all(iters[:, :2] >= 2)
    pl.close()


def test_update_lamb_ij_takes_the_local_lambda(batches):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, n_scenarios=2, prob=[1, 0], t_step0=12, max_admm_iter=0, update_lamb_ij=1)
    before = pl.get("STATE")
    assert pl.iterate() == 0
    after = pl.get("STATE")
    res = obca.OBCAResult(pl.get("LOCAL_OUT"), pl.get("LOCAL_IST"))
    erecs = pl.get("EDGE_REC")
    for k in range(2):
        dev = obca.unpack_state(after[k])[0]
        for v in (0, 1):
            _bits(dev["lamb_ij"][v], res.Lam[2 * k + v], "lamb_ij = Lambda")
        assert not np.array_equal(dev["lamb_ij"], obca.unpack_state(before[k])[0]["lamb_ij"])
        _bits(obca.edge_unpack(erecs[k])["lamb_ij"], dev["lamb_ij"], "the edge record carries it")
    pl.shift()
    pl.close()
    # and the whole step, stage by stage.  With lamb_ij = the local Lambda the range row (5a) the
    # local solve holds active puts ueq at min_dis to rounding, so check_converge's flag stands
    # within the margin by construction: those are counted, every other comparison is made.
    pl = obca.OBCADevicePlanner(b, n_scenarios=2, prob=[1, 0], t_step0=12, max_admm_iter=1, update_lamb_ij=1,
                                round_decimals=-1)
    stats = dict(dA=0.0, db=0.0, near=0, conv_checked=0, stop_checked=0)
    teacher_forced_step(pl, ref, stats)
    assert stats["stop_checked"] == 4
    pl.close()


def test_errors_before_any_launch(batches):
    b, ref = batches
    lib = b._lib
    for kw in (dict(rho=0.0), dict(prob=[1, 2]), dict(max_iter=0), dict(start=2), dict(round_decimals=16),
               dict(t_step0=44)):
        args = dict(n_scenarios=2, prob=[1, 0], t_step0=12, max_admm_iter=0)
        args.update(kw)
        with pytest.raises(_lib.PiadmmError, match="obca_plan_begin") as ei:
            obca.OBCADevicePlanner(b, **args)
        assert ei.value.code == _lib.E_ARG
    with pytest.raises(_lib.PiadmmError, match="n_scenarios >= 1"):
        obca.OBCADevicePlanner(b, n_scenarios=0, prob=[], t_step0=12)
    # out of order: no plan yet on a fresh handle; shift while scenarios are active
    fresh = obca.OBCABatch(0)
    left = ctypes.c_int32()
    assert lib.piadmm_obca_plan_iterate(fresh._h, ctypes.byref(left)) == _lib.E_STATE
    assert lib.piadmm_obca_plan_shift(fresh._h) == _lib.E_STATE
    assert lib.piadmm_obca_plan_end(fresh._h) == 0
    fresh.close()
    # a valid plan runs afterwards; the reference runs out instead of being read past its end
    pl = obca.OBCADevicePlanner(b, n_scenarios=2, prob=[1, 0], t_step0=43, max_admm_iter=0)
    assert pl.n_ref == 51
    with pytest.raises(_lib.PiadmmError, match="still active") as ei:
        pl.shift()
    assert ei.value.code == _lib.E_STATE
    bad = np.zeros(5)
    assert lib.piadmm_obca_plan_get(b._h, obca.PLAN_GET["STATE"][0], bad.ctypes.data, bad.nbytes) == _lib.E_ARG
    pl.step()
    assert np.asarray(pl.record.iter_num_record).tolist() == [[1, 1]]
    for call in (pl.step, pl.iterate):
        with pytest.raises(_lib.PiadmmError, match="reference exhausted") as ei:
            call()
        assert ei.value.code == _lib.E_STATE
    # the plan took the buffers over: the resident-batch calls refuse until the next upload
    with pytest.raises(_lib.PiadmmError, match="libpiadmm error -3"):
        b.run_async(1)
    with pytest.raises(_lib.PiadmmError, match="libpiadmm error -3"):
        b.time(1)
    with pytest.raises(_lib.PiadmmError, match="libpiadmm error -3"):
        b.download(4)
    recs = obca.scenario_batch(40, seed=3)
    want = ref.solve(recs)
    got = b.solve(recs)
    _bits(got.raw, want.raw, "solve after a plan")
    _bits(got.status, want.status, "status after a plan")
    b.run_async(1)
    _bits(b.download(len(recs)).raw, want.raw, "the resident batch after a plan")
    # that upload ended the plan
    with pytest.raises(_lib.PiadmmError, match="no open plan") as ei:
        pl.iterate()
    assert ei.value.code == _lib.E_STATE
