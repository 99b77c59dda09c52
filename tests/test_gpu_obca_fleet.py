"""The device-resident OBCA-ADMM loop with a reference and a parameter row per scenario
(piadmm_obca_fleet_begin, piadmm.obca.OBCADevicePlanner with specs= / sequences), by the method
of tests/test_gpu_obca_plan.py: teacher-forced, every stage's device output against the host
function applied to that stage's device input with the SCENARIO'S OWN row and reference; the two
solves replayed on a second handle.

Bars (those of tests/test_gpu_obca_plan.py; the positions are of the same size, |x| + |y| <= 170).
Copies, records, the replayed solves, the dual residual, the shift: bit-equal.  A: 1e-15, b: 1e-12
absolute.  Flags are compared where the host value stands at least 1e-9 from its threshold; the
closer ones are counted and the count must be 0.

The reference-end test runs on references of 10 rows from t_step0 = 0.  The rule of
piadmm_obca_plan_iterate is unchanged (a step needs rows t_step .. t_step + 7, so it runs while
t_step + 8 <= n_ref): steps 0, 1 and 2 run, each checked for its window, and the step after
them is the one refused."""
import ctypes

import numpy as np
import pytest

import _obca_fleet_cases as F
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

MARGIN = 1e-9


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
    """One MPC step of the fleet `pl` iterate by iterate, every stage checked with scenario s's own
    parameters (pl.<name>_s[s]) and reference (pl.ref_traj_s[s]); returns the stop iterates."""
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
        want = np.stack([obca.local_record(bar_in[k][0], v, t_step, bar_in[k][1][v], pl.ref_traj_s[s], rho=pl.rho_s[s],
                                           min_dis=pl.min_dis_s[s], prob=pl.prob[s], max_x=pl.max_x_s[s],
                                           max_y=pl.max_y_s[s], r=pl.r_s[s], q=pl.q_s[s], max_iter=pl.max_iter_s[s])
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
        # ---- check_converge of the device's own bar, at the scenario's conv_thres and min_dis ----
        conv = pl.get("CONVERGE")
        for k, s in enumerate(act):
            if _converge_margin(bar_ex[k], pl.conv_thres_s[s], pl.min_dis_s[s]) < MARGIN:
                stats["near"] += 1
                continue
            assert bool(conv[s]) == obca.check_converge(bar_ex[k], pl.conv_thres_s[s], pl.min_dis_s[s]), (s, i_iter)
            stats["conv_checked"] += 1
        # ---- the edge record and the edge solve ----
        erecs = pl.get("EDGE_REC")
        want = np.stack([obca.edge_record(bar_ex[k], rho=pl.rho_s[s], min_dis=pl.min_dis_s[s], prob=pl.prob[s],
                                          max_iter=pl.max_iter_s[s], round_decimals=pl.round_decimals_s[s],
                                          start=pl.start_s[s], x_bound=pl.x_bound_s[s], mu_max=pl.mu_max_s[s],
                                          g_max=pl.g_max_s[s])
                         for k, s in enumerate(act)])
        _bits(erecs, want, "EDGE_REC")
        eres = ref.solve_edge(erecs)
        _bits(pl.get("EDGE_OUT"), eres.raw, "EDGE_OUT")
        _bits(pl.get("EDGE_IST"), np.stack([eres.status, eres.iters, eres.qp_steps], axis=2), "EDGE_IST")
        # ---- residual: the stop rule at the scenario's own max_admm_iter ----
        primal, dual, stop, iters = pl.get("PRIMAL"), pl.get("DUAL"), pl.get("STOP"), pl.get("ITERS")
        _bits(dual[act], eres.dual_residual(), "DUAL")
        nxt = []
        for k, s in enumerate(act):
            dev = obca.unpack_state(after[s])[0]
            _bits(dev["Z_bar"], eres.Z_bar[k], "Z_bar")
            _bits(dev["lamb_bar"], eres.lamb_bar[k], "lamb_bar")
            want_p = float(np.abs(ctrl[s] - ctrlp_before[s]).sum())
            assert abs(primal[s] - want_p) <= 1e-12 * max(1.0, want_p), (s, primal[s], want_p)
            forced = i_iter > pl.max_admm_iter_s[s]
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


# 1 ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("t_step0", F.T_STEPS)
def test_stage_parity(batches, t_step0):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, **F.fleet_kwargs(range(4), t_step0))
    assert pl.fleet
    stats = dict(dA=0.0, db=0.0, near=0, conv_checked=0, stop_checked=0)
    iters = np.stack([teacher_forced_step(pl, ref, stats) for _ in range(2)])
    print(f"fleet stage parity (t_step0 {t_step0}): max |dA| {stats['dA']:.2e}  max |db| {stats['db']:.2e}  flags "
          f"checked {stats['conv_checked']} + {stats['stop_checked']}, within 1e-9 of a threshold {stats['near']}")
    assert stats["near"] == 0
    assert stats["conv_checked"] > 0 and stats["stop_checked"] > 0
    assert iters.tolist() == [F.STOP_ITERS, F.STOP_ITERS]
    pl.close()


# 2 ------------------------------------------------------------------------------------------
def test_a_fleet_of_the_shared_configuration_equals_the_shared_plan(batches):
    b, _ = batches
    n = 6
    kw = dict(n_scenarios=n, prob=[k % 2 for k in range(n)], t_step0=12, max_admm_iter=2, round_decimals=-1,
              primal_thres=[0.01, 0.01, np.inf] * 2, dual_thres=[0.01, 0.01, np.inf] * 2, rho=1.5, min_dis=0.2,
              x_bound=800.0)
    refs = np.stack([np.stack(obca.ref_traj_gen())] * n)
    got = {}
    for kind, extra in (("shared", {}), ("fleet", dict(ref_traj=refs))):
        pl = obca.OBCADevicePlanner(b, **kw, **extra)
        assert pl.fleet == (kind == "fleet")
        assert pl.iterate() >= 0
        got[kind] = dict(LOCAL_REC=pl.get("LOCAL_REC"), EDGE_REC=pl.get("EDGE_REC"))
        pl.close()
        pl = obca.OBCADevicePlanner(b, **kw, **extra)
        pl.step()
        got[kind].update({k: pl.get(k) for k in ("STATE", "STATE_PREV", "X", "ITERS", "LAMBDA")})
        pl.close()
    for key in got["shared"]:
        _bits(got["fleet"][key], got["shared"][key], key)
    assert got["shared"]["ITERS"].max() > 1


# 3 ------------------------------------------------------------------------------------------
def _final(pl):
    return dict(STATE=pl.get("STATE"), X=pl.get("X"), ITERS=pl.get("ITERS"),
                iter_num_record=np.asarray(pl.record.iter_num_record))


@pytest.fixture(scope="module")
def alone(batches):
    """Each of the four cases run alone for 2 MPC steps (computed once, never changed)."""
    b, _ = batches
    out = []
    for c in range(4):
        pl = obca.OBCADevicePlanner(b, **F.single_kwargs(c, 12))
        assert pl.fleet                         # a spec makes it one, also at n = 1
        pl.run(2)
        out.append(_final(pl))
        pl.close()
    return out


@pytest.mark.parametrize("n", [1, 5, 70])
def test_position_independence(batches, alone, n):
    b, _ = batches
    cases = [k % 4 for k in range(n)]
    pl = obca.OBCADevicePlanner(b, **F.fleet_kwargs(cases, 12))
    pl.run(2)
    got = _final(pl)
    pl.close()
    for k, c in enumerate(cases):
        for key in ("STATE", "X", "ITERS"):
            _bits(got[key][k], alone[c][key][0], f"{key} of scenario {k}")
        _bits(got["iter_num_record"][:, k], alone[c]["iter_num_record"][:, 0], f"stop iterates of scenario {k}")
    assert got["iter_num_record"].tolist() == [[F.STOP_ITERS[c] for c in cases]] * 2


# 4 ------------------------------------------------------------------------------------------
def test_reference_stride_and_the_end_of_the_reference(batches):
    b, _ = batches
    cases = [0, 1, 2, 3, 1]
    kw = F.fleet_kwargs(cases, 0)
    refs = np.stack([np.stack(obca.ref_traj_gen(sp))[:, :10] for sp in kw["specs"]])
    refs[:, :, :, 1] += 0.001 * np.arange(len(cases))[:, None, None]      # no two references alike
    refs = np.ascontiguousarray(refs)
    assert refs.shape == (5, 2, 10, 5)
    pl = obca.OBCADevicePlanner(b, ref_traj=refs, **kw)
    assert pl.n_ref == 10
    _bits(pl.get("REF"), refs, "REF")
    steps = 0
    while pl.t_step + 8 <= 10:
        t = pl.t_step
        assert pl.iterate() >= 0
        recs, act = pl.get("LOCAL_REC"), pl.get("ACTIVE")
        assert act.tolist() == list(range(5))
        for k, s in enumerate(act):
            for v in (0, 1):
                _bits(obca.unpack(recs[2 * k + v])["ref"], refs[s, v, t:t + 8], f"window {t} {s} {v}")
        while pl.counts()[1]:
            pl.iterate()
        pl.shift()
        pl.t_step += 1
        steps += 1
    assert steps == 3 and int(pl.get("T_STEP")[0]) == 3
    iters = np.zeros(5, np.int32)
    rc = b._lib.piadmm_obca_plan_step(b._h, _lib.iptr(iters))
    assert rc == _lib.E_STATE and b"reference exhausted" in b._lib.piadmm_obca_last_error(b._h)
    with pytest.raises(_lib.PiadmmError, match="reference exhausted"):
        pl.iterate()
    # the plan stays open
    assert pl.counts() == (0, 5, 0) and pl.get("STATE").shape == (5, obca.PLAN_STATE)
    pl.close()


# 5 ------------------------------------------------------------------------------------------
def test_plan_step_equals_stepping_by_hand_and_ref_par_come_back(batches):
    b, _ = batches
    kw = F.fleet_kwargs(range(4), 12)
    pl = obca.OBCADevicePlanner(b, **kw)
    seen = []
    for _ in range(2):
        n_it = 0
        while True:
            n_it += 1
            if pl.iterate() == 0:
                break
        assert n_it == max(F.ROWS["max_admm_iter"]) + 1
        seen.append(pl.get("ITERS"))
        pl.shift()
    hand = dict(STATE=pl.get("STATE"), X=pl.get("X"), ITERS=np.stack(seen))
    pl.close()
    pl = obca.OBCADevicePlanner(b, **kw)
    rec = pl.run(2)
    _bits(pl.get("STATE"), hand["STATE"], "STATE")
    _bits(pl.get("X"), hand["X"], "X")
    _bits(np.asarray(rec.iter_num_record, np.int32), hand["ITERS"], "ITERS")
    assert hand["ITERS"].tolist() == [F.STOP_ITERS, F.STOP_ITERS]
    # what was passed comes back, one row per scenario
    ref, par = pl.get("REF"), pl.get("PAR")
    _bits(ref, np.stack([np.stack(obca.ref_traj_gen(sp)) for sp in F.SPECS]), "REF")
    assert par.shape == (4, 16)
    _bits(par, pl.par, "PAR")
    for j, name in enumerate(obca.FLEET_ROW):
        want = F.ROWS.get(name, [getattr(pl, name + "_s")[0]] * 4)
        assert par[:, j].tolist() == [float(x) for x in want], name
    assert not par[:, 14:].any()
    assert par[:, 10].tolist() == [2.0, 2.0, 1.0, 2.0] and par[:, 11].tolist() == [60.0] * 4
    pl.close()
    # a plan from piadmm_obca_plan_begin: the one shared row and reference
    pl = obca.OBCADevicePlanner(b, n_scenarios=3, prob=[1, 0, 1], t_step0=12, rho=1.5, max_admm_iter=1)
    assert not pl.fleet
    ref, par = pl.get("REF"), pl.get("PAR")
    _bits(ref, np.stack(obca.ref_traj_gen())[None], "REF of a shared plan")
    assert par.tolist() == [[1.5, 0.1, 0.1, 150.0, 20.0, 1e4, 1e5, 1000.0, 1e5, 1000.0, 1.0, 60.0, 4.0, 1.0, 0.0, 0.0]]
    bad = np.zeros((3, 16))
    assert b._lib.piadmm_obca_plan_get(b._h, obca.PLAN_GET["PAR"][0], bad.ctypes.data, bad.nbytes) == _lib.E_ARG
    pl.close()


# 6 ------------------------------------------------------------------------------------------
def test_refusals_before_any_launch():
    """Every refusal is judged before a device call: on a fresh handle no plan opens (a following
    plan_get is PIADMM_E_STATE), and the row is named.  (A NULL ref_traj has no row to name.)"""
    fresh = obca.OBCABatch(0)
    lib = fresh._lib
    probe = np.zeros(3, np.int32)

    def no_plan():
        rc = lib.piadmm_obca_plan_get(fresh._h, obca.PLAN_GET["COUNTS"][0], probe.ctypes.data, probe.nbytes)
        assert rc == _lib.E_STATE

    for name, value in (("rho", 0.0), ("max_iter", 2.5), ("start", 2), ("round_decimals", 16), ("max_admm_iter", -1)):
        kw = F.fleet_kwargs(range(4), 12)
        kw.setdefault(name, [dict(max_iter=60, start=1).get(name)] * 4)
        kw[name] = list(kw[name])
        kw[name][2] = value
        with pytest.raises(_lib.PiadmmError, match=r"obca_fleet_begin: row 2: ") as ei:
            obca.OBCADevicePlanner(fresh, **kw)
        assert ei.value.code == _lib.E_ARG, name
        no_plan()
    # a NULL ref_traj, through the C-ABI
    n = 2
    cfg = _lib.ObcaPlanCfgC(n_scenarios=n, t_step0=12, update_lamb_ij=0, n_ref=51)
    prob, thr = np.array([1, 0], np.int32), np.full(n, 0.01)
    par = np.tile([1.0, 0.1, 0.1, 150.0, 20.0, 1e4, 1e5, 1000.0, 1e5, 1000.0, 2.0, 60.0, 4.0, 1.0, 0.0, 0.0], (n, 1))
    state = np.stack([obca.pack_state(obca.seeded_bar_state(12, int(p)),
                                      np.stack([obca.executed_path(v, 1.2) for v in (0, 1)])) for p in prob])
    refs = np.ascontiguousarray(np.stack([np.stack(obca.ref_traj_gen())] * n))
    args = [fresh._h, ctypes.byref(cfg), _lib.iptr(prob), _lib.dptr(thr), _lib.dptr(thr), None, _lib.dptr(par),
            _lib.dptr(state)]
    assert lib.piadmm_obca_fleet_begin(*args) == _lib.E_ARG
    assert b"obca_fleet_begin" in lib.piadmm_obca_last_error(fresh._h)
    no_plan()
    # the same call with the reference opens the plan; a refused call afterwards leaves it open
    args[5] = _lib.dptr(refs)
    assert lib.piadmm_obca_fleet_begin(*args) == 0
    par[1, 0] = -1.0
    assert lib.piadmm_obca_fleet_begin(*args) == _lib.E_ARG
    assert b"row 1" in lib.piadmm_obca_last_error(fresh._h)
    assert lib.piadmm_obca_plan_get(fresh._h, obca.PLAN_GET["COUNTS"][0], probe.ctypes.data, probe.nbytes) == 0
    assert probe.tolist() == [0, n, 0]
    # and a NULL table runs every scenario on the configuration's row
    cfg2 = _lib.ObcaPlanCfgC(n_scenarios=n, t_step0=12, max_admm_iter=1, round_decimals=4, start=1, update_lamb_ij=0,
                             max_sqp_iter=60, n_ref=51, rho=1.0, min_dis=0.1, conv_thres=0.1, max_x=150.0, max_y=20.0,
                             r=1e4, q=1e5, x_bound=1000.0, mu_max=1e5, g_max=1000.0)
    args[1], args[6] = ctypes.byref(cfg2), None
    assert lib.piadmm_obca_fleet_begin(*args) == 0
    back = np.zeros((n, 16))
    assert lib.piadmm_obca_plan_get(fresh._h, obca.PLAN_GET["PAR"][0], back.ctypes.data, back.nbytes) == 0
    assert back.tolist() == [[1.0, 0.1, 0.1, 150.0, 20.0, 1e4, 1e5, 1000.0, 1e5, 1000.0, 1.0, 60.0, 4.0, 1.0, 0.0, 0.0]] * n
    assert lib.piadmm_obca_plan_end(fresh._h) == 0
    fresh.close()


# 7 ------------------------------------------------------------------------------------------
def test_first_iterate_equals_the_host_planner(batches):
    b, ref = batches
    host_stages, dev_stages = [], []
    kw = F.fleet_kwargs(range(4), 12)
    hp = obca.OBCAPlanner(ref, on_stage=lambda *a: host_stages.append(a), **kw)
    dp = obca.OBCADevicePlanner(b, on_stage=lambda *a: dev_stages.append(a), **kw)
    hrec, drec = hp.run(2), dp.run(2)
    h0 = [s for s in host_stages if s[0] == "local"][0]
    d0 = [s for s in dev_stages if s[0] == "local"][0]
    assert h0[1]["i_iter"] == d0[1]["i_iter"] == 1 and h0[1]["scenarios"] == d0[1]["scenarios"] == [0, 1, 2, 3]
    _bits(d0[1]["recs"], h0[1]["recs"], "first local records")
    _bits(d0[2]["result"].raw, h0[2]["result"].raw, "first local outputs")
    _bits(d0[2]["result"].status, h0[2]["result"].status, "first local status")
    # from here the runs part in the last bits of A: information only
    dev = float(np.abs(np.asarray(drec.state_record) - np.asarray(hrec.state_record)).max())
    print(f"fleet free-running: max |state_record(device) - state_record(host)| after 2 steps {dev:.3e}; "
          f"iterates host {np.asarray(hrec.iter_num_record).tolist()} device {np.asarray(drec.iter_num_record).tolist()}")
    dp.close()
