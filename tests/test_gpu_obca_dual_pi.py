"""The PI anti-windup dual law of the device-resident OBCA-ADMM plan (k_plan_dual_pi and
k_plan_dual_shift in csrc/piadmm_obca_plan_attach.hip behind piadmm_obca_dual_plan / piadmm_obca_dual_pi;
OBCADevicePlanner(dual=...) / set_dual / clear_dual, OBCABatch.dual_pi), against the host
restatement piadmm.obca.lambda_update_pi / shift_dual.

Bars.  The kernel and the host restatement are the same uncontracted statements: lamb_bar, S, D,
the 7 residual partials, the dual residual and every copy are bit-equal.  Against the plain plan
with kP = 0, kI = rho, windup = 0 (the fused update may be contracted, the law is not):
2^-52 (|rho e| + |lam'|) per entry of lamb_bar, a slot's residual partial within the sum of its
entries' bars.  Stop flags are compared where the host value stands at least 1e-9 from its
threshold; closer ones are counted and the count must be 0.  The gains and the coverage counts are
those of tests/test_obca_dual_pi_host.py (tests/_obca_dual_cases.py)."""
import ctypes

import numpy as np
import pytest

import _obca_dual_cases as C
import _obca_fleet_cases as F
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

SETUP, MARGIN, _bits = P.SETUP, P.MARGIN, P._bits
EPS = 2.0 ** -52
NT = obca.NT
CASES = [0, 1, 2, 3]
PLANS = {"setup": (dict(SETUP, n_scenarios=3), C.GAINS),
         "fleet": (F.fleet_kwargs(CASES, 12), C.fleet_gains(CASES))}


@pytest.fixture(scope="module")
def batches():
    """(the handle under test, a second handle)."""
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    b, ref = obca.OBCABatch(0), obca.OBCABatch(0)
    yield b, ref
    b.close()
    ref.close()


# ---------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------
STATUS_CYCLE = (0, 1, 2, 3, 4, 7, 0)          # all five codes and one value outside them


def _alone_inputs(n, seed):
    rng = np.random.default_rng(seed)
    shp = (n, 2, NT, 9)
    w, zb = rng.standard_normal(shp), rng.standard_normal(shp)
    lamb, S, D = 0.3 * rng.standard_normal(shp), 0.3 * rng.standard_normal(shp), 0.1 * rng.standard_normal(shp)
    status = np.array([[STATUS_CYCLE[(k + t) % 7] for t in range(NT)] for k in range(n)], np.int32)
    return w, zb, lamb, status, S, D


def _alone_gains(kind, n):
    if kind == "shared_windup":
        return obca.dual_rows(n, dict(kP=0.5, kI=1.25, windup_sat=0.6, d_gain=0.5, windup=1))
    if kind == "shared_plain":
        return obca.dual_rows(n, dict(kP=0.5, kI=1.25, windup_sat=0.6, d_gain=0.5, windup=0))
    k = np.arange(n)
    return obca.dual_rows(n, dict(kP=0.1 + 0.05 * (k % 5), kI=0.5 + 0.25 * (k % 4), windup_sat=0.3 + 0.1 * (k % 3),
                                  d_gain=0.25 * (k % 3), windup=k % 2))


def _host_alone(w, zb, lamb, status, gains, S, D):
    n = w.shape[0]
    out = [np.zeros_like(w), np.zeros_like(w), np.zeros_like(w), np.zeros((n, NT))]
    for k in range(n):
        bar = dict(local_x=w[k, :, :, :5], lamb_ij=w[k, :, :, 5:], Z_bar=zb[k], lamb_bar=lamb[k])
        got = obca.lambda_update_pi(bar, S[k], D[k], gains[k % len(gains)], C.wrote_of(status[k]))
        out[0][k], out[1][k], out[2][k], out[3][k] = got[0]["lamb_bar"], got[1], got[2], got[3]
    return out


@pytest.mark.parametrize("n", [1, 5, 70])
@pytest.mark.parametrize("kind", ["shared_windup", "shared_plain", "per_scenario"])
def test_kernel_alone(batches, n, kind):
    b, _ = batches
    w, zb, lamb, status, S, D = _alone_inputs(n, 40 + n)
    assert set(status.ravel()) == {0, 1, 2, 3, 4, 7}
    gains = _alone_gains(kind, n)
    assert len(gains) == (n if kind == "per_scenario" else 1)
    S_in, D_in = S.copy(), D.copy()
    got = b.dual_pi(w, zb, lamb, status, gains, S, D)
    _bits(S, S_in, "the arguments stay")
    want = _host_alone(w, zb, lamb, status, gains, S, D)
    worst = [float(np.abs(g - h).max()) for g, h in zip(got, want)]
    print(f"kernel alone n={n} {kind}: worst |device - host| lamb {worst[0]:.2e} S {worst[1]:.2e} D {worst[2]:.2e} "
          f"dres {worst[3]:.2e}")
    for g, h, name in zip(got, want, ("lamb_out", "S", "D", "dres_out")):
        _bits(g, h, name)
    # both branches ran: written and unwritten slots, clipped and unclipped entries
    wrote = np.isin(status, obca.EDGE_WRITES_ITERATE)
    assert wrote.any() and (~wrote).any()
    assert not got[3][~wrote].any() and np.all(got[3][wrote] > 0.0)
    if kind == "shared_windup":
        m = np.broadcast_to(wrote[:, None, :, None], w.shape)
        assert (np.abs(got[0][m]) == 0.6).any() and (np.abs(got[0][m]) < 0.6).any()
        assert got[2][m].any()
    if kind == "shared_plain":
        assert not got[2][np.broadcast_to(wrote[:, None, :, None], w.shape)].any()
    if n == 70:
        # position independence: every scenario equals its run alone
        for k in range(n):
            one = b.dual_pi(w[k:k + 1], zb[k:k + 1], lamb[k:k + 1], status[k:k + 1], gains[k % len(gains)][None],
                            S[k:k + 1], D[k:k + 1])
            for g, o, name in zip(got, one, ("lamb_out", "S", "D", "dres_out")):
                _bits(g[k], o[0], f"{name} of scenario {k} alone")


# ---------------------------------------------------------------------------------------------
# 2. the plain update recovered
# ---------------------------------------------------------------------------------------------
def _plain_gains(pl):
    return dict(kP=0.0, kI=pl.rho if pl.rho is not None else list(pl.rho_s), windup=0)


@pytest.mark.parametrize("plan", ["setup", "fleet"])
def test_plain_recovered(batches, plan):
    b, ref = batches
    kw = PLANS[plan][0]
    plain, pi = obca.OBCADevicePlanner(ref, **kw), obca.OBCADevicePlanner(b, **kw)
    pi.set_dual(**_plain_gains(pi))
    _bits(pi.get("DUAL_S"), np.stack([obca.unpack_state(v)[0]["lamb_bar"] for v in pi.get("STATE")]),
          "S = lamb_bar when attached")
    assert not pi.get("DUAL_D").any()
    # teacher-forced over one iterate: both start from the same state
    _bits(pi.get("STATE"), plain.get("STATE"), "same start")
    assert plain.iterate() == pi.iterate()
    eo_plain, eo_pi, erec = plain.get("EDGE_OUT"), pi.get("EDGE_OUT"), pi.get("EDGE_REC")
    _bits(erec, plain.get("EDGE_REC"), "same edge records")
    ist = pi.get("EDGE_IST")
    _bits(ist, plain.get("EDGE_IST"), "same edge statuses")
    rp, rq = obca.OBCAEdgeResult(eo_plain, ist), obca.OBCAEdgeResult(eo_pi, ist)
    _bits(rq.Z_bar, rp.Z_bar, "Z_bar")
    worst, worst_d = 0.0, 0.0
    for k in range(pi.n):
        rho = pi.rho_s[k]
        bar = C.bar_of_edge(erec[k], rq.Z_bar[k])
        e = obca.local_z(bar) - bar["Z_bar"]
        bound = EPS * (np.abs(rho * e) + np.abs(rq.lamb_bar[k]))
        diff = np.abs(rq.lamb_bar[k] - rp.lamb_bar[k])
        worst = max(worst, float(diff.max()))
        assert np.all(diff <= bound), (k, float(diff.max()))
        dd = np.abs(rq.dres[k] - rp.dres[k])
        worst_d = max(worst_d, float(dd.max()))
        assert np.all(dd <= bound.sum(axis=(0, 2))), (k, dd)
    sp, sq = plain.get("STATE"), pi.get("STATE")
    for k in range(pi.n):
        _bits(obca.unpack_state(sq[k])[0]["lamb_bar"], rq.lamb_bar[k], "the state takes the law's lamb_bar")
    _bits(pi.get("DUAL_S"), rq.lamb_bar, "kP = 0: S is the dual")
    # free-running over the rest of the step
    while plain.counts()[1]:
        plain.iterate()
    while pi.counts()[1]:
        pi.iterate()
    _bits(pi.get("ITERS"), plain.get("ITERS"), "stop iterates")
    assert pi.get("ITERS").max() == 3
    free = float(np.abs(pi.get("STATE") - plain.get("STATE")).max())
    print(f"plain recovered ({plan}): teacher-forced worst |d lamb_bar| {worst:.2e}, worst |d dres| {worst_d:.2e} "
          f"(state {float(np.abs(sq - sp).max()):.2e}); free-running worst |d STATE| after the step {free:.2e}")
    plain.close()
    pi.close()


# ---------------------------------------------------------------------------------------------
# 3. stage parity with real gains
# ---------------------------------------------------------------------------------------------
def _dual_step(pl, ref, stats, cover):
    """One MPC step iterate by iterate: the law's stage of every iterate against the host functions
    applied to that iterate's device input; returns (stop iterates, the per-iterate history of
    (STATE, DUAL_S, DUAL_D), the last as they stood before the shift)."""
    n = pl.n
    hist = [(pl.get("STATE"), pl.get("DUAL_S"), pl.get("DUAL_D"))]
    expect_active = list(range(n))
    i_iter = 0
    while expect_active:
        i_iter += 1
        before, S0, D0 = hist[-1]
        prev_before, ctrlp_before = pl.get("STATE_PREV"), pl.get("CTRL_PREV")
        left = pl.iterate()
        act = [int(s) for s in pl.get("ACTIVE")]
        assert act == expect_active
        after, prev_after, S1, D1 = pl.get("STATE"), pl.get("STATE_PREV"), pl.get("DUAL_S"), pl.get("DUAL_D")
        erec, eout, eist = pl.get("EDGE_REC"), pl.get("EDGE_OUT"), pl.get("EDGE_IST")
        dev = obca.OBCAEdgeResult(eout, eist)
        # the edge solve replayed: the law touches lamb_bar_new and dres of the edge output alone
        rep = ref.solve_edge(erec)
        _bits(eist[:, :, 0], rep.status, "edge status")
        keep = np.ones(obca.EDGE_OUT, bool)
        keep[obca._EO_LBN:obca._EO_LBN + 126] = False
        keep[obca._EO_DRES:obca._EO_DRES + NT] = False
        _bits(eout[:, keep], rep.raw[:, keep], "the rest of EDGE_OUT")
        primal, dual, stop, iters = pl.get("PRIMAL"), pl.get("DUAL"), pl.get("STOP"), pl.get("ITERS")
        ctrl = pl.get("CTRL")
        nxt = []
        for k, s in enumerate(act):
            row = pl.dual_par[s % len(pl.dual_par)]
            bar = C.bar_of_edge(erec[k], dev.Z_bar[k])
            _bits(bar["lamb_bar"], obca.unpack_state(before[s])[0]["lamb_bar"], "the record carries the old lamb_bar")
            wrote = C.wrote_of(eist[k, :, 0])
            want, Sw, Dw, dres = obca.lambda_update_pi(bar, S0[s], D0[s], row, wrote)
            _bits(dev.lamb_bar[k], want["lamb_bar"], "lamb_bar_new of EDGE_OUT")
            _bits(dev.dres[k], dres, "dres of EDGE_OUT")
            _bits(S1[s], Sw, "DUAL_S")
            _bits(D1[s], Dw, "DUAL_D")
            st = obca.unpack_state(after[s])[0]
            _bits(st["lamb_bar"], want["lamb_bar"], "lamb_bar of STATE")
            _bits(st["Z_bar"], dev.Z_bar[k], "Z_bar of STATE")
            acc = 0.0
            for t in range(NT):
                acc = acc + dres[t]
            assert dual[s] == acc, (s, i_iter, dual[s], acc)
            c = C.coverage(want["lamb_bar"], D0[s], wrote, row)
            tot = cover.setdefault((pl.t_step, i_iter), [0, 0, 0])
            for j in range(3):
                tot[j] += c[j]
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
                _bits(prev_after[s], prev_before[s], "a stopped scenario's previous state is frozen (B16)")
            else:
                _bits(prev_after[s], after[s], "a continuing scenario's state becomes the previous one")
                nxt.append(s)
        for s in set(range(n)) - set(act):          # not submitted: untouched
            _bits(after[s], before[s], "STATE of a stopped scenario")
            _bits(S1[s], S0[s], "DUAL_S of a stopped scenario")
            _bits(D1[s], D0[s], "DUAL_D of a stopped scenario")
        assert left == len(nxt)
        expect_active = nxt
        hist.append((after, S1, D1))
    iters, frozen, X = pl.get("ITERS").copy(), pl.get("STATE_PREV"), pl.get("X")
    last = pl.get("STATE")
    pl.shift()
    now, S2, D2 = pl.get("STATE"), pl.get("DUAL_S"), pl.get("DUAL_D")
    _bits(now, pl.get("STATE_PREV"), "the shift fills both states")
    for s in range(n):
        j = int(iters[s]) - 1                       # the iterate before the stopping one
        _bits(frozen[s], hist[j][0][s], "STATE_PREV is the state before the stopping iterate")
        _bits(now[s], obca.pack_state(obca.iterate_next_state(obca.unpack_state(frozen[s])[0]), X[s, :, 1]), f"shift {s}")
        Sw, Dw = obca.shift_dual(hist[j][1][s], hist[j][2][s])
        _bits(S2[s], Sw, f"DUAL_S after the shift, scenario {s}")
        _bits(D2[s], Dw, f"DUAL_D after the shift, scenario {s}")
        _bits(pl.get("LAMBDA")[s], obca.unpack_state(last[s])[0]["lamb_bar"], "LAMBDA")
    pl.t_step += 1
    return iters, hist


@pytest.mark.parametrize("plan", ["setup", "fleet"])
def test_stage_parity_with_real_gains(batches, plan):
    b, ref = batches
    kw, gains = PLANS[plan]
    pl = obca.OBCADevicePlanner(b, dual=gains, **kw)
    _bits(pl.get("DUAL_PAR"), obca.dual_rows(pl.n, gains), "DUAL_PAR")
    stats, cover = dict(near=0, stop_checked=0), {}
    iters = np.stack([_dual_step(pl, ref, stats, cover)[0] for _ in range(2)])
    print(f"stage parity with the law ({plan}): stop iterates {iters.tolist()}, flags checked {stats['stop_checked']}, "
          f"within 1e-9 of a threshold {stats['near']}; coverage (clipped, unclipped, D fed back) {cover}")
    assert stats["near"] == 0 and stats["stop_checked"] > 0
    assert iters.max() == 3 and iters.min() == 1
    for i in (1, 2, 3):                             # the counts the host test chose the gains by
        clipped, unclipped, fed = cover[(12, i)]
        assert clipped > 0 and unclipped > 0 and (fed > 0) == (i > 1), (i, cover[(12, i)])
    pl.close()


# ---------------------------------------------------------------------------------------------
# 4. B16 and the shift
# ---------------------------------------------------------------------------------------------
def _b16_kwargs(n, only=None):
    """Scenario k is kind (k + 2) % 3 of: stops at iterate 1 by its thresholds, at 2 and at 3 by
    its max_admm_iter; prob = k % 2.  only: scenario `only` of that fleet alone."""
    ks = list(range(n)) if only is None else [only]
    kind = [(k + 2) % 3 for k in ks]
    thres = [np.inf if c == 0 else 0.01 for c in kind]
    return dict(n_scenarios=len(ks), prob=[k % 2 for k in ks], primal_thres=thres, dual_thres=thres, t_step0=12,
                max_admm_iter=[(2, 1, 2)[c] for c in kind], round_decimals=-1), [(1, 2, 3)[c] for c in kind]


def _b16_run(b, kw):
    pl = obca.OBCADevicePlanner(b, dual=C.GAINS, **kw)
    hist = [(pl.get("STATE"), pl.get("DUAL_S"), pl.get("DUAL_D"))]
    while pl.counts()[1]:
        pl.iterate()
        hist.append((pl.get("STATE"), pl.get("DUAL_S"), pl.get("DUAL_D")))
    iters, X = pl.get("ITERS"), pl.get("X")
    pl.shift()
    out = dict(ITERS=iters, X=X, hist=hist, STATE=pl.get("STATE"), STATE_PREV=pl.get("STATE_PREV"),
               DUAL_S=pl.get("DUAL_S"), DUAL_D=pl.get("DUAL_D"))
    pl.close()
    return out


@pytest.fixture(scope="module")
def b16_alone(batches):
    """Each of the 6 scenario kinds (k % 6) run alone (computed once, never changed)."""
    b, _ = batches
    return [_b16_run(b, _b16_kwargs(6, only=k)[0]) for k in range(6)]


@pytest.mark.parametrize("n", [1, 5, 70])
def test_b16_and_the_shift(batches, b16_alone, n):
    b, _ = batches
    kw, stops = _b16_kwargs(n)
    got = _b16_run(b, kw)
    assert got["ITERS"].tolist() == stops
    _bits(got["STATE"], got["STATE_PREV"], "the shift fills both states")
    for s in range(n):
        state, S, D = (a[s] for a in got["hist"][stops[s] - 1])        # before the stopping iterate
        Sw, Dw = obca.shift_dual(S, D)
        _bits(got["DUAL_S"][s], Sw, f"DUAL_S of scenario {s}")
        _bits(got["DUAL_D"][s], Dw, f"DUAL_D of scenario {s}")
        want = obca.pack_state(obca.iterate_next_state(obca.unpack_state(state)[0]), got["X"][s, :, 1])
        _bits(got["STATE"][s], want, f"STATE of scenario {s}: the same iterate as the integrator")
        if stops[s] > 2:
            assert D.any()                          # a non-zero D went through the shift
        one = b16_alone[s % 6]
        for key in ("STATE", "DUAL_S", "DUAL_D", "X"):
            _bits(got[key][s], one[key][0], f"{key} of scenario {s} against its run alone")


# ---------------------------------------------------------------------------------------------
# 5. the trace, 6. the host planner
# ---------------------------------------------------------------------------------------------
def test_trace_with_the_law(batches):
    b, _ = batches
    kw = dict(SETUP, n_scenarios=3)
    pl = obca.OBCADevicePlanner(b, dual=C.GAINS, **kw)
    rec = pl.run(3)
    state = pl.get("STATE")
    pl.close()
    pt = obca.OBCADevicePlanner(b, dual=C.GAINS, **kw)
    tr = pt.run_traced(3)
    for k in ("state_record", "iter_num_record", "lambda_record"):
        _bits(np.asarray(getattr(pt.record, k)), np.asarray(getattr(rec, k)), k)
    _bits(pt.get("STATE"), state, "STATE")
    _bits(tr.lamb, np.asarray(rec.lambda_record), "the trace's LAMBDA rows are the law's duals")
    pt.close()
    # they are the law's: clipped at windup_sat, which the plain duals of the same plan exceed
    assert np.abs(tr.lamb).max() == C.GAINS["windup_sat"]
    pp = obca.OBCADevicePlanner(b, **kw)
    assert np.abs(np.asarray(pp.run(1).lambda_record)).max() > C.GAINS["windup_sat"]
    pp.close()


def test_first_iterate_equals_the_host_planner(batches):
    b, ref = batches
    host_stages, dev_stages = [], []
    kw = dict(SETUP, n_scenarios=3)
    hp = obca.OBCAPlanner(ref, dual=C.GAINS, on_stage=lambda *a: host_stages.append(a), **kw)
    dp = obca.OBCADevicePlanner(b, dual=C.GAINS, on_stage=lambda *a: dev_stages.append(a), **kw)
    hp.run(1)
    dp.run(1)
    h0 = [s for s in host_stages if s[0] == "residual"][0]
    d0 = [s for s in dev_stages if s[0] == "residual"][0]
    assert h0[1]["i_iter"] == d0[1]["i_iter"] == 1 and h0[1]["scenarios"] == d0[1]["scenarios"] == [0, 1, 2]
    _bits(np.stack(d0[1]["lamb_bar_prev"]), np.stack(h0[1]["lamb_bar_prev"]), "lamb_bar before")
    _bits(np.stack(d0[1]["lamb_bar"]), np.stack(h0[1]["lamb_bar"]), "the law's lamb_bar")
    _bits(d0[2]["dual"], h0[2]["dual"], "the dual residual")
    assert np.abs(np.stack(d0[1]["lamb_bar"])).max() == C.GAINS["windup_sat"]
    dp.close()


# ---------------------------------------------------------------------------------------------
# 7. errors before any launch
# ---------------------------------------------------------------------------------------------
def test_errors_before_any_launch(batches):
    b, ref = batches
    lib = b._lib
    kw = dict(SETUP, n_scenarios=3)
    pl = obca.OBCADevicePlanner(b, **kw)
    probe = np.zeros((3, 2, NT, 9))
    code = obca.PLAN_GET["DUAL_S"][0]
    assert lib.piadmm_obca_plan_get(b._h, code, probe.ctypes.data, probe.nbytes) == _lib.E_STATE
    assert b"no dual law" in lib.piadmm_obca_last_error(b._h)
    start = pl.get("STATE")
    good = obca.dual_rows(3, C.GAINS)
    bad_rows = []
    for j, v in ((0, np.nan), (1, np.inf), (4, 2.0), (2, 0.0), (2, -1.0), (6, 1.0)):
        rows = np.repeat(good, 3, axis=0)
        rows[1, j] = v
        bad_rows.append(rows)
    for rows in bad_rows:
        assert lib.piadmm_obca_dual_plan(b._h, _lib.dptr(rows), 3) == _lib.E_ARG
        assert b"obca_dual_plan: row 1: " in lib.piadmm_obca_last_error(b._h)
        z = np.zeros((3, 2, NT, 9))
        st = np.zeros((3, NT), np.int32)
        assert lib.piadmm_obca_dual_pi(b._h, 3, _lib.dptr(z), _lib.dptr(z), _lib.dptr(z), _lib.iptr(st), _lib.dptr(rows), 3,
                                       _lib.dptr(z.copy()), _lib.dptr(z.copy()), _lib.dptr(z.copy()),
                                       _lib.dptr(np.zeros((3, NT)))) == _lib.E_ARG
        assert b"obca_dual_pi: row 1: " in lib.piadmm_obca_last_error(b._h)
    two = np.repeat(good, 2, axis=0)
    assert lib.piadmm_obca_dual_plan(b._h, _lib.dptr(two), 2) == _lib.E_ARG
    assert b"rows must be 1 or n" in lib.piadmm_obca_last_error(b._h)
    with pytest.raises(_lib.PiadmmError, match="row 0: windup_sat > 0") as ei:
        pl.set_dual(kP=0.5, kI=1.0, windup_sat=0.0, windup=1)
    assert ei.value.code == _lib.E_ARG and pl.dual_par is None
    # the kernel-alone call: n and a non-finite input
    z, st = np.zeros((1, 2, NT, 9)), np.zeros((1, NT), np.int32)
    nan = z.copy()
    nan[0, 1, 2, 3] = np.nan
    for n_arg, w_arg in ((0, z), (1, nan)):
        assert lib.piadmm_obca_dual_pi(b._h, n_arg, _lib.dptr(w_arg), _lib.dptr(z), _lib.dptr(z), _lib.iptr(st),
                                       _lib.dptr(good), 1, _lib.dptr(z.copy()), _lib.dptr(z.copy()), _lib.dptr(z.copy()),
                                       _lib.dptr(np.zeros((1, NT)))) == _lib.E_ARG
    # nothing above touched the plan: still no law, the state as it was
    assert lib.piadmm_obca_plan_get(b._h, code, probe.ctypes.data, probe.nbytes) == _lib.E_STATE
    _bits(pl.get("STATE"), start, "the plan is unchanged")
    # attaching after an iterate of the open step
    pl.iterate()
    with pytest.raises(_lib.PiadmmError, match="only at a step boundary") as ei:
        pl.set_dual(**C.GAINS)
    assert ei.value.code == _lib.E_STATE
    while pl.counts()[1]:
        pl.iterate()
    pl.shift()
    pl.t_step += 1
    # at the boundary it attaches; a bad row then leaves the attached law as it was
    pl.set_dual(**C.GAINS)
    assert lib.piadmm_obca_dual_plan(b._h, _lib.dptr(bad_rows[0]), 3) == _lib.E_ARG
    _bits(pl.get("DUAL_PAR"), good, "the attached law stays")
    pl.step()
    assert (np.abs(pl.get("LAMBDA")) == C.GAINS["windup_sat"]).any()
    # detaching restores the plain path: the next step equals that of a plan that never had a law
    pl.clear_dual()
    assert lib.piadmm_obca_plan_get(b._h, code, probe.ctypes.data, probe.nbytes) == _lib.E_STATE
    state = pl.get("STATE")
    never = obca.OBCADevicePlanner(ref, state=state, **dict(kw, t_step0=pl.t_step))
    _bits(never.get("STATE"), state, "same start")
    pl.step()
    never.step()
    for key in ("STATE", "STATE_PREV", "X", "ITERS", "LAMBDA", "DUAL", "PRIMAL"):
        _bits(pl.get(key), never.get(key), f"{key} after detaching")
    never.close()
    # no plan: PIADMM_E_STATE; the end of the plan frees the law
    pl.set_dual(**C.GAINS)
    pl.close()
    assert lib.piadmm_obca_dual_plan(b._h, _lib.dptr(good), 1) == _lib.E_STATE
    again = obca.OBCADevicePlanner(b, **kw)
    assert lib.piadmm_obca_plan_get(b._h, code, probe.ctypes.data, probe.nbytes) == _lib.E_STATE
    again.close()
