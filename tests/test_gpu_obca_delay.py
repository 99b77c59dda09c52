"""Communication delay in the exchange of the device OBCA plan (k_plan_delay and k_delay_exchange in
csrc/piadmm_obca_plan_delay.hip, k_plan_exchange_stale in csrc/piadmm_obca_plan.hip, behind
piadmm_obca_delay_tau / _delay_exchange / _delay_plan; OBCABatch.delay_tau, OBCABatch.delay_exchange,
OBCADevicePlanner(delay=...), set_delay, clear_delay, the DELAY_ items of `get`).

Bars.  The generator's words are compared with obca.noise_raw(calls=(3,)) exactly.  The latencies
are compared with the host statement obca.delay_tau at _obca_delay_cases.DELAY_TOL (device libm is
not NumPy's; the figure is 8 times the largest deviation measured over these cases); std = 0 and rows
whose every draw clips are exact.  The stale states are compared with obca.stale_states bit for bit
(every operation is exact IEEE arithmetic); A and b of the stale states with obca.halfspaces at the
bars tests/test_gpu_obca_plan.py holds them to (1e-15 and 1e-12 absolute; the states' |x| + |y|
stays below that file's 170).  Everything in the plan is bit equality between device runs.

3 fleet scenarios with different OvertakeSpecs (5 for the re-run), max_admm_iter <= 2, t_step0 = 12,
2 MPC steps.  The yardstick runs are computed once and never changed."""
import ctypes

import numpy as np
import pytest

import _obca_delay_cases as C
import _obca_dual_cases as D
import _obca_fleet_cases as F
import _obca_noise_cases as Z
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

_bits = P._bits
CASES, T0, N = [0, 1, 2], 12, 3
S_A, S_B, S_LX, S_INIT = 126, 238, 476, 546
ITEMS = ("STATE", "STATE_PREV", "X", "CTRL", "CTRL_PREV", "PRIMAL", "DUAL", "STATUS_MASK", "LAMBDA", "ITERS")
# delay rows, one per scenario; streams and a seed with both words in use
DPAR = np.stack([C.UNIT_ROW, obca.delay_row(avg=(0.03, 0.06), std=0.05, tau_max=(0.1, 0.08), trunc=1.5),
                 obca.delay_row(avg=0.02, std=(0.0, 0.04))])
STREAMS = np.array([5, 2 ** 32 + 1, 2 ** 63 - 1], np.int64)
SEED, K0 = 2 ** 63 + 12345, 7
DELAY = dict(par=DPAR, streams=STREAMS, seed=SEED, k0=K0)
_i64p = ctypes.POINTER(ctypes.c_int64)


@pytest.fixture(scope="module")
def batches():
    """(the handle under test, a second handle for the yardsticks)."""
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    b, ref = obca.OBCABatch(0), obca.OBCABatch(0)
    yield b, ref
    b.close()
    ref.close()


def _kw(cases=CASES, **extra):
    return dict(F.fleet_kwargs(cases, T0), **extra)


def _items(pl, names=ITEMS):
    return {k: pl.get(k).copy() for k in names}


def _expect(code, what, call, *a, **k):
    with pytest.raises(_lib.PiadmmError, match=what) as e:
        call(*a, **k)
    assert f"error {code}:" in str(e.value), str(e.value)


def _two_traced_steps(pl):
    """Two traced MPC steps: the items after each, and the trace's rows."""
    pl.trace_begin(2)
    assert pl.trace_run(1) == 1
    after1 = _items(pl)
    assert pl.trace_run(1) == 1
    after2 = _items(pl)
    out = dict(after1=after1, after2=after2, states=pl.trace_get("STATES"), clearance=pl.trace_get("CLEARANCE"),
               iters=pl.trace_get("ITERS"), mask=pl.trace_get("STATUS_MASK"), primal=pl.trace_get("PRIMAL"),
               dual=pl.trace_get("DUAL"), lamb=pl.trace_get("LAMBDA"), summary=pl.trace_get("SUMMARY"))
    pl.trace_end()
    return out


TRACE_KEYS = ("states", "clearance", "iters", "mask", "primal", "dual", "lamb", "summary")


def _same_run(a, b, what):
    for step in ("after1", "after2"):
        for key in ITEMS:
            _bits(a[step][key], b[step][key], f"{what}: {key} {step}")
    for key in TRACE_KEYS:
        _bits(a[key], b[key], f"{what}: the trace's {key}")


@pytest.fixture(scope="module")
def plain(batches):
    """The fleet without any attachment."""
    _, ref = batches
    pl = obca.OBCADevicePlanner(ref, **_kw())
    out = _two_traced_steps(pl)
    pl.close()
    return out


@pytest.fixture(scope="module")
def drawn(batches):
    """Plan A: the fleet with the latencies drawn in the plan, no tape."""
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, delay=DELAY, **_kw())
    _bits(pl.get("DELAY_PAR"), DPAR, "DELAY_PAR")
    _bits(pl.get("DELAY_STREAMS"), STREAMS, "DELAY_STREAMS")
    assert pl.get("DELAY_SEED").tolist() == [SEED, K0, 0]
    tau0 = pl.get("DELAY_TAU")
    out = _two_traced_steps(pl)
    assert pl.get("DELAY_SEED").tolist() == [SEED, K0, 2] and int(pl.get("T_STEP")[0]) == T0 + 2
    out["tau0"], out["tau2"] = tau0, pl.get("DELAY_TAU")
    pl.close()
    return out


@pytest.fixture(scope="module")
def dev_tau(batches):
    """The device's latencies of the same rows, streams, seed and k0: N x 3 x 2."""
    _, ref = batches
    return ref.delay_tau(N, 3, DPAR, STREAMS, SEED, K0)


# ---------------------------------------------------------------------------------------------
# k_plan_delay alone
# ---------------------------------------------------------------------------------------------
KERNEL_CASES = C.kernel_cases()


@pytest.mark.parametrize("case", range(len(KERNEL_CASES)))
def test_kernel_alone(batches, case):
    b, _ = batches
    n, cap, streams, seed, k0 = KERNEL_CASES[case]
    keep = streams.copy()
    tau, raw = b.delay_tau(n, cap, C.UNIT_ROW, streams, seed, k0, raw=True)
    assert tau.shape == (n, cap, 2) and raw.shape == (n, cap, 2, 4) and raw.dtype == np.uint32
    for i in range(cap):
        _bits(raw[:, i], obca.noise_raw(seed, streams, k0 + i, calls=(3,))[:, :, 0], f"the words of step index {k0 + i}")
    want = obca.delay_tau(n, cap, C.UNIT_ROW, streams, seed, k0)
    assert np.isfinite(tau).all() and (tau >= 0.0).all() and (tau <= obca.DT).all()
    dev = float(np.abs(tau - want).max())
    print(f"k_plan_delay vs obca.delay_tau, n = {n}, cap = {cap}, seed = {seed}, k0 = {k0}: "
          f"max |deviation| {dev:.6e} (bound {C.DELAY_TOL:.6e}), tau in [{want.min():.4f}, {want.max():.4f}]")
    assert dev <= C.DELAY_TOL, (n, cap, dev)
    assert np.array_equal(streams, keep)
    # a second call gives the same bits, without the words too; one shared row is the n rows
    _bits(b.delay_tau(n, cap, C.UNIT_ROW, streams, seed, k0), tau, "repeat, raw_out NULL")
    _bits(b.delay_tau(n, cap, np.tile(C.UNIT_ROW, (n, 1)), streams, seed, k0), tau, "n rows")
    # std = 0: min(tau_max, avg) bit for bit
    row = obca.delay_row(avg=(1 / 30, 0.09), std=0.0, tau_max=(0.1, 0.07))
    _bits(b.delay_tau(n, cap, row, streams, seed, k0), obca.delay_tau(n, cap, row, streams, seed, k0), "std = 0")
    _bits(b.delay_tau(n, cap, row, streams, seed, k0), np.broadcast_to([1 / 30, 0.07], (n, cap, 2)).copy(), "std = 0")
    # rows whose every draw clips: |z| stays below 9 (u1 >= 2^-53), so avg = 1 is above tau_max and a
    # tape of -1 below 0 whatever is drawn
    high = obca.delay_row(avg=1.0, std=0.025, tau_max=(0.1, 0.0625))
    _bits(b.delay_tau(n, cap, high, streams, seed, k0), np.broadcast_to([0.1, 0.0625], (n, cap, 2)).copy(), "all at tau_max")
    tape = np.full((n, cap, 2), -1.0)
    _bits(b.delay_tau(n, cap, C.UNIT_ROW, streams, seed, k0, tape=tape), np.zeros((n, cap, 2)), "all at 0")
    # a tape adds its term in front of the draw
    tape = np.random.default_rng(case).uniform(-0.05, 0.05, (n, cap, 2))
    got = b.delay_tau(n, cap, C.UNIT_ROW, streams, seed, k0, tape=tape)
    assert np.abs(got - obca.delay_tau(n, cap, C.UNIT_ROW, streams, seed, k0, tape=tape)).max() <= C.DELAY_TOL


def test_kernel_alone_streams_k0_and_refusals(batches):
    b, _ = batches
    n, seed = 33, C.SEEDS[1]
    a = b.delay_tau(n, 4, C.UNIT_ROW, None, seed, 0)
    _bits(a, b.delay_tau(n, 4, C.UNIT_ROW, np.arange(n, dtype=np.int64), seed, 0), "streams NULL")
    _bits(b.delay_tau(n, 1, C.UNIT_ROW, None, seed, 3)[:, 0], a[:, 3], "k0 = 3")
    assert b.delay_tau(n, 0, C.UNIT_ROW).shape == (n, 0, 2)
    # independent of the noise under the same seed and streams: other words
    _, words = b.delay_tau(n, 1, C.UNIT_ROW, None, seed, 0, raw=True)
    _, noise = b.noise_tape(n, 1, obca.noise_row(sigma=1.0), None, seed, 0, raw=True)
    for j in range(3):
        assert not (words[:, 0] == noise[:, 0, :, j]).all(axis=-1).any()
    for row, word in C.bad_rows():
        rows = np.stack([C.UNIT_ROW, C.UNIT_ROW, row, C.UNIT_ROW])
        _expect(-1, "obca_delay_tau: row 2: .*" + word, b.delay_tau, 4, 1, rows)
    _expect(-1, "rows must be 1 or n", b.delay_tau, 4, 1, np.stack([C.UNIT_ROW, C.UNIT_ROW]))
    _expect(-1, "streams\\[1\\]", b.delay_tau, 2, 1, C.UNIT_ROW, [0, -1])
    _expect(-1, "k0 >= 0", b.delay_tau, 2, 1, C.UNIT_ROW, None, 0, -1)
    _expect(-1, "k0 >= 0", b.delay_tau, 2, 2, C.UNIT_ROW, None, 0, 2 ** 31 - 1)
    assert b.delay_tau(2, 1, C.UNIT_ROW, None, 0, 2 ** 31 - 1).shape == (2, 1, 2)
    bad = np.zeros((2, 2, 2))
    bad[1, 1, 0] = np.inf
    _expect(-1, "the tape of scenario 1 is not finite \\(step 1\\)", b.delay_tau, 2, 2, C.UNIT_ROW, None, 0, 0, bad)
    # the sizes, before any pointer is read
    lib, dp = b._lib, _lib.dptr(C.UNIT_ROW)
    for m, cap in ((0, 1), (-1, 1), (2 ** 20 + 1, 1), (1, -1), (1, 2 ** 20 + 1), (2 ** 20, 128)):
        assert lib.piadmm_obca_delay_tau(b._h, m, cap, dp, 1, None, 0, 0, None, None, None) == _lib.E_ARG, (m, cap)
    assert lib.piadmm_obca_delay_tau(b._h, 2, 1, None, 1, None, 0, 0, None, None, None) == _lib.E_ARG
    assert lib.piadmm_obca_delay_tau(b._h, 2, 1, dp, 1, None, 0, 0, None, None, None) == _lib.E_ARG     # tau_out NULL
    assert lib.piadmm_obca_delay_tau(b._h, 2, 0, dp, 1, None, 0, 0, None, None, None) == 0


# ---------------------------------------------------------------------------------------------
# the stale message alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.EXCHANGE_SIZES)
def test_exchange_alone(batches, n):
    b, _ = batches
    X, tau = C.exchange_states(n, seed=n), C.exchange_taus(n, seed=n)
    assert (tau == 0.0).any() and (tau == obca.DT).any() and np.abs(X[..., :2]).sum(axis=-1).max() < 170.0
    want = obca.stale_states(X, tau)
    worst = [0.0, 0.0]
    for prob in (0, 1, np.arange(n) % 2):
        lx, A, bb = b.delay_exchange(X, prob, tau)
        _bits(lx, want, "local_x is stale_states, bit for bit")
        pr = np.broadcast_to(prob, (n,))
        for s in range(n):
            for v in (0, 1):
                for t in range(7):
                    Ah, bh = obca.halfspaces(want[s, v, t], int(pr[s]))
                    worst[0] = max(worst[0], float(np.abs(A[s, v, t] - Ah).max()))
                    worst[1] = max(worst[1], float(np.abs(bb[s, v, t] - bh).max()))
    print(f"k_delay_exchange vs halfspaces(stale_states), n = {n}: max |dA| {worst[0]:.3e}, max |db| {worst[1]:.3e}")
    assert worst[0] <= 1e-15 and worst[1] <= 1e-12, worst
    # tau = 0 everywhere and one ulp above 0: X[1:], bit for bit (the latter where X[1:] is not 0)
    lx0, A0, b0 = b.delay_exchange(X, 1, np.zeros((n, 2)))
    _bits(lx0, X[:, :, 1:], "tau = 0")
    lx1, _, _ = b.delay_exchange(X, 1, np.full((n, 2), 5e-324))
    _bits(lx1, obca.stale_states(X, np.full((n, 2), 5e-324)), "tau one ulp above 0")
    # tau = DT everywhere
    _bits(b.delay_exchange(X, 0, np.full((n, 2), obca.DT))[0], obca.stale_states(X, np.full((n, 2), obca.DT)), "tau = DT")


def test_exchange_alone_at_tau_zero_is_the_plain_exchange(batches):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, **_kw())
    pl.iterate()
    X, st = pl.get("X"), pl.get("STATE")
    lx, A, bb = ref.delay_exchange(X, pl.prob, np.zeros((N, 2)))
    _bits(lx, st[:, S_LX:S_INIT].reshape(N, 2, 7, 5), "local_x of the plain exchange")
    _bits(A, st[:, S_A:S_B].reshape(N, 2, 7, 4, 2), "A of the plain exchange")
    _bits(bb, st[:, S_B:S_B + 56].reshape(N, 2, 7, 4), "b of the plain exchange")
    pl.close()


def test_exchange_alone_refusals(batches):
    b, _ = batches
    X, tau = C.exchange_states(2), np.array([[0.0, 0.05], [0.1, 0.02]])
    assert b.delay_exchange(X, [0, 1], tau)[0].shape == (2, 2, 7, 5)
    for bad in (np.nextafter(obca.DT, 1.0), -1e-300, np.nan, np.inf):
        t = tau.copy()
        t[1, 0] = bad
        _expect(-1, "obca_delay_exchange: tau of scenario 1 must be in \\[0, DT\\]", b.delay_exchange, X, 1, t)
    _expect(-1, "prob\\[1\\] must be 0 or 1", b.delay_exchange, X, [0, 2], tau)
    Xb = X.copy()
    Xb[1, 0, 0, 3] = np.nan
    _expect(-1, "X of scenario 1 is not finite", b.delay_exchange, Xb, 1, tau)
    lib = b._lib
    for m in (0, -1, 2 ** 20 + 1):
        assert lib.piadmm_obca_delay_exchange(b._h, m, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.piadmm_obca_delay_exchange(b._h, 2, _lib.dptr(X), None, _lib.dptr(tau), None, None, None) == _lib.E_ARG


# ---------------------------------------------------------------------------------------------
# in the plan
# ---------------------------------------------------------------------------------------------
def test_drawn_in_the_plan_is_the_plan_given_the_devices_latencies(batches, drawn, dev_tau, plain):
    _, ref = batches
    _bits(drawn["tau0"], dev_tau[:, 0], "DELAY_TAU at the attachment")
    _bits(drawn["tau2"], dev_tau[:, 2], "DELAY_TAU after two shifts")
    assert np.abs(dev_tau - obca.delay_tau(N, 3, DPAR, STREAMS, SEED, K0)).max() <= C.DELAY_TOL
    pl = obca.OBCADevicePlanner(ref, delay=dict(par=C.ZERO_ROW, tape=dev_tau[:, :2]), **_kw())
    _bits(pl.get("DELAY_TAU"), dev_tau[:, 0], "the tape's first row")
    _same_run(drawn, _two_traced_steps(pl), "delay_plan drawn against delay_plan(tape = delay_tau, zero row)")
    # with a tape its cap applies: the tape's two steps are closed
    _expect(-3, "obca_plan_step: latency tape exhausted", pl.step)
    pl.close()
    # the delay changed what was exchanged, and so the run
    assert dev_tau[:, :2].min(axis=1).max() > 0.0
    assert not np.array_equal(drawn["after1"]["STATE"], plain["after1"]["STATE"])


def test_zero_row_and_attach_then_detach_are_the_plain_plan(batches, plain):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, delay=dict(par=C.ZERO_ROW, streams=STREAMS, seed=SEED), **_kw())
    assert not pl.get("DELAY_TAU").any()
    _same_run(_two_traced_steps(pl), plain, "the zero row")
    pl.close()
    pl = obca.OBCADevicePlanner(b, **_kw())
    _expect(-3, "no delay attached", pl.get, "DELAY_PAR")
    pl.set_delay(**DELAY)
    pl.set_delay(par=DPAR[0], seed=3)                   # a second call replaces the first
    _bits(pl.get("DELAY_PAR"), DPAR[:1], "the replaced row")
    _bits(pl.get("DELAY_STREAMS"), np.arange(N, dtype=np.int64), "the replaced streams")
    assert pl.get("DELAY_SEED").tolist() == [3, 0, 0]
    pl.clear_delay()
    for item in obca.DELAY_GET:
        _expect(-3, "no delay attached", pl.get, item)
    pl.clear_delay()                                    # detaching nothing is not an error
    _same_run(_two_traced_steps(pl), plain, "attach then detach")
    pl.close()


def test_rerun_by_stream_id(batches):
    b, ref = batches
    cases = [0, 1, 2, 3, 1]
    rows = np.stack([obca.delay_row(avg=0.03 + 0.01 * s, std=0.02 + 0.005 * s) for s in range(5)])
    big = obca.OBCADevicePlanner(b, delay=dict(par=rows, seed=SEED, k0=K0), **_kw(cases))
    _bits(big.get("DELAY_STREAMS"), np.arange(5, dtype=np.int64), "streams NULL")
    tb = _two_traced_steps(big)
    big.close()
    pick = [1, 3]
    small = obca.OBCADevicePlanner(ref, delay=dict(par=rows[pick], streams=pick, seed=SEED, k0=K0),
                                   **_kw([cases[s] for s in pick]))
    ts = _two_traced_steps(small)
    small.close()
    for step in ("after1", "after2"):
        for key in ITEMS:
            _bits(ts[step][key], tb[step][key][pick], f"{key} {step} of scenarios {pick} re-run alone")
    for key in TRACE_KEYS:
        axis = 0 if key == "summary" else 1
        _bits(ts[key], np.take(tb[key], pick, axis=axis), f"the trace's {key} of scenarios {pick} re-run alone")
    # other ids draw something else
    other = obca.OBCADevicePlanner(ref, delay=dict(par=rows[pick], streams=[0, 1], seed=SEED, k0=K0),
                                   **_kw([cases[s] for s in pick]))
    other.step()
    assert not np.array_equal(other.get("STATE"), tb["after1"]["STATE"][pick])
    other.close()


def test_resume_by_k0(batches, drawn):
    _, ref = batches
    pl = obca.OBCADevicePlanner(ref, state=drawn["after1"]["STATE"], delay=dict(DELAY, k0=K0 + 1),
                                **dict(_kw(), t_step0=T0 + 1))
    iters = np.zeros(N, np.int32)
    pl._check(pl._lib.piadmm_obca_plan_step(ref._h, _lib.iptr(iters)))
    for key in ("STATE", "STATE_PREV", "X", "CTRL", "PRIMAL", "DUAL", "STATUS_MASK", "LAMBDA", "ITERS"):
        _bits(pl.get(key), drawn["after2"][key], f"{key} of step 2, resumed")
    _bits(iters, drawn["iters"][1], "ITERS of step 2, resumed")
    pl.close()


def test_with_feedback_and_noise_on_top(batches, dev_tau):
    b, ref = batches
    fpar = np.stack([obca.feedback_row(method=1, n_sub=4, lr=1.1, lf=1.4, gain_a=0.9),
                     obca.feedback_row(n_sub=(2, 64), gain_w=(1.2, 0.7)), obca.feedback_row()])
    zpar = obca.noise_row(sigma=Z.SIGMA)
    # noise and delay share the seed and the streams: their calls differ
    noise = dict(par=zpar, streams=STREAMS, seed=SEED, k0=K0)
    pa = obca.OBCADevicePlanner(b, feedback=dict(par=fpar), noise=noise, delay=DELAY, **_kw())
    pb = obca.OBCADevicePlanner(ref, feedback=dict(par=fpar), noise=noise,
                                delay=dict(par=C.ZERO_ROW, tape=dev_tau[:, :2]), **_kw())
    ra, rb = _two_traced_steps(pa), _two_traced_steps(pb)
    _same_run(ra, rb, "feedback + noise + delay")
    assert pa.feedback_steps() == 2 and pa.get("DELAY_SEED").tolist() == [SEED, K0, 2]
    # a new feedback attachment drops the noise and leaves the delay and its step count
    pa.set_feedback(par=fpar)
    assert pa.feedback_steps() == 0 and pa.get("DELAY_SEED").tolist() == [SEED, K0, 2]
    _bits(pa.get("DELAY_TAU"), dev_tau[:, 2], "DELAY_TAU of the third step")
    pa.close()
    pb.close()
    # against the same closed loop without the delay: the exchange differs, the plant is the same
    pc = obca.OBCADevicePlanner(ref, feedback=dict(par=fpar), noise=noise, **_kw())
    pc.step()
    assert not np.array_equal(pc.get("STATE"), ra["after1"]["STATE"])
    pc.close()


def test_order_and_dual_law_on_top_change_nothing(batches):
    b, ref = batches
    gains = D.fleet_gains(CASES)
    law = ("DUAL_S", "DUAL_D", "DUAL_S_PREV", "DUAL_D_PREV")
    pa = obca.OBCADevicePlanner(b, delay=DELAY, dual=gains, order=True, **_kw())
    pb = obca.OBCADevicePlanner(ref, delay=DELAY, dual=gains, **_kw())
    for step in (1, 2):
        pa.step()
        pb.step()
        for key in ITEMS + law + ("DELAY_TAU",):
            _bits(pa.get(key), pb.get(key), f"{key} after step {step} with the order")
    pa.close()
    pb.close()


def test_on_stage_sees_the_stale_exchange(batches, dev_tau):
    b, _ = batches
    seen = []

    def on_stage(name, inputs, outputs):
        if name == "local":
            seen.append(dict(X=outputs["result"].X.copy(), scenarios=list(inputs["scenarios"]), tau=pl.get("DELAY_TAU"),
                             step=pl.t_step))
        elif name == "exchange":
            seen[-1]["bar"] = outputs["bar"]

    pl = obca.OBCADevicePlanner(b, delay=DELAY, on_stage=on_stage, **_kw())
    pl.run(2)
    pl.close()
    assert {it["step"] for it in seen} == {T0, T0 + 1} and len(seen) >= 4
    for it in seen:
        # one latency per vehicle over all iterates of the step; another at the next step
        _bits(it["tau"], dev_tau[:, it["step"] - T0], "DELAY_TAU at every iterate of the step")
        for k, s in enumerate(it["scenarios"]):
            for v in (0, 1):
                _bits(it["bar"][k]["local_x"][v], obca.stale_states(it["X"][2 * k + v], it["tau"][s, v]),
                      "S_LX after the exchange is stale_states of the iterate's local output")
                for t in range(7):
                    Ah, bh = obca.halfspaces(it["bar"][k]["local_x"][v, t], pl.prob[s])
                    assert np.abs(it["bar"][k]["A"][v, t] - Ah).max() <= 1e-15
                    assert np.abs(it["bar"][k]["b"][v, t] - bh).max() <= 1e-12
    assert not np.array_equal(dev_tau[:, 0], dev_tau[:, 1])


def test_effect(batches, plain):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, delay=dict(par=obca.delay_row(avg=obca.AVG_DELAY, std=0.0)), **_kw())
    _bits(pl.get("DELAY_TAU"), np.full((N, 2), obca.AVG_DELAY), "tau = AVG_DELAY")
    pl.step()
    st, want = pl.get("STATE"), plain["after1"]["STATE"]
    for s in range(N):
        assert not np.array_equal(st[s, S_A:S_B], want[s, S_A:S_B]), f"A of scenario {s}"
        assert not np.array_equal(st[s, S_B:S_B + 56], want[s, S_B:S_B + 56]), f"b of scenario {s}"
    pl.close()


# ---------------------------------------------------------------------------------------------
# refusals and items
# ---------------------------------------------------------------------------------------------
def test_refusals_and_items(batches, plain):
    b, ref = batches
    lib = b._lib

    def attach(h, par, rows, streams=None, seed=0, k0=0, tape=None, cap=0, mode=1):
        s = None if streams is None else np.ascontiguousarray(streams, np.int64)
        return lib.piadmm_obca_delay_plan(h, mode, _lib.dptr(par), rows, None if s is None else s.ctypes.data_as(_i64p),
                                          ctypes.c_uint64(seed), k0, _lib.dptr(tape), cap)
    # no open plan (every planner before closed its own)
    assert attach(b._h, DPAR, N) == _lib.E_STATE
    assert b"no open plan" in lib.piadmm_obca_last_error(b._h)
    # host checks: the earlier attachment and the plan stay
    pl = obca.OBCADevicePlanner(b, delay=DELAY, **_kw())
    tau0 = pl.get("DELAY_TAU")

    def unchanged(what):
        _bits(pl.get("DELAY_PAR"), DPAR, f"DELAY_PAR after {what}")
        _bits(pl.get("DELAY_STREAMS"), STREAMS, f"DELAY_STREAMS after {what}")
        _bits(pl.get("DELAY_TAU"), tau0, f"DELAY_TAU after {what}")
        assert pl.get("DELAY_SEED").tolist() == [SEED, K0, 0]

    for row, word in C.bad_rows():
        rows = DPAR.copy()
        rows[1] = row
        _expect(-1, "obca_delay_plan: row 1: .*" + word, pl.set_delay, par=rows)
    assert attach(b._h, np.ascontiguousarray(DPAR[:2]), 2) == _lib.E_ARG
    assert attach(b._h, DPAR, N, mode=2) == _lib.E_ARG
    assert lib.piadmm_obca_delay_plan(b._h, 1, None, 1, None, 0, 0, None, 0) == _lib.E_ARG
    _expect(-1, "streams\\[2\\]", pl.set_delay, par=DPAR, streams=[0, 1, -1])
    _expect(-1, "k0 >= 0", pl.set_delay, par=DPAR, k0=-1)
    bad = np.zeros((N, 2, 2))
    bad[2, 0, 1] = np.nan
    _expect(-1, "the tape of scenario 2 is not finite \\(step 0\\)", pl.set_delay, par=DPAR, tape=bad)
    assert attach(b._h, DPAR, N, tape=np.zeros((N, 1, 2)), cap=-1) == _lib.E_ARG
    unchanged("the refused calls")
    # the items' sizes
    out = np.zeros(4, np.uint64)
    assert lib.piadmm_obca_plan_get(b._h, obca.DELAY_GET["DELAY_SEED"][0], out.ctypes.data, 16) == _lib.E_ARG
    assert lib.piadmm_obca_plan_get(b._h, obca.DELAY_GET["DELAY_TAU"][0], out.ctypes.data, 8) == _lib.E_ARG
    # the clock and the tenant records do not go with the delay
    _expect(-3, "obca_clock_plan: the delay is attached", pl.set_clock)
    _expect(-3, "obca_tenant_export: the delay is attached", pl.export_tenants, [0])
    pl.clear_delay()
    blob = pl.export_tenants([0])
    pl.set_delay(**DELAY)
    _expect(-3, "obca_tenant_import: the delay is attached", pl.import_tenants, [0], blob)
    unchanged("the clock and tenant calls")
    # mid-step
    pl.iterate()
    _expect(-3, "obca_delay_plan: only at a step boundary", pl.set_delay, **DELAY)
    _expect(-3, "obca_delay_plan: only at a step boundary", pl.clear_delay)
    unchanged("the mid-step calls")
    pl.close()
    # a clock attached
    pl = obca.OBCADevicePlanner(b, clock=True, **_kw())
    _expect(-3, "obca_delay_plan: a clock is attached", pl.set_delay, **DELAY)
    _expect(-3, "no delay attached", pl.get, "DELAY_TAU")
    pl.close()
    # a tape of one row: the first step runs, every call that would run the second is refused with nothing run
    pl = obca.OBCADevicePlanner(b, delay=dict(par=C.ZERO_ROW, tape=np.zeros((N, 1, 2))), **_kw())
    pl.step()
    for key in ITEMS:
        _bits(pl.get(key), plain["after1"][key], f"{key} after the tape's one step")
    before = _items(pl)
    _expect(-3, "obca_plan_step: latency tape exhausted", pl.step)
    _expect(-3, "obca_plan_iterate: latency tape exhausted", pl.iterate)
    _expect(-3, "obca_plan_shift: latency tape exhausted", pl.shift)
    pl.trace_begin(2)
    _expect(-3, "obca_trace_run: latency tape exhausted before 1 steps$", pl.trace_run, 1)
    assert pl.trace_rows() == 0
    pl.trace_end()
    assert pl.counts() == (0, N, 0) and pl.get("DELAY_SEED").tolist() == [0, 0, 1]
    for key in ITEMS:
        _bits(pl.get(key), before[key], f"{key} after the refused steps")
    # a tape without rows refuses the first
    pl.set_delay(par=C.ZERO_ROW, tape=np.zeros((N, 0, 2)))
    _expect(-3, "obca_plan_step: latency tape exhausted", pl.step)
    # the step index ends at 2^31 - 1: refused before anything runs
    pl.set_delay(par=DPAR, k0=2 ** 31 - 1)
    pl.trace_begin(2)
    _expect(-3, "obca_trace_run: delay step index exhausted before 2 steps$", pl.trace_run, 2)
    assert pl.trace_rows() == 0 and pl.counts() == (0, N, 0) and pl.get("DELAY_SEED").tolist() == [0, 2 ** 31 - 1, 0]
    pl.trace_end()
    # and the plan is still the plain plan once the delay is gone
    pl.clear_delay()
    pl.step()
    for key in ITEMS:
        _bits(pl.get(key), plain["after2"][key], f"{key} after the refusals")
    pl.close()


def test_refusal_texts_in_full(batches):
    """The refusals the tests above match by a part, to their last word, and the step index limit as
    piadmm_obca_plan_step, _iterate and _shift name it.  2 scenarios, one MPC step."""
    b, _ = batches
    _expect(-1, "obca_delay_tau: rows must be 1 or n \\(4\\)$", b.delay_tau, 4, 1, np.stack([C.UNIT_ROW, C.UNIT_ROW]))
    _expect(-1, "obca_delay_tau: streams\\[1\\] must be >= 0$", b.delay_tau, 2, 1, C.UNIT_ROW, [0, -1])
    _expect(-1, "obca_delay_tau: k0 >= 0 and every step index below 2\\^31$", b.delay_tau, 2, 1, C.UNIT_ROW, None, 0, -1)
    _expect(-1, "obca_delay_tau: k0 >= 0 and every step index below 2\\^31$", b.delay_tau, 2, 2, C.UNIT_ROW, None, 0, 2 ** 31 - 1)
    bad = np.zeros((2, 2, 2))
    bad[1, 1, 0] = np.inf
    _expect(-1, "obca_delay_tau: the tape of scenario 1 is not finite \\(step 1\\)$", b.delay_tau, 2, 2, C.UNIT_ROW, None, 0, 0, bad)
    pl = obca.OBCADevicePlanner(b, **_kw(CASES[:2]))
    _expect(-1, "obca_delay_plan: rows must be 1 or n \\(2\\)$", pl.set_delay, par=DPAR)
    _expect(-1, "obca_delay_plan: streams\\[1\\] must be >= 0$", pl.set_delay, par=DPAR[:2], streams=[0, -1])
    _expect(-1, "obca_delay_plan: k0 >= 0 and every step index below 2\\^31$", pl.set_delay, par=DPAR[:2], k0=-1)
    _expect(-1, "obca_delay_plan: the tape of scenario 1 is not finite \\(step 1\\)$", pl.set_delay, par=DPAR[:2], tape=bad)
    pl.set_delay(par=DPAR[:2], k0=2 ** 31 - 1)
    pl.step()
    _expect(-3, "obca_plan_step: delay step index exhausted$", pl.step)
    _expect(-3, "obca_plan_iterate: delay step index exhausted$", pl.iterate)
    _expect(-3, "obca_plan_shift: delay step index exhausted$", pl.shift)
    assert pl.get("DELAY_SEED").tolist() == [0, 2 ** 31 - 1, 1]
    pl.close()
