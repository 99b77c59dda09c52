"""Device-side disturbance noise of the closed-loop OBCA plan (k_plan_noise in
csrc/piadmm_obca_plan_feedback.hip behind piadmm_obca_noise_tape / piadmm_obca_noise_plan; OBCABatch.noise_tape,
OBCADevicePlanner(noise=...), set_noise, clear_noise, the NOISE_ items of `get`).

Bars.  The generator's words are compared with obca.philox4x32 exactly.  The normals are compared
with the host statement obca.noise_tape at _obca_noise_cases.NOISE_TOL (device libm is not NumPy's;
the figure is 8 times the largest deviation measured over these cases); sigma = 0 and a truncation
that clips everything are exact.  Everything in the plan is bit equality between device runs: the
plan that draws its noise against the plan that is given the device's tape, a scenario re-run alone
by its stream id, a run resumed by k0.

3 fleet scenarios with different OvertakeSpecs (5 for the re-run), max_admm_iter <= 2, t_step0 = 12,
2 MPC steps.  The yardstick runs are computed once and never changed."""
import ctypes

import numpy as np
import pytest

import _obca_dual_cases as D
import _obca_fleet_cases as F
import _obca_noise_cases as C
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

_bits = P._bits
CASES, T0, N = [0, 1, 2], 12, 3
S_INIT = 546
ITEMS = ("STATE", "STATE_PREV", "X", "CTRL", "CTRL_PREV", "PRIMAL", "DUAL", "STATUS_MASK", "LAMBDA")
# plant rows off nominal and noise rows, one per scenario; streams and a seed with both words in use
PAR = np.stack([obca.feedback_row(method=1, n_sub=4, lr=1.1, lf=1.4, gain_a=0.9),
                obca.feedback_row(n_sub=(2, 64), gain_w=(1.2, 0.7), a_max=(0.5, 5.0)),
                obca.feedback_row()])
ZPAR = np.stack([obca.noise_row(sigma=C.SIGMA), obca.noise_row(sigma=np.array(C.SIGMA) * 2.0, bias=0.002, trunc=1.5),
                 obca.noise_row(sigma=[C.SIGMA, np.array(C.SIGMA) * 0.5])])
STREAMS = np.array([5, 2 ** 32 + 1, 2 ** 63 - 1], np.int64)
SEED, K0 = 2 ** 63 + 12345, 7
NOISE = dict(par=ZPAR, streams=STREAMS, seed=SEED, k0=K0)
TAPE = np.random.default_rng(7).normal(0.0, C.SIGMA, (N, 2, 2, 5))
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


def _init(state):
    return np.ascontiguousarray(state[:, S_INIT:].reshape(-1, 2, 5))


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
               iters=pl.trace_get("ITERS"))
    pl.trace_end()
    return out


def _same_run(a, b, what):
    for step in ("after1", "after2"):
        for key in ITEMS:
            _bits(a[step][key], b[step][key], f"{what}: {key} {step}")
    for key in ("states", "clearance", "iters"):
        _bits(a[key], b[key], f"{what}: the trace's {key}")


@pytest.fixture(scope="module")
def drawn(batches):
    """Plan A: the fleet with PAR and the noise drawn in the plan, no tape."""
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR), noise=NOISE, **_kw())
    _bits(pl.get("NOISE_PAR"), ZPAR, "NOISE_PAR")
    _bits(pl.get("NOISE_STREAMS"), STREAMS, "NOISE_STREAMS")
    assert pl.get("NOISE_SEED").tolist() == [SEED, K0]
    out = _two_traced_steps(pl)
    assert pl.feedback_steps() == 2 and int(pl.get("T_STEP")[0]) == T0 + 2
    pl.close()
    return out


@pytest.fixture(scope="module")
def dev_tape(batches):
    """The device's tape of the same rows, streams, seed and k0: N x 2 x 2 x 5."""
    _, ref = batches
    return ref.noise_tape(N, 2, ZPAR, STREAMS, SEED, K0)


@pytest.fixture(scope="module")
def fb_only(batches):
    """The fleet with PAR, no tape and no noise."""
    _, ref = batches
    pl = obca.OBCADevicePlanner(ref, feedback=dict(par=PAR), **_kw())
    out = _two_traced_steps(pl)
    pl.close()
    return out


# ---------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------
KERNEL_CASES = C.kernel_cases()


@pytest.mark.parametrize("case", range(len(KERNEL_CASES)))
def test_kernel_alone(batches, case):
    b, _ = batches
    n, cap, streams, seed, k0 = KERNEL_CASES[case]
    unit = obca.noise_row(sigma=1.0)
    keep = streams.copy()
    tape, raw = b.noise_tape(n, cap, unit, streams, seed, k0, raw=True)
    assert tape.shape == (n, cap, 2, 5) and raw.shape == (n, cap, 2, 3, 4) and raw.dtype == np.uint32
    for i in range(cap):
        _bits(raw[:, i], obca.noise_raw(seed, streams, k0 + i), f"the words of step index {k0 + i}")
    if case == 0:
        assert (n, seed, k0, int(streams[0])) == (1, 0, 0, 0)
        assert raw[0, 0, 0, 0].tolist() == list(C.KNOWN[0][2])
    want = obca.noise_tape(n, cap, unit, streams, seed, k0)
    assert np.isfinite(tape).all()
    dev = float(np.abs(tape - want).max())
    print(f"k_plan_noise vs obca.noise_tape, n = {n}, cap = {cap}, seed = {seed}, k0 = {k0}: "
          f"max |deviation| {dev:.6e} (bound {C.NOISE_TOL:.6e}), max |z| {np.abs(want).max():.3f}")
    assert dev <= C.NOISE_TOL, (n, cap, dev)
    assert np.array_equal(streams, keep)
    # a second call gives the same bits, without the words too; one shared row is the n rows
    _bits(b.noise_tape(n, cap, unit, streams, seed, k0), tape, "repeat, raw_out NULL")
    _bits(b.noise_tape(n, cap, np.tile(unit, (n, 1)), streams, seed, k0), tape, "n rows")
    # sigma = 0: the bias bit for bit
    bias = np.array([[0.1, -0.2, 1e-300, 0.0, 3.0], [1 / 3, -1e300, 5e-324, 0.0, -7.0]])
    _bits(b.noise_tape(n, cap, obca.noise_row(bias=bias), streams, seed, k0), np.broadcast_to(bias, (n, cap, 2, 5)),
          "sigma = 0")


def test_kernel_alone_everything_clipped_is_exact(batches):
    b, _ = batches
    n, cap, seed, k0, trunc = 33, 3, C.SEEDS[1], 11, 0.001
    ids = C.all_clipped_streams(seed, k0, cap, n, trunc)
    row = obca.noise_row(sigma=[C.SIGMA, np.array(C.SIGMA) * 3.0], bias=0.25, trunc=trunc)
    want = obca.noise_tape(n, cap, row, ids, seed, k0)
    # the NumPy statement shows every z of these streams clipped
    assert set(np.unique(np.abs(obca.noise_tape(n, cap, obca.noise_row(sigma=1.0, trunc=trunc), ids, seed, k0)))) == {trunc}
    _bits(b.noise_tape(n, cap, row, ids, seed, k0), want, "every z clipped")
    # streams = NULL is 0 .. n-1, k0 shifts
    unit = obca.noise_row(sigma=1.0)
    a = b.noise_tape(n, 4, unit, None, seed, 0)
    _bits(a, b.noise_tape(n, 4, unit, np.arange(n, dtype=np.int64), seed, 0), "streams NULL")
    _bits(b.noise_tape(n, 1, unit, None, seed, 3)[:, 0], a[:, 3], "k0 = 3")
    assert b.noise_tape(n, 0, unit).shape == (n, 0, 2, 5)


def test_kernel_alone_refusals(batches):
    b, _ = batches
    unit = obca.noise_row(sigma=1.0)
    for row, word in C.bad_rows():
        rows = np.stack([unit, unit, row, unit])
        _expect(-1, "obca_noise_tape: row 2: .*" + word, b.noise_tape, 4, 1, rows)
    _expect(-1, "rows must be 1 or n", b.noise_tape, 4, 1, np.stack([unit, unit]))
    _expect(-1, "streams\\[1\\]", b.noise_tape, 2, 1, unit, [0, -1])
    _expect(-1, "k0 >= 0", b.noise_tape, 2, 1, unit, None, 0, -1)
    _expect(-1, "k0 >= 0", b.noise_tape, 2, 2, unit, None, 0, 2 ** 31 - 1)
    assert b.noise_tape(2, 1, unit, None, 0, 2 ** 31 - 1).shape == (2, 1, 2, 5)
    # the sizes, before any pointer is read
    lib, dp = b._lib, _lib.dptr(unit)
    for n, cap in ((0, 1), (-1, 1), (2 ** 20 + 1, 1), (1, -1), (1, 2 ** 20 + 1), (2 ** 20, 26)):
        assert lib.piadmm_obca_noise_tape(b._h, n, cap, dp, 1, None, 0, 0, None, None) == _lib.E_ARG, (n, cap)
    assert lib.piadmm_obca_noise_tape(b._h, 2, 1, None, 1, None, 0, 0, None, None) == _lib.E_ARG
    assert lib.piadmm_obca_noise_tape(b._h, 2, 1, dp, 1, None, 0, 0, None, None) == _lib.E_ARG     # tape_out NULL
    assert lib.piadmm_obca_noise_tape(b._h, 2, 0, dp, 1, None, 0, 0, None, None) == 0


# ---------------------------------------------------------------------------------------------
# in the plan
# ---------------------------------------------------------------------------------------------
def test_drawn_in_the_plan_is_the_plan_given_the_devices_tape(batches, drawn, dev_tape, fb_only):
    _, ref = batches
    pl = obca.OBCADevicePlanner(ref, feedback=dict(par=PAR, tape=dev_tape), **_kw())
    _same_run(drawn, _two_traced_steps(pl), "noise_plan against feedback_plan(tape = noise_tape)")
    pl.close()
    # the noise moved the vehicles, and the device's tape is the statement's within the bound
    assert not np.array_equal(drawn["states"][1], fb_only["states"][1])
    assert np.abs(dev_tape - obca.noise_tape(N, 2, ZPAR, STREAMS, SEED, K0)).max() <= C.NOISE_TOL
    # without a tape nothing is exhausted, and the trace records the reached states
    _bits(drawn["states"][2], _init(drawn["after2"]["STATE"]), "STATES row 2 is init_state")


def test_tape_plus_noise_is_the_summed_tape(batches, dev_tape):
    b, ref = batches
    pa = obca.OBCADevicePlanner(b, feedback=dict(par=PAR, tape=TAPE), noise=NOISE, **_kw())
    pb = obca.OBCADevicePlanner(ref, feedback=dict(par=PAR, tape=TAPE + dev_tape), **_kw())
    _same_run(_two_traced_steps(pa), _two_traced_steps(pb), "tape + noise")
    # with a tape its cap still applies
    _expect(-3, "obca_plan_step: disturbance tape exhausted", pa.step)
    pa.close()
    pb.close()


def test_rerun_by_stream_id(batches):
    b, ref = batches
    cases = [0, 1, 2, 3, 1]
    rows = np.stack([obca.noise_row(sigma=np.array(C.SIGMA) * (1.0 + 0.25 * s), bias=0.001 * s) for s in range(5)])
    big = obca.OBCADevicePlanner(b, feedback=dict(), noise=dict(par=rows, seed=SEED, k0=K0), **_kw(cases))
    _bits(big.get("NOISE_STREAMS"), np.arange(5, dtype=np.int64), "streams NULL")
    tb = _two_traced_steps(big)
    big.close()
    pick = [1, 3]
    small = obca.OBCADevicePlanner(ref, feedback=dict(),
                                   noise=dict(par=rows[pick], streams=pick, seed=SEED, k0=K0),
                                   **_kw([cases[s] for s in pick]))
    ts = _two_traced_steps(small)
    small.close()
    for key in ("states", "clearance", "iters"):
        _bits(ts[key], tb[key][:, pick], f"the trace's {key} of scenarios {pick} re-run alone")
    # other ids draw something else
    other = obca.OBCADevicePlanner(ref, feedback=dict(),
                                   noise=dict(par=rows[pick], streams=[0, 1], seed=SEED, k0=K0),
                                   **_kw([cases[s] for s in pick]))
    other.step()
    assert not np.array_equal(_init(other.get("STATE")), tb["states"][1][pick])
    other.close()


def test_resume_by_k0(batches, drawn):
    _, ref = batches
    pl = obca.OBCADevicePlanner(ref, state=drawn["after1"]["STATE"], feedback=dict(par=PAR),
                                noise=dict(NOISE, k0=K0 + 1), **dict(_kw(), t_step0=T0 + 1))
    iters = np.zeros(N, np.int32)
    pl._check(pl._lib.piadmm_obca_plan_step(ref._h, _lib.iptr(iters)))
    for key in ("STATE", "STATE_PREV", "X", "CTRL", "PRIMAL", "DUAL", "STATUS_MASK", "LAMBDA"):
        _bits(pl.get(key), drawn["after2"][key], f"{key} of step 2, resumed")
    _bits(iters, drawn["iters"][1], "ITERS of step 2, resumed")
    pl.close()


def test_attach_then_detach_is_the_feedback_only_plan(batches, fb_only):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR), **_kw())
    _expect(-3, "no noise attached", pl.get, "NOISE_PAR")
    pl.set_noise(**NOISE)
    pl.set_noise(par=ZPAR[0], seed=3)                   # a second call replaces the first
    _bits(pl.get("NOISE_PAR"), ZPAR[:1], "the replaced row")
    _bits(pl.get("NOISE_STREAMS"), np.arange(N, dtype=np.int64), "the replaced streams")
    assert pl.get("NOISE_SEED").tolist() == [3, 0]
    pl.clear_noise()
    for item in obca.NOISE_GET:
        _expect(-3, "no noise attached", pl.get, item)
    pl.clear_noise()                                    # detaching nothing is not an error
    _same_run(_two_traced_steps(pl), fb_only, "attach then detach")
    pl.close()


def test_zero_noise_is_the_feedback_only_plan(batches, fb_only):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR), noise=dict(par=obca.noise_row(), seed=SEED), **_kw())
    got = _two_traced_steps(pl)
    pl.close()
    # x + 0.0 is x but for a negative zero: there is none in what is compared
    # (the recorded states are every init_state the zero row was added to)
    for run in (got, fb_only):
        assert not (np.signbit(run["states"]) & (run["states"] == 0.0)).any()
    for step in ("after1", "after2"):
        for key in ITEMS:
            assert np.array_equal(got[step][key], fb_only[step][key]), (step, key)
    for key in ("states", "clearance", "iters"):
        assert np.array_equal(got[key], fb_only[key]), key


def test_order_and_dual_law_on_top_change_nothing(batches):
    b, ref = batches
    gains = D.fleet_gains(CASES)
    law = ("DUAL_S", "DUAL_D", "DUAL_S_PREV", "DUAL_D_PREV")
    pa = obca.OBCADevicePlanner(b, feedback=dict(par=PAR), noise=NOISE, dual=gains, order=True, **_kw())
    pb = obca.OBCADevicePlanner(ref, feedback=dict(par=PAR), noise=NOISE, dual=gains, **_kw())
    for step in (1, 2):
        pa.step()
        pb.step()
        for key in ITEMS + law:
            _bits(pa.get(key), pb.get(key), f"{key} after step {step} with the order")
    pa.close()
    pb.close()
    # the law's integrators after a step are the plan's without feedback: the plant moves init_state only
    pa = obca.OBCADevicePlanner(b, feedback=dict(par=PAR), noise=NOISE, dual=gains, **_kw())
    pp = obca.OBCADevicePlanner(ref, dual=gains, **_kw())
    pa.step()
    pp.step()
    for key in law + ("LAMBDA", "X"):
        _bits(pa.get(key), pp.get(key), key)
    _bits(pa.get("STATE")[:, :S_INIT], pp.get("STATE")[:, :S_INIT], "STATE but init_state")
    assert not np.array_equal(_init(pa.get("STATE")), _init(pp.get("STATE")))
    pa.close()
    pp.close()


def test_refusals_and_items(batches, fb_only):
    b, ref = batches
    lib = b._lib

    def attach(h, par, rows, streams=None, seed=0, k0=0, mode=1):
        s = None if streams is None else np.ascontiguousarray(streams, np.int64)
        return lib.piadmm_obca_noise_plan(h, mode, _lib.dptr(par), rows, None if s is None else s.ctypes.data_as(_i64p),
                                          ctypes.c_uint64(seed), k0)
    # no open plan (every planner before closed its own)
    assert attach(b._h, ZPAR, N) == _lib.E_STATE
    assert b"no open plan" in lib.piadmm_obca_last_error(b._h)
    # no feedback attached
    pl = obca.OBCADevicePlanner(b, **_kw())
    _expect(-3, "obca_noise_plan: no feedback attached", pl.set_noise, **NOISE)
    _expect(-3, "no noise attached", pl.get, "NOISE_SEED")
    pl.close()
    _expect(-3, "obca_noise_plan: no feedback attached", obca.OBCADevicePlanner, b, noise=NOISE, **_kw())
    # host checks: the earlier attachment and the plan stay
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR), noise=NOISE, **_kw())
    for row, word in C.bad_rows():
        rows = ZPAR.copy()
        rows[1] = row
        _expect(-1, "obca_noise_plan: row 1: .*" + word, pl.set_noise, par=rows)
    assert attach(b._h, np.ascontiguousarray(ZPAR[:2]), 2) == _lib.E_ARG
    assert attach(b._h, ZPAR, N, mode=2) == _lib.E_ARG
    assert lib.piadmm_obca_noise_plan(b._h, 1, None, 1, None, 0, 0) == _lib.E_ARG
    _expect(-1, "streams\\[2\\]", pl.set_noise, par=ZPAR, streams=[0, 1, -1])
    _expect(-1, "k0 >= 0", pl.set_noise, par=ZPAR, k0=-1)
    _bits(pl.get("NOISE_PAR"), ZPAR, "NOISE_PAR after the refused calls")
    _bits(pl.get("NOISE_STREAMS"), STREAMS, "NOISE_STREAMS after the refused calls")
    assert pl.get("NOISE_SEED").tolist() == [SEED, K0] and pl.feedback_steps() == 0
    # the items' sizes
    out = np.zeros(4, np.uint64)
    assert lib.piadmm_obca_plan_get(b._h, obca.NOISE_GET["NOISE_SEED"][0], out.ctypes.data, 8) == _lib.E_ARG
    # mid-step
    pl.iterate()
    _expect(-3, "obca_noise_plan: only at a step boundary", pl.set_noise, **NOISE)
    _expect(-3, "obca_noise_plan: only at a step boundary", pl.clear_noise)
    _bits(pl.get("NOISE_PAR"), ZPAR, "NOISE_PAR after the refused calls")
    pl.close()
    # attaching the feedback again, or detaching it, detaches the noise
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR), noise=NOISE, **_kw())
    pl.set_feedback(par=PAR)
    _expect(-3, "no noise attached", pl.get, "NOISE_PAR")
    assert pl._noise is None
    pl.set_noise(**NOISE)
    pl.clear_feedback()
    _expect(-3, "no noise attached", pl.get, "NOISE_PAR")
    _expect(-3, "obca_noise_plan: no feedback attached", pl.set_noise, **NOISE)
    # a refused feedback call leaves the noise as it was
    pl.set_feedback(par=PAR)
    pl.set_noise(**NOISE)
    rows = PAR.copy()
    rows[1, 9] = 0.0
    _expect(-1, "obca_feedback_plan: row 1: ", pl.set_feedback, par=rows)
    _bits(pl.get("NOISE_PAR"), ZPAR, "NOISE_PAR after the refused feedback call")
    # the step index ends at 2^31 - 1: refused before anything runs
    pl.set_noise(par=ZPAR, k0=2 ** 31 - 1)
    pl.trace_begin(2)
    _expect(-3, "obca_trace_run: noise step index exhausted before 2 steps$", pl.trace_run, 2)
    assert pl.trace_rows() == 0 and pl.counts() == (0, N, 0) and pl.feedback_steps() == 0
    pl.trace_end()
    # and the plan is still the feedback-only plan once the noise is gone
    pl.clear_noise()
    pl.step()
    for key in ITEMS:
        _bits(pl.get(key), fb_only["after1"][key], f"{key} after the refusals")
    pl.close()


def test_refusal_texts_in_full(batches):
    """The refusals the tests above match by a part, to their last word, and the step index limit as
    piadmm_obca_plan_step and piadmm_obca_plan_shift name it.  2 scenarios.  This runs more than one
    MPC step, on purpose: k0 is at most 2^31 - 1, so the limit k0 + k < 2^31 is first missed at k = 1,
    after one whole step, and piadmm_obca_plan_shift refuses only a step whose iterates have all run;
    so one MPC step runs and then the iterates of the next (max_admm_iter <= 2)."""
    b, _ = batches
    unit = obca.noise_row(sigma=1.0)
    _expect(-1, "obca_noise_tape: rows must be 1 or n \\(4\\)$", b.noise_tape, 4, 1, np.stack([unit, unit]))
    _expect(-1, "obca_noise_tape: streams\\[1\\] must be >= 0$", b.noise_tape, 2, 1, unit, [0, -1])
    _expect(-1, "obca_noise_tape: k0 >= 0 and every step index below 2\\^31$", b.noise_tape, 2, 1, unit, None, 0, -1)
    _expect(-1, "obca_noise_tape: k0 >= 0 and every step index below 2\\^31$", b.noise_tape, 2, 2, unit, None, 0, 2 ** 31 - 1)
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR[:2]), **_kw(CASES[:2]))
    _expect(-1, "obca_noise_plan: rows must be 1 or n \\(2\\)$", pl.set_noise, par=ZPAR)
    _expect(-1, "obca_noise_plan: streams\\[1\\] must be >= 0$", pl.set_noise, par=ZPAR[:2], streams=[0, -1])
    _expect(-1, "obca_noise_plan: k0 >= 0 and every step index below 2\\^31$", pl.set_noise, par=ZPAR[:2], k0=-1)
    pl.set_noise(par=ZPAR[:2], k0=2 ** 31 - 1)
    pl.step()
    _expect(-3, "obca_plan_step: noise step index exhausted$", pl.step)
    while pl.iterate():
        pass
    _expect(-3, "obca_plan_shift: noise step index exhausted$", pl.shift)
    assert pl.feedback_steps() == 1
    pl.close()
