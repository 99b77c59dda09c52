"""The loop of the device OBCA plan (k_loop_close, k_loop_open and k_loop_draw in
csrc/piadmm_obca_plan_loop.hip behind piadmm_obca_loop_plan / _loop_admit / _loop_draw;
OBCADevicePlanner(clock=, loop=), set_loop, clear_loop, loop_tau, admit(loop=), the LOOP_ items of `get`
and the loop section of the tenant records).

Bars.  Every comparison is bit equality between two device results: the draws against the device
outputs of piadmm_obca_noise_tape / _delay_tau at each scenario's own step index, the clocked plan
with the loop against unclocked plans with feedback + noise + delay, a blob against
piadmm.obca.tenant_pack of the plan's own items.  Nothing is compared with a NumPy draw.

6 fleet scenarios (the cases of tests/_obca_fleet_cases.py), max_admm_iter <= 2, 3 MPC steps.  The
one-scenario yardstick runs are computed once per (scenario, start) and never changed."""
import numpy as np
import pytest

import _obca_dual_cases as D
import _obca_fleet_cases as F
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

_bits = P._bits
CASES, N, N_REF, STEPS = [0, 1, 2, 3, 0, 1], 6, 51, 3
ITEMS = ("STATE", "STATE_PREV", "X", "CTRL", "LAMBDA", "ITERS", "STATUS_MASK")
PLANT = np.stack([obca.feedback_row(method=s % 2, n_sub=1 + s % 3, gain_a=1.0 - 0.02 * s, lr=(1.0, 1.0 + 0.02 * s))
                  for s in range(N)])
NOISE = np.stack([obca.noise_row(sigma=0.004 * (s + 1), bias=0.0005 * s, trunc=0.0 if s % 2 else 1.5) for s in range(N)])
DELAY = np.stack([obca.delay_row(avg=(0.03, 0.02 + 0.01 * s), std=0.04, tau_max=(0.1, 0.08), trunc=1.5) for s in range(N)])
STREAMS = np.array([5, 2 ** 32 + 1, 2 ** 63 - 1, 9, 2 ** 40 + 3, 0], np.int64)
SEED, K0 = 2 ** 63 + 12345, 7
LOOP = dict(plant=PLANT, noise=NOISE, delay=DELAY, streams=STREAMS, seed=SEED, k0=K0)
LOOP_NAMES = ("LOOP_PLANT", "LOOP_NOISE", "LOOP_DELAY", "LOOP_TAU", "LOOP_STREAMS", "LOOP_SEED")


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


def _kw(cases=CASES, t0=0, **extra):
    return dict(F.fleet_kwargs(list(cases), t0), **extra)


def _items(pl, names=ITEMS):
    return {k: pl.get(k).copy() for k in names}


def _expect(code, what, call, *a, **k):
    with pytest.raises(_lib.PiadmmError, match=what) as e:
        call(*a, **k)
    assert f"error {code}:" in str(e.value), str(e.value)


def _clock(c0, length=None):
    length = [N_REF] * len(c0) if length is None else length
    return np.array(list(zip(c0, length)), np.int32)


_ALONE = {}


def _alone(ref, case, c0, plant, noise, delay, stream, steps=STEPS):
    """A one-scenario unclocked fleet plan started at t_step0 = c0 with feedback + noise + delay at
    k0 + c0: per step (the latency the step ran under, the items after it), and the open latency."""
    key = (case, c0, plant.tobytes(), noise.tobytes(), delay.tobytes(), int(stream), steps)
    if key not in _ALONE:
        draw = dict(streams=[int(stream)], seed=SEED, k0=K0 + c0)
        pl = obca.OBCADevicePlanner(ref, feedback=dict(par=plant), noise=dict(par=noise, **draw),
                                    delay=dict(par=delay, **draw), **_kw([case], c0))
        out = []
        for _ in range(steps):
            tau = pl.get("DELAY_TAU")[0].copy()
            pl.step()
            out.append((tau, {k: v[0] for k, v in _items(pl).items()}))
        _ALONE[key] = (out, pl.get("DELAY_TAU")[0].copy())
        pl.close()
    return _ALONE[key]


def _same_scenario(pl, s, want, what):
    got = _items(pl)
    for k in ITEMS:
        _bits(got[k][s], want[k], f"{what}: {k} of scenario {s}")


# ---------------------------------------------------------------------------------------------
# 1. the draw alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("each", (False, True))
def test_loop_draw_alone(batches, each):
    b, ref = batches
    n, k0 = 130, 5                                    # 260 lanes: the draw crosses a 256-lane workgroup
    rng = np.random.default_rng(3)
    c = rng.integers(0, 40, n)
    c[[0, 64, 129]] = (0, 2 ** 30, 2 ** 30)
    c[7] = 0
    clock = np.ascontiguousarray(np.stack((c, np.full(n, 51), np.ones(n, int)), axis=1), np.int32)
    streams = rng.integers(0, 2 ** 62, n).astype(np.int64)
    streams[:3] = (0, 2 ** 32 + 1, 2 ** 63 - 1)
    noise = np.stack([obca.noise_row(sigma=0.01 * (1 + s % 5), bias=0.001 * s, trunc=0.0 if s % 3 else 1.25) for s in range(n)])
    delay = np.stack([obca.delay_row(avg=(0.03, 0.02 + 0.0003 * s), std=0.04, tau_max=(0.1, 0.08), trunc=2.0) for s in range(n)])
    if not each:
        noise, delay = noise[1], delay[1]
    w, tau = b.loop_draw(clock, noise, delay, streams, SEED, k0)
    assert w.shape == (n, 2, 5) and tau.shape == (n, 2) and w.all() and tau.any()
    for cv in np.unique(c):
        # the device's tape and latencies at this step index: one row, every stream
        tape = ref.noise_tape(n, 1, noise, streams, SEED, k0 + int(cv))[:, 0]
        lat = ref.delay_tau(n, 1, delay, streams, SEED, k0 + int(cv))[:, 0]
        at = c == cv
        _bits(w[at], tape[at], f"w at clock {cv}")
        _bits(tau[at], lat[at], f"tau at clock {cv}")
    # an absent kind draws zeros; streams=None is 0 .. n-1
    _bits(b.loop_draw(clock, None, delay, streams, SEED, k0)[0], np.zeros((n, 2, 5)), "no noise")
    _bits(b.loop_draw(clock, noise, None, streams, SEED, k0)[1], np.zeros((n, 2)), "no delay")
    _bits(b.loop_draw(clock, noise, None, streams, SEED, k0)[0], w, "the noise does not depend on the delay")
    got = b.loop_draw(clock, noise, delay, None, SEED, k0)
    want = b.loop_draw(clock, noise, delay, np.arange(n), SEED, k0)
    _bits(got[0], want[0], "streams=None")
    _bits(got[1], want[1], "streams=None")
    bad = clock.copy()
    bad[5, 0] = -1
    _expect(-1, "obca_loop_draw: row 5: c >= 0", b.loop_draw, bad, noise, delay, streams, SEED, k0)
    _expect(-1, "obca_loop_draw: row 64: .*2\\^31", b.loop_draw, clock, noise, delay, streams, SEED, 2 ** 30)
    if each:
        bad = delay.copy()
        bad[3, 4] = 0.2
        _expect(-1, "obca_loop_draw: delay row 3: .*tau_max", b.loop_draw, clock, noise, bad, streams, SEED, k0)


# ---------------------------------------------------------------------------------------------
# 2. every clock at zero: the unclocked closed loop
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("extras", (False, True))
def test_clock_at_zero_is_the_old_closed_loop(batches, extras):
    b, ref = batches
    more = dict(dual=D.fleet_gains(CASES), order=True) if extras else {}
    draw = dict(streams=STREAMS, seed=SEED, k0=K0)
    old = obca.OBCADevicePlanner(ref, feedback=dict(par=PLANT), noise=dict(par=NOISE, **draw), delay=dict(par=DELAY, **draw),
                                 **_kw(**more))
    new = obca.OBCADevicePlanner(b, clock=True, loop=LOOP, **_kw(**more))
    _bits(new.get("LOOP_PLANT"), PLANT, "LOOP_PLANT")
    _bits(new.get("LOOP_NOISE"), NOISE, "LOOP_NOISE")
    _bits(new.get("LOOP_DELAY"), DELAY, "LOOP_DELAY")
    _bits(new.get("LOOP_STREAMS"), STREAMS, "LOOP_STREAMS")
    assert new.get("LOOP_SEED").tolist() == [SEED, K0, 7]
    for step in range(STEPS):
        _bits(new.loop_tau(), old.get("DELAY_TAU"), f"the latencies of step {step}")
        assert new.loop_tau().any()
        old.step()
        new.step()
        got, want = _items(new), _items(old)
        for k in ITEMS:
            _bits(got[k], want[k], f"{k} after step {step + 1}")
    _bits(new.loop_tau(), old.get("DELAY_TAU"), "the open latencies")
    assert new.clock()[:, 0].tolist() == [STEPS] * N
    old.close()
    new.close()


# ---------------------------------------------------------------------------------------------
# 3. mixed phases and retiring
# ---------------------------------------------------------------------------------------------
C0 = (0, 2, 0, 1, 2, 0)
LEN = (N_REF, 10, N_REF, N_REF, 11, N_REF)          # scenario 1 retires after step 1, scenario 4 after step 2
FROZEN = ("STATE", "STATE_PREV", "X", "CTRL", "LAMBDA")


def test_mixed_phases_and_retiring(batches):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    ran = {s: 0 for s in range(N)}
    frozen = {}
    for step in range(STEPS):
        alive = pl.alive().copy()
        assert alive.tolist() == [True, step < 1, True, True, step < 2, True]
        tau = pl.loop_tau()
        pl.step()
        got = _items(pl)
        for s in range(N):
            out, _ = _alone(ref, CASES[s], C0[s], PLANT[s], NOISE[s], DELAY[s], STREAMS[s])
            if alive[s]:
                _bits(tau[s], out[ran[s]][0], f"step {step}: the latency of scenario {s}")
                _same_scenario(pl, s, out[ran[s]][1], f"after step {step + 1}")
                ran[s] += 1
                if not pl.alive()[s]:
                    frozen[s] = ({k: got[k][s].copy() for k in FROZEN}, pl.loop_tau()[s].copy())
            else:
                # retired: every item, the latency included, stays (ITERS and STATUS_MASK are the step's own)
                for k in FROZEN:
                    _bits(got[k][s], frozen[s][0][k], f"frozen after step {step + 1}: {k} of scenario {s}")
                _bits(pl.loop_tau()[s], frozen[s][1], f"the frozen latency of scenario {s}")
    assert sorted(frozen) == [1, 4] and ran == {0: 3, 1: 1, 2: 3, 3: 3, 4: 2, 5: 3}
    # a retired scenario's latency is the one its last step ran under; an alive one's is the open step's
    for s in range(N):
        out, open_tau = _alone(ref, CASES[s], C0[s], PLANT[s], NOISE[s], DELAY[s], STREAMS[s])
        _bits(pl.loop_tau()[s], out[ran[s] - 1][0] if s in frozen else open_tau, f"the last latency of scenario {s}")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 4. admission
# ---------------------------------------------------------------------------------------------
def test_admission(batches):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    pl.step()
    assert not pl.alive()[1]
    before = {k: pl.get(k).copy() for k in LOOP_NAMES}
    # clock_admit alone: the slot keeps its rows and stream, the latency is drawn at the new c0
    pl.admit([1], _clock([5]), specs=[F.SPECS[CASES[1]]])
    for k in ("LOOP_PLANT", "LOOP_NOISE", "LOOP_DELAY", "LOOP_STREAMS", "LOOP_SEED"):
        _bits(pl.get(k), before[k], f"{k} after clock_admit")
    out, _ = _alone(ref, CASES[1], 5, PLANT[1], NOISE[1], DELAY[1], STREAMS[1], steps=1)
    _bits(pl.loop_tau()[1], out[0][0], "the latency at the new c0")
    others = [0, 2, 3, 4, 5]
    _bits(pl.loop_tau()[others], before["LOOP_TAU"][others], "the other latencies")
    # clock_admit + loop_admit: a fresh tenant with its own rows and stream
    plant, noise = obca.feedback_row(method=1, n_sub=3, gain_w=0.9), obca.noise_row(sigma=0.003, bias=0.001)
    delay, stream = obca.delay_row(avg=0.04, std=0.03, trunc=1.0), 2 ** 50 + 1
    pl.admit([1], _clock([3]), specs=[F.SPECS[2]], par=pl.get("PAR")[2:3], prob=[F.ROWS["prob"][2]],
             primal_thres=pl.get("PRIMAL_THRES")[2:3], dual_thres=pl.get("DUAL_THRES")[2:3],
             loop=dict(plant=plant, noise=noise, delay=delay, streams=[stream]))
    _bits(pl.get("LOOP_PLANT")[1], plant, "the admitted plant row")
    _bits(pl.get("LOOP_NOISE")[1], noise, "the admitted noise row")
    _bits(pl.get("LOOP_DELAY")[1], delay, "the admitted delay row")
    assert pl.get("LOOP_STREAMS")[1] == stream
    _bits(np.delete(pl.get("LOOP_PLANT"), 1, axis=0), np.delete(PLANT, 1, axis=0), "the other plant rows")
    out, open_tau = _alone(ref, 2, 3, plant, noise, delay, stream, steps=2)
    for step in range(2):
        _bits(pl.loop_tau()[1], out[step][0], f"the tenant's latency of step {step}")
        pl.step()
        _same_scenario(pl, 1, out[step][1], f"the admitted tenant after step {step + 1}")
    _bits(pl.loop_tau()[1], open_tau, "the tenant's open latency")
    # the tenants around it went on as if nothing happened
    for s in (0, 3):
        ref_out, _ = _alone(ref, CASES[s], C0[s], PLANT[s], NOISE[s], DELAY[s], STREAMS[s])
        _same_scenario(pl, s, ref_out[2][1], "a neighbour after three steps")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 5. tenants
# ---------------------------------------------------------------------------------------------
def test_tenants_move_with_the_loop(batches, tmp_path):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    pl.step()
    slots = [4, 1, 0]                                 # scenario 1 is retired
    blob = pl.export_tenants(slots)
    want = obca.tenant_pack(pl.tenant_items(), slots, N_REF, update_lamb_ij=0, loop=True)
    _bits(np.frombuffer(blob, np.uint8), want, "the blob against tenant_pack")
    t = obca.tenant_unpack(blob)
    assert t["loop"] == 7 and t["LOOP_SEED"].tolist() == [SEED, K0, 7]
    _bits(t["LOOP_TAU"], pl.loop_tau()[slots], "the records' latencies")
    # into other slots of a second plan with the same loop (other rows there): they continue bit for bit
    other = obca.OBCADevicePlanner(ref, clock=_clock([1] * N), loop=dict(LOOP, plant=PLANT[::-1].copy(), streams=STREAMS[::-1].copy()),
                                   **_kw([3, 2, 1, 0, 3, 2]))
    dst = [2, 5, 3]
    other.import_tenants(dst, blob)
    assert other.alive()[dst].tolist() == [True, False, True]
    for k, (s, d) in enumerate(zip(slots, dst)):
        _bits(other.get("LOOP_PLANT")[d], PLANT[s], "the plant row travelled")
        assert other.get("LOOP_STREAMS")[d] == STREAMS[s]
        _bits(other.loop_tau()[d], pl.loop_tau()[s], "the latency travelled")
    for step in range(2):
        pl.step()
        other.step()
        a, o = _items(pl), _items(other)
        for s, d in zip(slots, dst):
            for k in ITEMS:
                _bits(o[k][d], a[k][s], f"{k} of the moved tenant {s}, {step + 1} steps on")
            _bits(other.loop_tau()[d], pl.loop_tau()[s], f"the latency of the moved tenant {s}")
    other.close()
    # compact and save / load: the alive tenants go on bit for bit
    twin = obca.OBCADevicePlanner(ref, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    twin.run(3)
    alive = np.flatnonzero(pl.alive())
    assert alive.tolist() == [0, 2, 3, 5]
    path = pl.save(str(tmp_path / "plan"))
    small = pl.compact()
    assert small.n == 4 and small.get("LOOP_SEED").tolist() == [SEED, K0, 7]
    _bits(small.loop_tau(), twin.loop_tau()[alive], "the latencies after compact()")
    small.step()
    twin.step()
    a, o = _items(twin), _items(small)
    for k in ITEMS:
        _bits(o[k], a[k][alive], f"{k} one step after compact()")
    small.close()
    back = obca.OBCADevicePlanner.load(b, path)
    back.step()
    o = _items(back)
    for k in ITEMS:
        _bits(o[k], a[k], f"{k} one step after load()")
    _bits(back.loop_tau(), twin.loop_tau(), "the latencies one step after load()")
    back.close()
    twin.close()


def test_shared_row_plan_refuses_a_differing_record(batches):
    b, ref = batches
    src = obca.OBCADevicePlanner(ref, clock=True, loop=LOOP, **_kw())
    blob = src.export_tenants([2, 3])
    shared = obca.OBCADevicePlanner(b, clock=True, loop=dict(LOOP, noise=NOISE[2]), **_kw())
    before = {k: shared.get(k).copy() for k in ITEMS + LOOP_NAMES + ("CLOCK",)}
    _expect(-1, "obca_tenant_import: row 1: the noise row differs from the plan's shared one", shared.import_tenants, [0, 1], blob)
    for k, v in before.items():
        _bits(shared.get(k), v, f"{k} after the refusal")
    shared.import_tenants([0], src.export_tenants([2]))           # the equal row is taken
    _bits(shared.get("LOOP_NOISE"), NOISE[2:3], "the shared row stays one row")
    # the loop in one and not in the other, another seed, other row kinds
    bare = obca.OBCADevicePlanner(b, clock=True, **_kw())
    _expect(-3, "the blob carries the loop, the plan has none attached", bare.import_tenants, [0, 1], blob)
    plain_blob = bare.export_tenants([0, 1])
    assert obca.tenant_unpack(plain_blob)["loop"] == 0
    lp = obca.OBCADevicePlanner(b, clock=True, loop=dict(LOOP, seed=SEED + 1), **_kw())
    _expect(-3, "the plan has the loop attached, the blob carries none", lp.import_tenants, [0, 1], plain_blob)
    _expect(-1, "the loop's seed or k0 differ", lp.import_tenants, [0, 1], blob)
    lp.set_loop(**dict(LOOP, delay=None))
    _expect(-1, "the loop's row kinds differ", lp.import_tenants, [0, 1], blob)
    lp.close()
    src.close()


# ---------------------------------------------------------------------------------------------
# 6. the trace
# ---------------------------------------------------------------------------------------------
def test_traced_run_is_the_stepwise_run(batches):
    b, ref = batches
    a = obca.OBCADevicePlanner(ref, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    a.run(STEPS)
    t = obca.OBCADevicePlanner(b, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    tr = t.run_traced(STEPS)
    got, want = _items(t), _items(a)
    for k in ITEMS:
        _bits(got[k], want[k], f"{k} after the traced run")
    _bits(t.loop_tau(), a.loop_tau(), "the latencies after the traced run")
    # the trace's state rows are the states the plant reached
    _bits(tr.states, np.asarray(a.record.state_record), "the trace's states")
    _bits(np.asarray(t.record.state_record), np.asarray(a.record.state_record), "state_record")
    x1 = want["X"][:, :, 1]
    assert not np.array_equal(tr.states[-1][[0, 2, 3, 5]], x1[[0, 2, 3, 5]])
    # admission under a trace stays refused
    t.trace_begin(1)
    _expect(-3, "obca_clock_admit: a trace is attached", t.admit, [1], _clock([3]))
    _expect(-3, "obca_loop_admit: a trace is attached", t.loop_admit, [1], streams=[4])
    t.trace_end()
    a.close()
    t.close()


# ---------------------------------------------------------------------------------------------
# 7. refusals
# ---------------------------------------------------------------------------------------------
def test_refusals_leave_the_plan_alone(batches):
    b, ref = batches
    names = ITEMS + ("CLOCK", "WINDOW", "PAR", "CTRL_PREV")
    # the loop without a clock, next to feedback, next to the delay
    pl = obca.OBCADevicePlanner(b, **_kw())
    before = _items(pl, ITEMS + ("PAR", "CTRL_PREV"))
    _expect(-3, "obca_loop_plan: no clock attached", pl.set_loop, **LOOP)
    pl.set_feedback(par=PLANT)
    _expect(-3, "obca_loop_plan: feedback is attached", pl.set_loop, **LOOP)
    pl.clear_feedback()
    pl.set_delay(par=DELAY)
    _expect(-3, "obca_loop_plan: the delay is attached", pl.set_loop, **LOOP)
    pl.clear_delay()
    _expect(-3, "obca_plan_get: no loop attached", pl.get, "LOOP_TAU")
    for k in before:
        _bits(pl.get(k), before[k], f"{k} after the refusals")
    pl.close()
    # on a clocked plan: the arguments, then an earlier loop stays as it was
    pl = obca.OBCADevicePlanner(b, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    before = _items(pl, names + LOOP_NAMES)
    for kind, rows, col, val, word in (("plant", PLANT, 1, 65.0, "n_sub"), ("noise", NOISE, 3, -1.0, "sigma"),
                                       ("delay", DELAY, 4, 0.2, "tau_max")):
        bad = rows.copy()
        bad[4, col] = val
        _expect(-1, f"obca_loop_plan: {kind} row 4: .*{word}", pl.set_loop, **dict(LOOP, **{kind: bad}))
    _expect(-1, "obca_loop_plan: plant rows must be 1 or n", pl.set_loop, **dict(LOOP, plant=PLANT[:2]))
    _expect(-1, "obca_loop_plan: streams\\[2\\] must be >= 0", pl.set_loop, **dict(LOOP, streams=[0, 1, -2, 3, 4, 5]))
    _expect(-1, "obca_loop_plan: k0 >= 0", pl.set_loop, **dict(LOOP, k0=-1))
    _expect(-3, "obca_loop_plan: loop step index exhausted", pl.set_loop, **dict(LOOP, k0=2 ** 31 - 2))
    _expect(-3, "obca_clock_plan: the loop is attached", pl.clear_clock)
    _expect(-3, "obca_clock_plan: the loop is attached", pl.set_clock, _clock(C0, LEN))
    _expect(-3, "obca_feedback_plan: a clock is attached", pl.set_feedback)
    _expect(-3, "obca_delay_plan: a clock is attached", pl.set_delay)
    _expect(-1, "obca_loop_admit: noise row 0: .*sigma", pl.loop_admit, [2], noise=-NOISE[1])
    _expect(-1, "obca_loop_admit: slots\\[1\\]", pl.loop_admit, [2, 2])
    pl.iterate()
    _expect(-3, "obca_loop_plan: only at a step boundary", pl.set_loop, **LOOP)
    _expect(-3, "obca_loop_plan: only at a step boundary", pl.clear_loop)
    _expect(-3, "obca_loop_admit: only at a step boundary", pl.loop_admit, [2], streams=[1])
    for k in LOOP_NAMES + ("CLOCK", "WINDOW", "PAR"):
        _bits(pl.get(k), before[k], f"{k} after the refusals")
    pl.close()
    # shared rows: loop_admit of that kind is refused, the other kinds are taken
    pl = obca.OBCADevicePlanner(b, clock=True, loop=dict(LOOP, delay=DELAY[0], noise=None), **_kw())
    assert pl.get("LOOP_SEED").tolist() == [SEED, K0, 5]
    _expect(-3, "obca_plan_get: the loop has no noise rows", pl.get, "LOOP_NOISE")
    _expect(-3, "obca_loop_admit: delay needs a loop with a delay row per scenario", pl.loop_admit, [2], delay=DELAY[1])
    _expect(-3, "obca_loop_admit: noise needs a loop with a noise row per scenario", pl.loop_admit, [2], noise=NOISE[1])
    pl.loop_admit([2], plant=PLANT[0], streams=[77])
    assert pl.get("LOOP_STREAMS")[2] == 77
    # the step index limit: the mirror refuses before any launch
    pl.set_loop(**dict(LOOP, k0=2 ** 31 - 1))
    pl.iterate()
    while pl.counts()[1]:
        pl.iterate()
    _expect(-3, "obca_plan_shift: loop step index exhausted", pl.shift)
    pl.close()
    pl = obca.OBCADevicePlanner(b, clock=True, loop=dict(LOOP, k0=2 ** 31 - 1), **_kw())
    _expect(-3, "obca_plan_step: loop step index exhausted", pl.step)
    pl.trace_begin(2)
    _expect(-3, "obca_trace_run: loop step index exhausted before 1 steps$", pl.trace_run, 1)
    pl.trace_end()
    # detaching gives the clocked plan without the loop: today's bits
    pl.clear_loop()
    bare = obca.OBCADevicePlanner(ref, clock=True, **_kw())
    pl.step()
    bare.step()
    got, want = _items(pl), _items(bare)
    for k in ITEMS:
        _bits(got[k], want[k], f"{k}: the clocked plan without the loop")
    pl.close()
    bare.close()


def test_import_refuses_a_bad_loop_section_on_the_device(batches):
    """piadmm_obca_tenant_import's own checks of the loop section and of the header's loop words: each
    refusal's code and text, every item unchanged; then what it takes of a record's latency."""
    b, ref = batches
    src = obca.OBCADevicePlanner(ref, clock=_clock(C0, LEN), loop=LOOP, **_kw())
    src.step()                                        # scenario 1 is retired
    good = np.frombuffer(src.export_tenants([0, 1]), np.uint8).copy()
    lay = obca.tenant_layout(N_REF, loop=True)
    dst = obca.OBCADevicePlanner(b, clock=True, loop=LOOP, **_kw())
    names = ITEMS + LOOP_NAMES + ("CLOCK", "WINDOW", "PAR", "REF", "PROB")
    before = _items(dst, names)

    def patched(k, name, at, value):
        """record k's word `at` of the segment `name` set to value (a double, or an int64's bits)."""
        blob = good.copy()
        o = 64 + k * lay["record_bytes"] + 8 * (lay["f64"][name][0] + at)
        blob[o:o + 8] = np.array([value], np.int64 if isinstance(value, int) else np.float64).view(np.uint8)
        return blob

    def header(word, value):
        blob = good.copy()
        blob[:64].view(np.int32)[word] = value
        return blob
    cases = (
        (patched(1, "LOOP_PLANT", 1, 65.0), -1, "obca_tenant_import: row 1: plant: 1 <= n_sub <= 64"),
        (patched(0, "LOOP_PLANT", 8 + 2, 0.0), -1, "obca_tenant_import: row 0: plant: lr, lf > 0"),
        (patched(1, "LOOP_NOISE", 3, -1.0), -1, "obca_tenant_import: row 1: noise: sigma >= 0"),
        (patched(0, "LOOP_NOISE", 21, 1.0), -1, "obca_tenant_import: row 0: noise: the reserved entry"),
        (patched(1, "LOOP_DELAY", 4, 0.2), -1, "obca_tenant_import: row 1: delay: 0 <= tau_max <= DT"),
        (patched(0, "LOOP_DELAY", 2, float("nan")), -1, "obca_tenant_import: row 0: delay: every entry finite"),
        (patched(1, "LOOP_TAU", 1, float(np.nextafter(obca.DT, 1.0))), -1, "obca_tenant_import: row 1: tau must be in \\[0, DT\\]"),
        (patched(0, "LOOP_TAU", 0, -1e-9), -1, "obca_tenant_import: row 0: tau must be in"),
        (patched(0, "LOOP_TAU", 1, float("nan")), -1, "obca_tenant_import: row 0: tau must be in"),
        (patched(1, "LOOP_STREAMS", 0, -1), -1, "obca_tenant_import: row 1: the stream id must be >= 0"),
        (header(11, 6), -1, "obca_tenant_import: bad header"),                 # kinds without the loop's bit
        (header(11, 15), -1, "obca_tenant_import: bad header"),                # an unknown flag bit
        (header(15, 1), -1, "obca_tenant_import: bad header"),
        (header(14, -1), -1, "obca_tenant_import: bad header"),
        (header(11, 0), -1, "obca_tenant_import: bad header"),                 # the section without its flag
        (header(11, 5), -1, "obca_tenant_import: the loop's row kinds differ"),      # a well-formed header of other kinds
        (header(14, K0 + 1), -1, "obca_tenant_import: the loop's seed or k0 differ"),
        (header(12, 1), -1, "obca_tenant_import: the loop's seed or k0 differ"),
    )
    for blob, code, text in cases:
        _expect(code, text, dst.import_tenants, [3, 4], blob)
        for k, v in before.items():
            _bits(dst.get(k), v, f"{k} after: {text}")
    # the step index limit: a plan at a large k0 takes the blob's header only with its own k0, and an
    # alive record whose k0 + c reaches 2^31 is refused; clock_admit refuses the same before any change
    far = obca.OBCADevicePlanner(b, clock=True, loop=dict(LOOP, k0=2 ** 31 - 1), **_kw())
    before = _items(far, names)
    _expect(-1, "obca_tenant_import: row 0: loop step index exhausted", far.import_tenants, [3, 4], header(14, 2 ** 31 - 1))
    _expect(-3, "obca_clock_admit: row 0: loop step index exhausted", far.admit, [2], _clock([1]))
    for k, v in before.items():
        _bits(far.get(k), v, f"{k} after the step index refusals")
    far.close()
    # a valid latency that is not the draw: the alive tenant's is drawn again, the retired one's travels
    dst = obca.OBCADevicePlanner(b, clock=True, loop=LOOP, **_kw())
    odd = patched(0, "LOOP_TAU", 0, 0.0123)
    odd[64 + lay["record_bytes"] + 8 * lay["f64"]["LOOP_TAU"][0]:][:8] = np.array([0.0456]).view(np.uint8)
    dst.import_tenants([3, 4], odd)
    _bits(dst.loop_tau()[3], src.loop_tau()[0], "the alive tenant's latency is the draw")
    assert dst.loop_tau()[4, 0] == 0.0456 and not dst.alive()[4]
    _bits(dst.loop_tau()[4, 1:], src.loop_tau()[1, 1:], "the retired tenant's other latency")
    src.step()
    dst.step()
    a, o = _items(src), _items(dst)
    for k in ITEMS:
        _bits(o[k][3], a[k][0], f"{k} of the moved tenant one step on")
    dst.close()
    src.close()


def test_loop_draw_refuses_n_out_of_range(batches):
    b, _ = batches
    h, lib = b._h, b._lib
    one = np.zeros((1, 3), np.int32)
    w, tau = np.zeros((1, 2, 5)), np.zeros((1, 2))
    for n in (0, -1, 2 ** 20 + 1):
        rc = lib.piadmm_obca_loop_draw(h, n, _lib.iptr(one), None, 0, None, 0, None, 0, 0, _lib.dptr(w), _lib.dptr(tau))
        assert rc == -1 and b"obca_loop_draw: 1 <= n <= 2^20" in lib.piadmm_obca_last_error(h), n
    rc = lib.piadmm_obca_loop_draw(h, 1, None, None, 0, None, 0, None, 0, 0, _lib.dptr(w), _lib.dptr(tau))
    assert rc == -1 and b"obca_loop_draw: null argument" in lib.piadmm_obca_last_error(h)
    rc = lib.piadmm_obca_loop_draw(h, 1, _lib.iptr(one), None, 0, None, 0, None, 0, -1, _lib.dptr(w), _lib.dptr(tau))
    assert rc == -1 and b"obca_loop_draw: k0 >= 0" in lib.piadmm_obca_last_error(h)
    assert not w.any() and not tau.any()
    # n = 1 draws
    assert lib.piadmm_obca_loop_draw(h, 1, _lib.iptr(one), _lib.dptr(NOISE[1:2].copy()), 1, _lib.dptr(DELAY[1:2].copy()), 1, None,
                                     SEED, 0, _lib.dptr(w), _lib.dptr(tau)) == 0
    assert w.all() and tau.any()


def test_refusal_texts_in_full(batches):
    """The argument refusals of piadmm_obca_loop_draw and piadmm_obca_loop_admit, to their last word.
    2 scenarios, no MPC step."""
    b, _ = batches
    clock = np.array([[0, N_REF, 1], [3, N_REF, 1]], np.int32)
    late = DELAY[:2].copy()
    late[1, 4] = 0.2
    loud = NOISE[:2].copy()
    loud[1, 3] = -1.0
    _expect(-1, "obca_loop_draw: noise rows must be 1 or n \\(2\\)$", b.loop_draw, clock, NOISE[:3])
    _expect(-1, "obca_loop_draw: delay rows must be 1 or n \\(2\\)$", b.loop_draw, clock, None, DELAY[:3])
    _expect(-1, "obca_loop_draw: noise row 1: sigma >= 0$", b.loop_draw, clock, loud)
    _expect(-1, "obca_loop_draw: delay row 1: 0 <= tau_max <= DT$", b.loop_draw, clock, None, late)
    _expect(-1, "obca_loop_draw: streams\\[1\\] must be >= 0$", b.loop_draw, clock, NOISE[:2], DELAY[:2], [4, -1])
    _expect(-1, "obca_loop_draw: row 1: c >= 0 and the step index k0 \\+ c below 2\\^31$", b.loop_draw, clock, NOISE[:2],
            None, None, 0, 2 ** 31 - 3)
    loop = dict(plant=PLANT[:2], noise=NOISE[:2], delay=DELAY[:2], streams=STREAMS[:2], seed=SEED, k0=K0)
    pl = obca.OBCADevicePlanner(b, clock=True, loop=loop, **_kw(CASES[:2]))
    before = _items(pl, LOOP_NAMES)
    coarse = PLANT[:1].copy()
    coarse[0, 1] = 65.0
    _expect(-1, "obca_loop_admit: streams\\[0\\] must be >= 0$", pl.loop_admit, [1], streams=[-3])
    _expect(-1, "obca_loop_admit: plant row 0: 1 <= n_sub <= 64, an integer$", pl.loop_admit, [1], plant=coarse)
    _expect(-1, "obca_loop_admit: delay row 0: 0 <= tau_max <= DT$", pl.loop_admit, [0], delay=late[1:])
    for k in LOOP_NAMES:
        _bits(pl.get(k), before[k], f"{k} after the refusals")
    pl.close()
