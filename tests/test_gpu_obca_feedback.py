"""Closed-loop feedback of the device-resident OBCA-ADMM plan (k_plan_propagate and k_plan_set_init
in csrc/piadmm_obca_plan_feedback.hip behind piadmm_obca_propagate / piadmm_obca_feedback_plan /
piadmm_obca_feedback_measure; OBCABatch.propagate, OBCADevicePlanner(feedback=...), set_feedback,
clear_feedback, measure, feedback_steps; OBCAPlanner(feedback=...)).

Bars.  The kernel alone is compared with the host statement obca.propagate at
_obca_feedback_cases.PROPAGATE_TOL (device libm is not NumPy's; the figure is 8 times the largest
deviation measured over these cases).  Everything else is bit equality: the in-plan step against the
stand-alone call on the same inputs, the rest of the shift against the same plan without feedback,
the next step against a plain plan opened from the state the vehicle reached.

3 fleet scenarios with different OvertakeSpecs, max_admm_iter <= 2, t_step0 = 12, 2 MPC steps.  The
yardstick runs are computed once and never changed."""
import numpy as np
import pytest

import _obca_dual_cases as D
import _obca_feedback_cases as C
import _obca_fleet_cases as F
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

_bits = P._bits
CASES, T0, N = [0, 1, 2], 12, 3
S_INIT = 546
ITEMS = ("STATE", "STATE_PREV", "X", "CTRL", "CTRL_PREV", "ITERS", "PRIMAL", "DUAL", "STATUS_MASK", "LAMBDA")
# plant rows off nominal, one per scenario, and two disturbance rows per scenario
PAR = np.stack([obca.feedback_row(method=1, n_sub=4, lr=1.1, lf=1.4, gain_a=0.9),
                obca.feedback_row(n_sub=(2, 64), gain_w=(1.2, 0.7), a_max=(0.5, 5.0)),
                obca.feedback_row()])
TAPE = np.random.default_rng(7).normal(0.0, (0.05, 0.05, 0.02, 0.002, 0.001), (N, 2, 2, 5))


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


def _kw(**extra):
    return dict(F.fleet_kwargs(CASES, T0), **extra)


def _items(pl, names=ITEMS):
    return {k: pl.get(k).copy() for k in names}


def _iterate_out(pl):
    """Every iterate of the open step, without the shift."""
    first = True
    while first or pl.counts()[1]:
        pl.iterate()
        first = False


def _u0(ctrl):
    """(a, omega) of slot 0 per vehicle from the CTRL item (n x 2 x 14: U[:, 0], then U[:, 1])."""
    return np.ascontiguousarray(np.stack((ctrl[:, :, 0], ctrl[:, :, obca.NT]), axis=-1))


def _init(state):
    return np.ascontiguousarray(state[:, S_INIT:].reshape(-1, 2, 5))


def _expect(code, what, call, *a, **k):
    with pytest.raises(_lib.PiadmmError, match=what) as e:
        call(*a, **k)
    assert f"error {code}:" in str(e.value), str(e.value)


@pytest.fixture(scope="module")
def plain(batches):
    """The fleet without feedback: the items after step 1."""
    _, ref = batches
    pl = obca.OBCADevicePlanner(ref, **_kw())
    pl.step()
    out = _items(pl)
    pl.close()
    return out


@pytest.fixture(scope="module")
def closed(batches):
    """The fleet with PAR and TAPE: what step 1 read (init_state, CTRL) before its shift, the items
    after step 1, the items of step 2 before and after its shift."""
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR, tape=TAPE), **_kw())
    assert pl.feedback_steps() == 0
    _bits(pl.get("FEEDBACK_PAR"), PAR, "FEEDBACK_PAR")
    _iterate_out(pl)
    x0, ctrl = _init(pl.get("STATE")), pl.get("CTRL")
    iters1 = pl.get("ITERS")
    pl.shift()
    assert pl.feedback_steps() == 1
    after1 = _items(pl)
    after1["ITERS"] = iters1
    _iterate_out(pl)
    open2 = _items(pl)
    pl.shift()
    after2 = _items(pl)
    assert pl.feedback_steps() == 2 and int(pl.get("T_STEP")[0]) == T0 + 2
    pl.close()
    return dict(x0=x0, ctrl=ctrl, after1=after1, open2=open2, after2=after2)


# ---------------------------------------------------------------------------------------------
# the kernel alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", C.KERNEL_SIZES)
def test_kernel_alone(batches, n):
    b, _ = batches
    st, con, par, w = C.kernel_cases(n)
    keep = [a.copy() for a in (st, con, par, w)]
    worst = 0.0
    for ww in (None, w):
        got = b.propagate(st, con, par, ww)
        want = obca.propagate(st, con, par, ww)
        assert got.shape == (n, 2, 5) and np.isfinite(got).all()
        dev = float(np.abs(got - want).max())
        worst = max(worst, dev)
        # the limits hold exactly, whatever libm does
        assert np.abs(got[..., 4] - (0.0 if ww is None else ww[..., 4])).max() <= obca.MAX_STEER + 1e-15
    print(f"k_plan_propagate vs obca.propagate, n = {n}: max |deviation| {worst:.3e} (bound {C.PROPAGATE_TOL:.3e})")
    assert worst <= C.PROPAGATE_TOL, (n, worst)
    for a, k in zip((st, con, par, w), keep):
        assert np.array_equal(a, k)
    # a second call gives the same bits, and one shared row is the n rows
    _bits(b.propagate(st, con, par, w), b.propagate(st, con, par, w), "repeat")
    _bits(b.propagate(st, con, par[0], w), b.propagate(st, con, np.tile(par[0], (n, 1)), w), "shared row")


def test_kernel_alone_saturation_is_exact(batches):
    b, _ = batches
    st = np.array([[[20.0, 0.0, 18.0, 0.0, 0.05]] * 2])
    got = b.propagate(st, np.array([[[9.0, 30.0], [-9.0, -30.0]]]), obca.feedback_row(n_sub=8))
    assert got[0, 0, 4] == obca.MAX_STEER and got[0, 1, 4] == -obca.MAX_STEER
    lim = b.propagate(st, np.array([[[5.0, 20.0], [-5.0, -20.0]]]), obca.feedback_row(n_sub=8))
    _bits(got, lim, "beyond the limits is at the limits")
    got = b.propagate(st, np.array([[[0.0, 7.0], [0.0, -7.0]]]), obca.feedback_row(gain_w=0.0))
    assert (got[..., 4] == 0.05).all()


def test_kernel_alone_refusals(batches):
    b, _ = batches
    st, con, par, w = C.kernel_cases(4)
    for field, value, _ in C.bad_rows():
        rows = par.copy()
        rows[2] = obca.feedback_row(**{field: (obca._FEEDBACK_DEFAULT[field], value)})
        _expect(-1, "obca_propagate: row 2: ", b.propagate, st, con, rows, w)
    for at in (0, 1, 3):
        args = [st.copy(), con.copy(), par, w.copy()]
        args[at][1, 1, 0] = np.nan
        _expect(-1, "not finite", b.propagate, *args)
    _expect(-1, "1 <= n", b.propagate, st[:0], con[:0], par[:0].reshape(0, 16))


# ---------------------------------------------------------------------------------------------
# in the plan
# ---------------------------------------------------------------------------------------------
def test_step_closes_through_the_plant(batches, plain, closed):
    b, _ = batches
    a1 = closed["after1"]
    want = b.propagate(closed["x0"], _u0(closed["ctrl"]), PAR, TAPE[:, 0])
    _bits(_init(a1["STATE"]), want, "init_state of STATE")
    _bits(_init(a1["STATE_PREV"]), want, "init_state of STATE_PREV")
    # the plant moved somewhere else than the prediction, and x0 is the step's init_state
    assert not np.array_equal(want, _init(plain["STATE"]))
    _bits(closed["x0"], np.stack([np.stack([obca.executed_path(v, T0 * obca.DT, F.SPECS[c]) for v in (0, 1)])
                                  for c in CASES]), "x0")
    # everything else the shift produces is the plan's without feedback
    for key in ("STATE", "STATE_PREV"):
        _bits(a1[key][:, :S_INIT], plain[key][:, :S_INIT], key)
    for key in ("LAMBDA", "CTRL_PREV", "ITERS", "X", "CTRL", "PRIMAL", "DUAL", "STATUS_MASK"):
        _bits(a1[key], plain[key], key)
    assert not a1["CTRL_PREV"].any()


def test_next_step_is_a_plain_plan_from_the_reached_state(batches, closed):
    _, ref = batches
    pp = obca.OBCADevicePlanner(ref, state=closed["after1"]["STATE"], **dict(_kw(), t_step0=T0 + 1))
    _iterate_out(pp)
    for key in ("ITERS", "X", "STATE", "PRIMAL", "DUAL", "STATUS_MASK", "CTRL"):
        _bits(closed["open2"][key], pp.get(key), f"{key} of step 2 before its shift")
    x0, ctrl = _init(pp.get("STATE")), pp.get("CTRL")
    pp.shift()
    a2 = closed["after2"]
    for key in ("STATE", "STATE_PREV"):
        _bits(a2[key][:, :S_INIT], pp.get(key)[:, :S_INIT], f"{key} after step 2")
    want = ref.propagate(x0, _u0(ctrl), PAR, TAPE[:, 1])
    _bits(_init(a2["STATE"]), want, "init_state after step 2: the second tape row")
    _bits(_init(a2["STATE_PREV"]), want, "init_state of STATE_PREV after step 2")
    pp.close()


def test_trace_records_the_reached_states(batches, closed):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR, tape=TAPE), **_kw())
    tr = pl.run_traced(2)
    assert tr.states.shape == (3, N, 2, 5)
    _bits(tr.states[1], _init(closed["after1"]["STATE"]), "STATES row 1")
    _bits(tr.states[2], _init(closed["after2"]["STATE"]), "STATES row 2")
    _bits(tr.states[2], _init(pl.get("STATE")), "STATES row 2 is the plan's init_state")
    _bits(np.stack(pl.init_state), tr.states[2], "the planner's init_state")
    for r in range(3):
        _bits(tr.clearance[r], b.clearance(tr.states[r], pl.prob), f"CLEARANCE row {r}")
    _bits(tr.min_clearance, tr.clearance[:, :, 0].min(axis=0), "min clearance")
    assert tr.min_row.tolist() == tr.clearance[:, :, 0].argmin(axis=0).tolist()
    _bits(tr.min_clearance_tight, tr.clearance[:, :, 1].min(axis=0), "min tight clearance")
    assert tr.iters_sum.tolist() == tr.iters.sum(axis=0).tolist()
    _bits(tr.iters[0], closed["after1"]["ITERS"], "ITERS row 0")
    assert pl.feedback_steps() == 2
    pl.close()


def test_order_on_top_changes_nothing(batches, closed):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=PAR, tape=TAPE), order=True, **_kw())
    pl.step()
    for key in ITEMS:
        _bits(pl.get(key), closed["after1"][key], f"{key} after step 1 with the order")
    pl.step()
    for key in ITEMS:
        _bits(pl.get(key), closed["after2"][key], f"{key} after step 2 with the order")
    pl.close()


def test_dual_law_integrators_are_the_plain_plans(batches):
    b, ref = batches
    gains = D.fleet_gains(CASES)
    pf = obca.OBCADevicePlanner(b, feedback=dict(par=PAR, tape=TAPE), dual=gains, **_kw())
    pp = obca.OBCADevicePlanner(ref, dual=gains, **_kw())
    pf.step()
    pp.step()
    for key in ("DUAL_S", "DUAL_D", "DUAL_S_PREV", "DUAL_D_PREV", "LAMBDA", "X"):
        _bits(pf.get(key), pp.get(key), key)
    _bits(pf.get("STATE")[:, :S_INIT], pp.get("STATE")[:, :S_INIT], "STATE but init_state")
    assert not np.array_equal(_init(pf.get("STATE")), _init(pp.get("STATE")))
    pf.close()
    pp.close()


def test_attach_then_detach_is_the_plain_plan(batches, plain):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, **_kw())
    _expect(-3, "no feedback attached", pl.get, "FEEDBACK_STEPS")
    _expect(-3, "no feedback attached", pl.get, "FEEDBACK_PAR")
    pl.set_feedback(par=PAR, tape=TAPE)
    pl.set_feedback()                                  # a second call replaces the first
    _bits(pl.get("FEEDBACK_PAR"), obca.feedback_row().reshape(1, 16), "the nominal row")
    pl.clear_feedback()
    _expect(-3, "no feedback attached", pl.get, "FEEDBACK_STEPS")
    pl.step()
    for key in ITEMS:
        _bits(pl.get(key), plain[key], key)
    _bits(np.stack(pl.init_state), _init(plain["STATE"]), "the planner's init_state")
    pl.close()


def test_tape_exhausted(batches):
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(tape=TAPE[:, :1]), **_kw())
    pl.step()
    assert pl.feedback_steps() == 1
    state = pl.get("STATE")
    _expect(-3, "obca_plan_step: disturbance tape exhausted", pl.step)
    assert pl.counts()[2] == 0                          # refused before any launch
    _iterate_out(pl)
    before = _items(pl)
    _expect(-3, "obca_plan_shift: disturbance tape exhausted", pl.shift)
    for key in ITEMS:
        _bits(pl.get(key), before[key], f"{key} after the refused shift")
    _bits(_init(pl.get("STATE")), _init(state), "init_state")
    assert pl.feedback_steps() == 1 and int(pl.get("T_STEP")[0]) == T0 + 1
    pl.close()
    # a traced run that does not fit the tape refuses with nothing run
    pl = obca.OBCADevicePlanner(b, feedback=dict(tape=TAPE[:, :1]), **_kw())
    state = pl.get("STATE")
    pl.trace_begin(2)
    _expect(-3, "obca_trace_run: disturbance tape exhausted before 2 steps \\(0 of 1 rows used\\)$", pl.trace_run, 2)
    assert pl.trace_rows() == 0 and pl.counts() == (0, N, 0) and pl.feedback_steps() == 0
    _bits(pl.get("STATE"), state, "STATE")
    assert pl.trace_run(1) == 1 and pl.feedback_steps() == 1
    pl.close()


def test_measure(batches):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, **_kw())
    pl.step()
    before = _items(pl)
    slots = np.array([0, 2], np.int32)
    meas = _init(before["STATE"])[slots] + np.array([0.05, -0.03, 0.1, 0.002, 0.001])
    # refusals leave the plan as it is
    _expect(-1, "slots\\[1\\]", pl.measure, [2, 0], meas)
    _expect(-1, "slots\\[1\\]", pl.measure, [2, 2], meas)
    _expect(-1, "slots\\[1\\]", pl.measure, [0, N], meas)
    _expect(-1, "slots\\[0\\]", pl.measure, [-1, 1], meas)
    bad = meas.copy()
    bad[1, 0, 3] = np.nan
    _expect(-1, "state pair 1 is not finite", pl.measure, slots, bad)
    for key in ITEMS:
        _bits(pl.get(key), before[key], f"{key} after the refused calls")
    pl.measure(slots, meas)
    want = {k: before[k].copy() for k in ("STATE", "STATE_PREV")}
    for key in want:
        want[key][slots, S_INIT:] = meas.reshape(2, 10)
        _bits(pl.get(key), want[key], key)
    for key in ITEMS[2:]:
        _bits(pl.get(key), before[key], f"{key}: nothing else moves")
    _bits(np.stack(pl.init_state)[slots], meas, "the planner's init_state")
    # the next step is a plain plan's opened from that state
    pp = obca.OBCADevicePlanner(ref, state=want["STATE"], **dict(_kw(), t_step0=T0 + 1))
    pl.step()
    pp.step()
    for key in ITEMS:
        _bits(pl.get(key), pp.get(key), f"{key} of the step after the measurement")
    pp.close()
    # mid-step and with a trace
    pl.iterate()
    _expect(-3, "only at a step boundary", pl.measure, slots, meas)
    pl.close()
    pl = obca.OBCADevicePlanner(b, **_kw())
    pl.trace_begin(1)
    _expect(-3, "a trace is attached", pl.measure, slots, meas)
    pl.trace_end()
    pl.measure(slots, meas)
    pl.close()


def test_refusals(batches, plain):
    b, ref = batches
    fb = dict(par=PAR, tape=TAPE)
    # clock and feedback do not go together, either way round
    pl = obca.OBCADevicePlanner(b, feedback=fb, **_kw())
    _expect(-3, "obca_clock_plan: feedback is attached", pl.set_clock)
    _expect(-3, "obca_tenant_export: feedback is attached", pl.export_tenants, [0])
    src = obca.OBCADevicePlanner(ref, **_kw())
    blob = src.export_tenants([1])
    src.close()
    _expect(-3, "obca_tenant_import: feedback is attached", pl.import_tenants, [0], blob)
    # a bad row: the earlier attachment and the plan stay
    rows = PAR.copy()
    rows[1, 9] = 0.0                                   # vehicle 1's n_sub
    _expect(-1, "obca_feedback_plan: row 1: ", pl.set_feedback, par=rows, tape=TAPE)
    tape = TAPE.copy()
    tape[2, 1, 0, 0] = np.inf
    _expect(-1, "the tape of scenario 2", pl.set_feedback, par=PAR, tape=tape)
    two = np.ascontiguousarray(PAR[:2])
    assert pl._lib.piadmm_obca_feedback_plan(b._h, 1, _lib.dptr(two), 2, None, 0) == _lib.E_ARG
    assert pl._lib.piadmm_obca_feedback_plan(b._h, 2, None, 0, None, 0) == _lib.E_ARG
    _bits(pl.get("FEEDBACK_PAR"), PAR, "FEEDBACK_PAR after the refused calls")
    assert pl.feedback_steps() == 0
    # mid-step
    pl.iterate()
    _expect(-3, "obca_feedback_plan: only at a step boundary", pl.set_feedback, par=PAR)
    _expect(-3, "obca_feedback_plan: only at a step boundary", pl.clear_feedback)
    pl.close()
    pl = obca.OBCADevicePlanner(b, clock=True, **_kw())
    _expect(-3, "obca_feedback_plan: a clock is attached", pl.set_feedback, par=PAR)
    # the refused plan is still usable, and without feedback the three calls behave as before
    pl.step()
    for key in ("STATE", "X", "ITERS", "LAMBDA"):
        _bits(pl.get(key), plain[key], f"{key} of the clocked plan after the refusal")
    assert len(pl.export_tenants([0])) > 0
    pl.close()


def test_host_loop_and_device_plan_describe_the_same_loop(batches):
    """tests/test_gpu_obca_plan.py compares the host loop with the device plan bit for bit on the first
    iterate's local records and outputs and prints the free-running deviation for information (the runs
    part in the last bits of A).  The same here, and in between what the feedback adds: each planner's
    step closes through the plant from its own init_state and first control -- the host's with
    obca.propagate bit for bit, the device's within the kernel's bound of it."""
    b, ref = batches
    kw = dict(F.single_kwargs(0, T0), feedback=dict(par=PAR[0], tape=TAPE[:1]))
    host_stages, dev_stages = [], []
    hp = obca.OBCAPlanner(ref, on_stage=lambda *a: host_stages.append(a), **kw)
    dp = obca.OBCADevicePlanner(b, on_stage=lambda *a: dev_stages.append(a), **kw)
    x0 = np.stack(hp.init_state)
    _bits(np.stack(dp.init_state), x0, "seeded init_state")
    hp.step()
    dp.step()
    h0 = [s for s in host_stages if s[0] == "local"][0]
    d0 = [s for s in dev_stages if s[0] == "local"][0]
    _bits(d0[1]["recs"], h0[1]["recs"], "first local records")
    _bits(d0[2]["result"].raw, h0[2]["result"].raw, "first local outputs")
    # the host's stopping solution: the last local stage
    hl = [s for s in host_stages if s[0] == "local"][-1][2]["result"]
    hu0 = np.stack([hl.U[v][0] for v in (0, 1)])[None]
    _bits(np.stack(hp.init_state), obca.propagate(x0, hu0, PAR[0], TAPE[:1, 0]), "the host loop's plant step")
    du0 = _u0(dp.get("CTRL"))
    dev = float(np.abs(np.stack(dp.init_state) - obca.propagate(x0, du0, PAR[0], TAPE[:1, 0])).max())
    assert dev <= C.PROPAGATE_TOL, dev
    _bits(np.stack(dp.init_state), _init(dp.get("STATE")), "the device planner's init_state")
    assert hp.feedback_steps() == dp.feedback_steps() == 1
    hp.step()
    dp.step()
    free = float(np.abs(np.asarray(dp.record.state_record) - np.asarray(hp.record.state_record)).max())
    print(f"free-running with feedback: max |state_record(device) - state_record(host)| after 2 steps {free:.3e}; "
          f"iterates host {np.asarray(hp.record.iter_num_record).tolist()} "
          f"device {np.asarray(dp.record.iter_num_record).tolist()}")
    # a measurement reaches both the same way
    meas = np.stack(hp.init_state) + 0.01
    hp.measure([0], meas)
    dp.measure([0], meas)
    _bits(np.stack(dp.init_state), np.stack(hp.init_state), "measured init_state")
    _bits(_init(dp.get("STATE")), meas, "measured STATE")
    dp.close()


def test_refusal_texts_in_full(batches):
    """piadmm_obca_feedback_plan's refusals of the row count and of a tape that is not finite, to their
    last word.  2 scenarios, no MPC step."""
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, **F.fleet_kwargs(CASES[:2], T0))
    rc = b._lib.piadmm_obca_feedback_plan(b._h, 1, _lib.dptr(PAR), 3, None, 0)
    assert rc == -1 and b._lib.piadmm_obca_last_error(b._h) == b"obca_feedback_plan: rows must be 1 or n (2)"
    bad = np.zeros((2, 2, 2, 5))
    bad[1, 1, 0, 3] = np.nan
    _expect(-1, "obca_feedback_plan: the tape of scenario 1 is not finite \\(step 1\\)$", pl.set_feedback, par=PAR[:2], tape=bad)
    _expect(-3, "obca_plan_get: no feedback attached", pl.get, "FEEDBACK_STEPS")
    pl.close()
