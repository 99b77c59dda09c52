"""The per-scenario clocks of the device-resident OBCA-ADMM plan (k_plan_clock and the list-taking
shifts in csrc/piadmm_obca_plan_attach.hip behind piadmm_obca_clock_plan / _clock_admit / _clock_tick;
OBCADevicePlanner(clock=...), set_clock, clear_clock, clock, admit; OBCABatch.clock_tick).

Bars.  Everything the clock adds is integers or copies, and a scenario's answers do not depend on
its place in a batch (tests/test_gpu_obca_order.py, bit for bit), so every comparison here is
bit-equality: scenario s of a clocked plan against that scenario alone in a plain plan opened at
t_step0 = c0[s]; a plan with clock_init = NULL against the same plan without a clock.

max_admm_iter <= 2 and n_ref = 51 throughout.  The yardsticks (each scenario alone, 3 MPC steps)
are computed once per (case, c0, law) on the second handle and never changed."""
import numpy as np
import pytest

import _obca_clock_cases as K
import _obca_dual_cases as C
import _obca_fleet_cases as F
import _obca_order_cases as R
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

SETUP, _bits = P.SETUP, P._bits
ITEMS = ("STATE", "STATE_PREV", "X", "CTRL", "ITERS", "PRIMAL", "DUAL", "STATUS_MASK", "LAMBDA")
FROZEN = ("STATE", "STATE_PREV", "X", "CTRL", "LAMBDA", "PRIMAL", "DUAL")
ALL_ITEMS = ITEMS + ("CTRL_PREV", "STOP", "CONVERGE", "T_STEP", "COUNTS", "REF", "PAR")
ITER_ITEMS = ("ACTIVE", "LOCAL_REC", "LOCAL_OUT", "LOCAL_IST", "EDGE_REC", "EDGE_OUT", "EDGE_IST")
CASES5 = [0, 1, 2, 3, 0]
N_REF = K.N_REF


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


def _gains(case):
    return {name: vals[case] for name, vals in C.FLEET_GAINS.items()}


_ALONE = {}


def alone(ref, case, c0, law=False, state=None, tag=None, gcase=None):
    """What a plain plan of case `case` alone, opened at t_step0 = c0 (on `state`, else seeded there;
    with the law, on the gains of case `gcase`, else its own), holds after each of 3 MPC steps: a
    list of {item: the scenario's row}."""
    gcase = case if gcase is None else gcase
    key = (case, c0, ("law", gcase) if law else None, tag)
    if key not in _ALONE:
        extra = dict(dual=_gains(gcase)) if law else {}
        if state is not None:
            extra["state"] = np.ascontiguousarray(state)[None]
        pl = obca.OBCADevicePlanner(ref, **F.single_kwargs(case, c0), **extra)
        assert pl.n_ref == N_REF
        steps = []
        for _ in range(3):
            pl.step()
            row = {k: pl.get(k)[0].copy() for k in ITEMS}
            if law:
                row.update({k: pl.get(k)[0].copy() for k in ("DUAL_S", "DUAL_D")})
            steps.append(row)
        pl.close()
        _ALONE[key] = steps
    return _ALONE[key]


def mixed(n, lens=None):
    """(cases, clock rows) of a fleet of n in mixed phases: case k % 4, c0 cycling over K.C0."""
    cases = [k % 4 for k in range(n)]
    c0 = [K.C0[k % 3] for k in range(n)]
    rows = np.array([[c, N_REF if lens is None else lens.get(k, N_REF)] for k, c in enumerate(c0)], np.int32)
    return cases, rows


def run_step(pl, mirror, check_rec=True):
    """One MPC step of a clocked plan iterate by iterate; the ticked mirror.  After the first iterate
    the ref field of every local record must be the scenario's own 8 reference rows."""
    first = True
    while first or pl.counts()[1]:
        pl.iterate()
        if first and check_rec:
            act, recs = pl.get("ACTIVE"), pl.get("LOCAL_REC")
            assert sorted(act.tolist()) == np.flatnonzero(mirror[:, 2]).tolist()
            for k, s in enumerate(act):
                c = mirror[s, 0]
                for v in (0, 1):
                    _bits(recs[2 * k + v, 5:45], pl.ref_traj_s[s][v][c:c + 8].reshape(-1), f"ref of scenario {s}")
        first = False
    pl.shift()
    mirror = obca.clock_tick(mirror, mirror[:, 2])
    assert pl.clock().tolist() == mirror.tolist()
    return mirror


def same_as_alone(pl, ref, s, case, c0, step, law=False, tag=None, state=None, keys=ITEMS, gcase=None):
    want = alone(ref, case, c0, law, state, tag, gcase)[step]
    for key in keys + (("DUAL_S", "DUAL_D") if law else ()):
        _bits(pl.get(key)[s], want[key], f"{key} of scenario {s} (case {case}, c0 {c0}) after its step {step + 1}")


# ---------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True])
@pytest.mark.parametrize("n", K.SIZES)
def test_kernel_alone(batches, n, shared):
    b, _ = batches
    clock, ran, ref = K.alone_case(n)
    ref = np.ascontiguousarray(ref[0]) if shared else ref
    clock_in, ran_in = clock.copy(), ran.copy()
    got, win, lst = b.clock_tick(clock, ran, ref)
    assert np.array_equal(clock, clock_in) and np.array_equal(ran, ran_in)
    want = obca.clock_tick(clock, ran)
    assert got.dtype == np.int32 and got.tolist() == want.tolist(), n
    assert got.tolist() == K.tick_by_hand(clock, ran).tolist()
    _bits(win, obca.clock_window(ref, want), "window")
    assert lst.dtype == np.int32 and lst.tolist() == np.flatnonzero(want[:, 2]).tolist()
    if n >= 64:
        assert 0 < len(lst) < n and (ran == 1).any() and (ran == 0).any()


# ---------------------------------------------------------------------------------------------
# 2. clock_init = NULL is the plan without a clock
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("plan", ["shared", "fleet"])
def test_null_clock_is_the_plain_plan(batches, plan):
    b, ref = batches
    kw = dict(SETUP, n_scenarios=3) if plan == "shared" else F.fleet_kwargs(CASES5, 12)
    pc = obca.OBCADevicePlanner(b, clock=True, **kw)
    pp = obca.OBCADevicePlanner(ref, **kw)
    assert pc.fleet == pp.fleet == (plan == "fleet")
    n = pc.n
    assert pc.clock().tolist() == [[12, N_REF, 1]] * n
    _bits(pc.get("WINDOW"), np.ascontiguousarray(pc.ref_traj_s[:, :, 12:20]), "WINDOW")

    def step(where):
        first = True
        while first or pc.counts()[1]:
            first = False
            assert pc.iterate() == pp.iterate()
            for key in ALL_ITEMS + ITER_ITEMS:
                _bits(pc.get(key), pp.get(key), f"{key} {where}")
        pc.shift()
        pp.shift()
        for key in ALL_ITEMS:
            _bits(pc.get(key), pp.get(key), f"{key} after the shift {where}")

    for k in range(2):
        step(f"of step {k}")
        assert pc.clock().tolist() == [[13 + k, N_REF, 1]] * n
    # detached, the plan goes on as the plain one: a bit-equal third step
    pc.clear_clock()
    assert pc.t_step == 14 and int(pc.get("T_STEP")[0]) == 14
    with pytest.raises(_lib.PiadmmError, match="no clock attached"):
        pc.get("CLOCK")
    step("of the step after detaching")
    pc.close()
    pp.close()


# ---------------------------------------------------------------------------------------------
# 3. mixed phases
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [5, 70])
def test_mixed_phases(batches, n):
    b, ref = batches
    cases, rows = mixed(n)
    pl = obca.OBCADevicePlanner(b, clock=rows, **F.fleet_kwargs(cases, 0))
    mirror = pl.clock()
    assert mirror.tolist() == [[c, N_REF, 1] for c in rows[:, 0]]
    _bits(pl.get("WINDOW"), obca.clock_window(pl.ref_traj_s, mirror), "WINDOW")
    for step in range(2):
        mirror = run_step(pl, mirror)
        _bits(pl.get("WINDOW"), obca.clock_window(pl.ref_traj_s, mirror), "WINDOW")
        for s in range(n):
            same_as_alone(pl, ref, s, cases[s], int(rows[s, 0]), step)
    assert int(pl.get("T_STEP")[0]) == 2 and mirror[:, 0].tolist() == (rows[:, 0] + 2).tolist()
    pl.close()


# ---------------------------------------------------------------------------------------------
# 4. retirement
# ---------------------------------------------------------------------------------------------
def test_retirement(batches):
    b, ref = batches
    n, short = 5, (1, 3)
    cases, rows = mixed(n)
    for s in short:
        rows[s, 1] = rows[s, 0] + 9                    # two steps: c0 and c0 + 1
    pl = obca.OBCADevicePlanner(b, clock=rows, **F.fleet_kwargs(cases, 0))
    mirror = pl.clock()
    for step in range(2):
        mirror = run_step(pl, mirror)
    assert mirror[:, 2].tolist() == [1, 0, 1, 0, 1]
    frozen = {key: pl.get(key) for key in FROZEN + ("WINDOW",)}
    for s in short:
        same_as_alone(pl, ref, s, cases[s], int(rows[s, 0]), 1)
    # the third step runs the others alone
    pl.iterate()
    assert pl.get("ACTIVE").tolist() == [0, 2, 4] and pl.counts()[0] == 3
    while pl.counts()[1]:
        pl.iterate()
    pl.shift()
    mirror = obca.clock_tick(mirror, mirror[:, 2])
    assert pl.clock().tolist() == mirror.tolist() and int(pl.get("T_STEP")[0]) == 3
    for s in short:
        for key in frozen:
            _bits(pl.get(key)[s], frozen[key][s], f"{key} of the retired scenario {s}")
        assert pl.get("ITERS")[s] == 0 and not pl.get("STATUS_MASK")[s].any()
    for s in (0, 2, 4):
        same_as_alone(pl, ref, s, cases[s], int(rows[s, 0]), 2)      # as in a run in which nobody retires
        assert pl.get("ITERS")[s] >= 1
    pl.close()
    # everyone retired: nothing runs
    cases, rows = mixed(3)
    rows[:, 1] = rows[:, 0] + 8
    pl = obca.OBCADevicePlanner(b, clock=rows, **F.fleet_kwargs(cases, 0))
    pl.run(5)                                          # stops cleanly after the one step there is
    assert pl.t_step == 1 and not pl.alive().any() and pl.clock()[:, 2].tolist() == [0, 0, 0]
    before = {key: pl.get(key) for key in ALL_ITEMS + ("CLOCK", "WINDOW")}
    lib = b._lib
    for call in (lambda: lib.piadmm_obca_plan_step(b._h, None), lambda: lib.piadmm_obca_plan_iterate(b._h, None)):
        assert call() == _lib.E_STATE
        assert b"no scenario alive" in lib.piadmm_obca_last_error(b._h)
    for key in before:
        _bits(pl.get(key), before[key], f"{key} after the refused step")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 5. with the dual law, the order and a trace attached together
# ---------------------------------------------------------------------------------------------
def test_with_law_order_and_trace(batches):
    b, ref = batches
    n, short = 5, 3
    cases, rows = mixed(n)
    rows[:, 1] = rows[:, 0] + 10                       # three steps each ...
    rows[short, 1] = rows[short, 0] + 9                # ... but one, which has two
    pl = obca.OBCADevicePlanner(b, clock=rows, dual=C.fleet_gains(cases), order=True,
                                work_init=R.reversing_work(n), **F.fleet_kwargs(cases, 0))
    assert pl.steps_left() == 3
    pl.trace_begin(8)
    with pytest.raises(_lib.PiadmmError, match="every reference ends before 4 steps") as ei:
        pl.trace_run(4)
    assert ei.value.code == _lib.E_STATE and pl.trace_rows() == 0
    pl.iterate()
    assert pl.get("ACTIVE").tolist() == [4, 3, 2, 1, 0]               # the seeded order, over the alive list
    while pl.counts()[1]:
        pl.iterate()
    pl.shift()
    assert pl.trace_run(2) == 2
    tr = pl.trace()
    mirror = pl.clock()
    assert mirror.tolist() == [[c + (2 if s == short else 3), ln, 0] for s, (c, ln) in enumerate(rows.tolist())]
    per_step = dict(iters="ITERS", status_mask="STATUS_MASK", primal="PRIMAL", dual="DUAL", lamb="LAMBDA")
    for s in range(n):
        steps = 2 if s == short else 3
        want = alone(ref, cases[s], int(rows[s, 0]), law=True)
        same_as_alone(pl, ref, s, cases[s], int(rows[s, 0]), steps - 1, law=True, keys=FROZEN)
        for r in range(steps):
            _bits(tr.states[r + 1, s], want[r]["STATE"][546:].reshape(2, 5), f"trace state {r + 1} of {s}")
            for field, key in per_step.items():
                _bits(getattr(tr, field)[r, s], want[r][key], f"trace {field} {r} of {s}")
        assert tr.iters_sum[s] == sum(int(want[r]["ITERS"]) for r in range(steps))
    # the retired scenario's row of the third step: frozen state and clearance, iterate 0, masks 0
    _bits(tr.states[3, short], tr.states[2, short], "frozen init_state")
    _bits(tr.clearance[3, short], tr.clearance[2, short], "frozen clearance")
    assert tr.iters[2, short] == 0 and not tr.status_mask[2, short].any()
    assert tr.min_row[short] <= 2 and tr.min_clearance[short] == tr.clearance[:3, short, 0].min()
    _bits(tr.min_row, np.array([int(np.argmin(tr.clearance[:, s, 0])) for s in range(n)]), "first row of the minimum")
    # nothing is alive now
    with pytest.raises(_lib.PiadmmError, match="no scenario alive"):
        pl.trace_run(1)
    assert pl.run_traced(2).iters.shape == (0, n)      # stops cleanly: an empty trace
    pl.close()


# ---------------------------------------------------------------------------------------------
# 6. admission
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["new", "new-law", "nulls"])
def test_admission(batches, variant):
    b, ref = batches
    law = variant == "new-law"
    n = 5
    cases, rows = mixed(n)
    rows[1, 1] = rows[1, 0] + 8                        # scenario 1 retires after the first step
    extra = dict(dual=C.fleet_gains(cases), order=True) if law else {}
    pl = obca.OBCADevicePlanner(b, clock=rows, **F.fleet_kwargs(cases, 0), **extra)
    mirror = run_step(pl, pl.clock())
    assert mirror[:, 2].tolist() == [1, 0, 1, 1, 1]
    slots, new_clock = [1, 2], np.array([[12, N_REF], [5, 20]], np.int32)     # a retired slot and a live one
    if variant == "nulls":
        tenants = [cases[1], cases[2]]
        states = pl.get("STATE")[slots]
        pl.admit(slots, new_clock)
        tags = [("kept", s) for s in slots]
    else:
        tenants = [3, 0]
        donor = obca.OBCADevicePlanner(ref, **F.fleet_kwargs(tenants, 0))     # the tenants' rows, as a fleet packs them
        par, pth, dth, prob = donor.par.copy(), donor.primal_thres.copy(), donor.dual_thres.copy(), list(donor.prob)
        donor.close()
        pl.admit(slots, new_clock, par=par, prob=prob, primal_thres=pth, dual_thres=dth,
                 specs=[F.SPECS[c] for c in tenants])
        states, tags = [None, None], [None, None]
        _bits(pl.get("PAR")[slots], par, "PAR")
    mirror[slots, :2] = new_clock
    mirror[slots, 2] = 1
    assert pl.clock().tolist() == mirror.tolist() and pl.alive().all()
    _bits(pl.get("WINDOW"), obca.clock_window(pl.ref_traj_s, mirror), "WINDOW")
    for key in ("CTRL", "CTRL_PREV", "X", "LAMBDA", "ITERS", "STATUS_MASK"):
        assert not pl.get(key)[slots].any(), key
    _bits(pl.get("STATE")[slots], pl.get("STATE_PREV")[slots], "both state copies")
    if law:
        _bits(pl.get("DUAL_S")[slots].reshape(2, -1), pl.get("STATE")[slots][:, 294:420], "S = lamb_bar of the new state")
        assert not pl.get("DUAL_D")[slots].any() and not pl.work()[slots].any()
    for step in range(2):
        mirror = run_step(pl, mirror)
        for k, s in enumerate(slots):
            # the gains rows are the slots': an admission leaves them
            same_as_alone(pl, ref, s, tenants[k], int(new_clock[k, 0]), step, law, tags[k], states[k], gcase=cases[s])
        for s in (0, 3, 4):                            # untouched: as in a run without the admission
            same_as_alone(pl, ref, s, cases[s], int(rows[s, 0]), step + 1, law)
    pl.close()


# ---------------------------------------------------------------------------------------------
# 7. refusals leave the plan as it was
# ---------------------------------------------------------------------------------------------
def test_refusals(batches):
    b, _ = batches
    lib = b._lib
    n = 5
    cases, rows = mixed(n)
    snap_keys = ALL_ITEMS + ("CLOCK", "WINDOW")

    def refused(pl, call, code, text, keys=snap_keys):
        before = {key: pl.get(key) for key in keys}
        assert call() == code, text
        assert text in lib.piadmm_obca_last_error(b._h), lib.piadmm_obca_last_error(b._h)
        for key in keys:
            _bits(pl.get(key), before[key], f"{key} after the refused call ({text})")

    ck = np.array([[5, N_REF]], np.int32)
    one = np.array([0], np.int32)
    admit = lambda slots, clock, ref=None: lib.piadmm_obca_clock_admit(       # noqa: E731
        b._h, len(slots), _lib.iptr(np.ascontiguousarray(slots, np.int32)), _lib.iptr(np.ascontiguousarray(clock, np.int32)),
        None, _lib.dptr(ref), None, None, None, None)
    # no plan; CLOCK and an admission without a clock
    assert lib.piadmm_obca_clock_plan(b._h, 1, None) == _lib.E_STATE
    assert b"no open plan" in lib.piadmm_obca_last_error(b._h)
    pl = obca.OBCADevicePlanner(b, **F.fleet_kwargs(cases, 5))
    probe = np.zeros((n, 3), np.int32)
    plain = ALL_ITEMS
    refused(pl, lambda: lib.piadmm_obca_plan_get(b._h, obca.PLAN_GET["CLOCK"][0], probe.ctypes.data, probe.nbytes),
            _lib.E_STATE, b"no clock attached", plain)
    refused(pl, lambda: admit(one, ck), _lib.E_STATE, b"no clock attached", plain)
    refused(pl, lambda: lib.piadmm_obca_clock_plan(b._h, 2, None), _lib.E_ARG, b"mode 0 (detach) or 1 (attach)", plain)
    # a bad row, each way (the row is named), attaches nothing
    for k, bad, why in ((2, [-1, N_REF], b"c0 >= 0"), (0, [5, 7], b"8 <= len <= n_ref"), (4, [5, N_REF + 1], b"8 <= len"),
                        (3, [44, N_REF], b"c0 + 8 <= len")):
        r = rows.copy()
        r[k] = bad
        refused(pl, lambda: lib.piadmm_obca_clock_plan(b._h, 1, _lib.iptr(r)), _lib.E_ARG,
                b"obca_clock_plan: row %d: " % k + why, plain)
    # mid-step: neither attaching nor detaching nor admitting
    pl.iterate()
    refused(pl, lambda: lib.piadmm_obca_clock_plan(b._h, 1, None), _lib.E_STATE, b"only at a step boundary", plain)
    while pl.counts()[1]:
        pl.iterate()
    pl.shift()
    pl.set_clock(rows)
    pl.iterate()
    for call in (lambda: lib.piadmm_obca_clock_plan(b._h, 0, None), lambda: lib.piadmm_obca_clock_plan(b._h, 1, None),
                 lambda: admit(one, ck)):
        refused(pl, call, _lib.E_STATE, b"only at a step boundary")
    while pl.counts()[1]:
        pl.iterate()
    pl.shift()
    # admission: a bad row, duplicate or out-of-range slots, with a trace attached
    refused(pl, lambda: admit([0, 1], [[5, N_REF], [44, N_REF]]), _lib.E_ARG, b"obca_clock_admit: row 1: c0 + 8 <= len")
    refused(pl, lambda: admit([1, 1], [[5, N_REF]] * 2), _lib.E_ARG, b"obca_clock_admit: slots[1]")
    refused(pl, lambda: admit([n], ck), _lib.E_ARG, b"obca_clock_admit: slots[0]")
    badpar = np.zeros((1, obca.FLEET_PAR))
    refused(pl, lambda: lib.piadmm_obca_clock_admit(b._h, 1, _lib.iptr(one), _lib.iptr(ck), None, None, _lib.dptr(badpar),
                                                    None, None, None), _lib.E_ARG, b"obca_clock_admit: row 0: bad parameters")
    pl.trace_begin(2)
    refused(pl, lambda: admit(one, ck), _lib.E_STATE, b"a trace is attached")
    pl.trace_end()
    # detaching with unequal clocks (rows cycles over three phases)
    refused(pl, lambda: lib.piadmm_obca_clock_plan(b._h, 0, None), _lib.E_STATE, b"detaching needs every scenario alive")
    with pytest.raises(_lib.PiadmmError, match="detaching needs") as ei:
        pl.clear_clock()
    assert ei.value.code == _lib.E_STATE and pl.clock()[:, 0].tolist() == (rows[:, 0] + 1).tolist()
    pl.close()
    # a reference for a plan that shares one
    ps = obca.OBCADevicePlanner(b, clock=True, **dict(SETUP, n_scenarios=3))
    assert not ps.fleet
    newref = np.zeros((1, 2, N_REF, 5))
    refused(ps, lambda: admit(one, ck, newref), _lib.E_STATE, b"ref needs a plan with a reference per scenario")
    # ... which still admits a tenant at another phase of the shared reference
    ps.admit([2], [[5, 30]])
    assert ps.clock().tolist() == [[12, N_REF, 1], [12, N_REF, 1], [5, 30, 1]]
    _bits(ps.get("WINDOW")[2], np.ascontiguousarray(ps.ref_traj_s[2][:, 5:13]), "the admitted window")
    ps.close()
    # the end of the plan frees the clock: a new plan has none
    again = obca.OBCADevicePlanner(b, **F.fleet_kwargs(cases, 5))
    assert lib.piadmm_obca_plan_get(b._h, obca.PLAN_GET["CLOCK"][0], probe.ctypes.data, probe.nbytes) == _lib.E_STATE
    again.close()


# ---------------------------------------------------------------------------------------------
# 8. Python: the host planner with clock= makes the same statement
# ---------------------------------------------------------------------------------------------
def test_host_planner_with_a_clock(batches):
    """Free-running, the host planner's halfspaces differ from the device's in the last bits
    (tests/test_gpu_obca_plan.py), so the two are compared where that cannot matter: the clocks,
    who ran, what is frozen, and the first step's records, which both pack from the same seeds."""
    b, ref = batches
    n = 4
    cases, rows = mixed(n)
    rows[2, 1] = rows[2, 0] + 8                        # one step
    seen = []
    host = obca.OBCAPlanner(ref, clock=rows, **F.fleet_kwargs(cases, 0),
                            on_stage=lambda name, i, o: seen.append((i["scenarios"], i["recs"])) if name == "local" and i["i_iter"] == 1 else None)
    dev = obca.OBCADevicePlanner(b, clock=rows, **F.fleet_kwargs(cases, 0))
    dev.iterate()
    host.run(3)
    assert seen[0][0] == dev.get("ACTIVE").tolist() == [0, 1, 2, 3]
    _bits(seen[0][1], dev.get("LOCAL_REC"), "the first local records")
    assert [sc for sc, _ in seen] == [[0, 1, 2, 3], [0, 1, 3], [0, 1, 3]]
    assert host.clock.tolist() == [[c + (1 if s == 2 else 3), ln, int(s != 2)] for s, (c, ln) in enumerate(rows.tolist())]
    it = np.asarray(host.record.iter_num_record)
    assert (it[0] >= 1).all() and it[1:, 2].tolist() == [0, 0] and (it[1:, [0, 1, 3]] >= 1).all()
    st, lam = np.asarray(host.record.state_record), np.asarray(host.record.lambda_record)
    _bits(st[2, 2], st[1, 2], "frozen init_state")
    _bits(st[3, 2], st[1, 2], "frozen init_state")
    _bits(lam[2, 2], lam[0, 2], "frozen lambda")
    dev.close()
