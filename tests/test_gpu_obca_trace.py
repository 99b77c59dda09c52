"""The device-side run record of an open plan (piadmm_obca_trace_*, k_plan_trace and
k_plan_clearance in csrc/piadmm_obca_plan_trace.hip; OBCADevicePlanner.run_traced).

What the trace copies (states, stop iterates, status masks, residuals, lamb_bar) is compared bit for
bit with a second handle that runs piadmm_obca_plan_step and downloads after every step: attaching a
trace changes nothing it records.  The clearances are teacher-forced: every CLEARANCE row against
piadmm.obca.clearance of that row's own STATES, at the 1e-12 bar of tests/test_gpu_obca_clearance.py;
zero / non-zero decisions and the argmin of SUMMARY are compared where the host stands at least
1e-9 from a tie, closer cases are counted and the count must be 0.

Two plans: the 3 scenarios of tests/test_gpu_obca_plan.py (prob [1, 0, 1], MPC step 12,
max_admm_iter 2) and the four-row fleet of tests/_obca_fleet_cases.py from the same step; 3 MPC
steps each."""
import ctypes

import numpy as np
import pytest

import _obca_fleet_cases as F
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

BAR, MARGIN, STEPS = 1e-12, 1e-9, 3
SETUP = dict(n_scenarios=3, prob=[1, 0, 1], t_step0=12, max_admm_iter=2, round_decimals=-1,
             primal_thres=[0.01, 0.01, np.inf], dual_thres=[0.01, 0.01, np.inf])
PLANS = {"shared": SETUP, "fleet": F.fleet_kwargs([0, 1, 2, 3], 12)}
ITEMS = ("STATES", "CLEARANCE", "ITERS", "STATUS_MASK", "PRIMAL", "DUAL", "LAMBDA", "SUMMARY")


@pytest.fixture(scope="module")
def batches():
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    a, b = obca.OBCABatch(0), obca.OBCABatch(0)
    yield a, b
    a.close()
    b.close()


def _bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (msg, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), msg


def _init(state):
    return state[:, obca.PLAN_STATE - 10:].reshape(-1, 2, obca.NX)


@pytest.fixture(scope="module")
def runs(batches):
    """Per plan: (the trace of piadmm_obca_trace_run(3) on handle A and its final states, the same
    steps by piadmm_obca_plan_step on handle B with downloads after each).  Computed once."""
    a, b = batches
    out = {}
    for name, kw in PLANS.items():
        pa = obca.OBCADevicePlanner(a, **kw)
        pa.trace_begin(STEPS, keep_lambda=True)
        assert pa.trace_rows() == 0
        assert pa.trace_run(STEPS) == STEPS
        tr = {k: pa.trace_get(k) for k in ITEMS}
        tr.update(ROWS=pa.trace_rows(), STATE=pa.get("STATE"), STATE_PREV=pa.get("STATE_PREV"),
                  T_STEP=int(pa.get("T_STEP")[0]), prob=list(pa.prob))
        pa.close()
        pb = obca.OBCADevicePlanner(b, **kw)
        st = dict(STATES=[_init(pb.get("STATE"))], ITERS=[], STATUS_MASK=[], PRIMAL=[], DUAL=[], LAMBDA=[])
        for _ in range(STEPS):
            iters = np.zeros(pb.n, np.int32)
            pb._check(pb._lib.piadmm_obca_plan_step(b._h, _lib.iptr(iters)))
            st["STATES"].append(_init(pb.get("STATE")))
            st["ITERS"].append(iters)
            _bits(pb.get("ITERS"), iters)
            for k in ("STATUS_MASK", "PRIMAL", "DUAL", "LAMBDA"):
                st[k].append(pb.get(k))
        st = {k: np.stack(v) for k, v in st.items()}
        st.update(STATE=pb.get("STATE"), STATE_PREV=pb.get("STATE_PREV"), T_STEP=int(pb.get("T_STEP")[0]))
        pb.close()
        out[name] = (tr, st)
    return out


@pytest.mark.parametrize("name", list(PLANS))
def test_trace_run_equals_stepping(runs, name):
    tr, st = runs[name]
    n = PLANS[name]["n_scenarios"]
    assert tr["ROWS"] == STEPS and tr["T_STEP"] == st["T_STEP"] == 12 + STEPS
    assert tr["STATES"].shape == (STEPS + 1, n, 2, 5) and tr["CLEARANCE"].shape == (STEPS + 1, n, 2)
    assert tr["LAMBDA"].shape == (STEPS, n, 2, obca.NT, 9)
    for k in ("STATES", "ITERS", "STATUS_MASK", "LAMBDA", "PRIMAL", "DUAL", "STATE", "STATE_PREV"):
        _bits(tr[k], st[k], k)
    assert np.all(tr["ITERS"] >= 1) and np.all(tr["STATUS_MASK"] >= 1)
    if name == "shared":                      # the scenarios stop at different iterates
        assert np.all(tr["ITERS"][:2, 2] == 1) and np.all(tr["ITERS"][:2, :2] >= 2)
    else:
        assert tr["ITERS"][0].tolist() == [F.STOP_ITERS[c] for c in range(4)]


@pytest.mark.parametrize("name", list(PLANS))
def test_clearance_and_summary_teacher_forced(runs, name):
    tr, _ = runs[name]
    states, clr, prob = tr["STATES"], tr["CLEARANCE"], tr["prob"]
    R1, n = clr.shape[:2]
    worst, near = 0.0, 0
    for r in range(R1):
        for s in range(n):
            want = obca.clearance(states[r, s], prob[s])
            for q, tight in enumerate((False, True)):
                gap = obca.box_clearance(obca.vehicle_box(states[r, s, 0], prob[s], tight),
                                         obca.vehicle_box(states[r, s, 1], prob[s], tight))[1]
                if abs(gap) < MARGIN:
                    near += 1
                    continue
                assert (clr[r, s, q] == 0.0) == (want[q] == 0.0), (r, s, q, clr[r, s, q], want[q])
                worst = max(worst, abs(clr[r, s, q] - want[q]))
            if not prob[s]:
                assert clr[r, s, 0] == clr[r, s, 1]
    print(f"trace clearance ({name}): max |device - host| {worst:.3e} over {R1 * n} state pairs; "
          f"min plain {clr[:, :, 0].min(axis=0)}")
    assert near == 0 and worst <= BAR, (near, worst)
    # SUMMARY against the minimum and the argmin over the device's own rows
    summ = tr["SUMMARY"]
    ties = 0
    for s in range(n):
        col = clr[:, s, 0]
        assert summ[s, 0] == col.min() and summ[s, 2] == clr[:, s, 1].min()
        two = np.sort(col)[:2]
        if two[1] - two[0] < MARGIN:
            ties += 1
        else:
            assert int(summ[s, 1]) == int(np.argmin(col)), (s, summ[s], col)
        assert summ[s, 1] == np.floor(summ[s, 1]) and 0 <= summ[s, 1] <= STEPS
        assert col[int(summ[s, 1])] == summ[s, 0]
        assert summ[s, 3] == tr["ITERS"][:, s].sum()
    assert ties == 0


def test_a_trace_stepped_by_hand(batches, runs):
    _, b = batches
    tr, _ = runs["shared"]
    pl = obca.OBCADevicePlanner(b, **SETUP)
    pl.trace_begin(STEPS, keep_lambda=True)
    _bits(pl.trace_get("STATES"), tr["STATES"][:1], "row 0")
    _bits(pl.trace_get("CLEARANCE"), tr["CLEARANCE"][:1], "row 0")
    for k in range(STEPS):
        while pl.iterate():
            pass
        assert pl.trace_rows() == k                    # the iterates record nothing
        pl.shift()
        assert pl.trace_rows() == k + 1
    for k in ITEMS:
        _bits(pl.trace_get(k), tr[k], k)
    _bits(pl.get("STATE"), tr["STATE"], "STATE")
    pl.close()


def test_error_paths(batches):
    a, _ = batches
    lib, h = a._lib, a._h
    rows = ctypes.c_int32(-1)

    def get_rows():
        assert lib.piadmm_obca_trace_get(h, obca.TRACE_GET["ROWS"][0], ctypes.byref(rows), 4) == 0
        return rows.value

    pl = obca.OBCADevicePlanner(a, **SETUP)
    # no trace yet
    assert lib.piadmm_obca_trace_run(h, 1, None) == _lib.E_STATE
    assert lib.piadmm_obca_trace_get(h, obca.TRACE_GET["ROWS"][0], ctypes.byref(rows), 4) == _lib.E_STATE
    assert lib.piadmm_obca_trace_end(h) == 0
    # bad arguments
    assert lib.piadmm_obca_trace_begin(h, 0, 0) == _lib.E_ARG
    assert lib.piadmm_obca_trace_begin(h, 2, 2) == _lib.E_ARG
    # without the flag the trace keeps no lamb_bar; a wrong size is refused
    pl.trace_begin(1, keep_lambda=False)
    buf = np.zeros(3 * 126)
    assert lib.piadmm_obca_trace_get(h, obca.TRACE_GET["LAMBDA"][0], buf.ctypes.data, 0) == _lib.E_STATE
    assert lib.piadmm_obca_trace_get(h, obca.TRACE_GET["STATES"][0], buf.ctypes.data, 8) == _lib.E_ARG
    assert lib.piadmm_obca_trace_get(h, 99, buf.ctypes.data, 8) == _lib.E_ARG
    # beyond the capacity: nothing runs
    done = ctypes.c_int32(-1)
    assert lib.piadmm_obca_trace_run(h, 2, ctypes.byref(done)) == _lib.E_STATE and done.value == 0
    assert pl.counts() == (0, 3, 0) and int(pl.get("T_STEP")[0]) == 12 and get_rows() == 0
    assert lib.piadmm_obca_trace_run(h, 0, None) == _lib.E_ARG
    # mid-step: no trace_begin
    pl.iterate()
    assert lib.piadmm_obca_trace_begin(h, 4, 0) == _lib.E_STATE
    assert b"step boundary" in lib.piadmm_obca_last_error(h)
    while pl.iterate():
        pass
    pl.shift()
    assert get_rows() == 1
    # the trace is full: the shift is refused before any launch and the plan stays as it was
    while pl.iterate():
        pass
    before, counts = pl.get("STATE"), pl.counts()
    assert lib.piadmm_obca_plan_shift(h) == _lib.E_STATE
    assert b"trace full" in lib.piadmm_obca_last_error(h)
    _bits(pl.get("STATE"), before, "STATE")
    assert int(pl.get("T_STEP")[0]) == 13 and get_rows() == 1 and pl.counts() == counts
    assert lib.piadmm_obca_plan_step(h, None) == _lib.E_STATE and pl.counts() == counts
    assert lib.piadmm_obca_last_error(h) == b"obca_plan_step: trace full"
    # the trace freed alone: the plan goes on
    assert lib.piadmm_obca_trace_end(h) == 0
    pl.shift()
    assert int(pl.get("T_STEP")[0]) == 14
    # beyond the reference: nothing runs (t_step 14, n_ref 51: 30 steps fit, 31 do not)
    pl.trace_begin(40, keep_lambda=False)
    assert lib.piadmm_obca_trace_run(h, 31, ctypes.byref(done)) == _lib.E_STATE and done.value == 0
    assert b"reference" in lib.piadmm_obca_last_error(h)
    assert pl.counts() == (0, 3, 0) and int(pl.get("T_STEP")[0]) == 14 and get_rows() == 0
    # a second trace_begin replaces the first
    pl.trace_begin(2, keep_lambda=True)
    assert pl.trace_run(1) == 1 and pl.trace_get("LAMBDA").shape == (1, 3, 2, obca.NT, 9)
    # plan_end frees the trace with the plan
    assert lib.piadmm_obca_plan_end(h) == 0
    assert lib.piadmm_obca_trace_get(h, obca.TRACE_GET["ROWS"][0], ctypes.byref(rows), 4) == _lib.E_STATE
    assert lib.piadmm_obca_trace_begin(h, 2, 0) == _lib.E_STATE
    assert lib.piadmm_obca_trace_end(h) == 0


@pytest.mark.parametrize("name", list(PLANS))
def test_run_traced_fills_the_record_of_run(batches, runs, name):
    a, b = batches
    p1, p2 = obca.OBCADevicePlanner(a, **PLANS[name]), obca.OBCADevicePlanner(b, **PLANS[name])
    tr = p1.run_traced(STEPS)
    rec = p2.run(STEPS)
    assert p1.t_step == p2.t_step == 12 + STEPS
    _bits(np.stack(p1.init_state), np.stack(p2.init_state), "init_state")
    for key in ("state_record", "iter_num_record", "lambda_record"):
        got, want = getattr(p1.record, key), getattr(rec, key)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            _bits(g, w, key)
    assert len(p1.record.status_record) == len(rec.status_record) == STEPS
    for g, w in zip(p1.record.status_record, rec.status_record):
        assert set(g) == set(w) and g["t_step"] == w["t_step"]
        for k in ("iters", "local_status_mask", "edge_status_mask"):
            _bits(g[k], w[k], k)
    # the returned trace is the one piadmm_obca_trace_run recorded
    ref = runs[name][0]
    for k, v in (("STATES", tr.states), ("CLEARANCE", tr.clearance), ("ITERS", tr.iters),
                 ("STATUS_MASK", tr.status_mask), ("PRIMAL", tr.primal), ("DUAL", tr.dual), ("LAMBDA", tr.lamb)):
        _bits(v, ref[k], k)
    _bits(tr.min_clearance, ref["SUMMARY"][:, 0])
    _bits(tr.min_clearance_tight, ref["SUMMARY"][:, 2])
    assert tr.min_row.tolist() == ref["SUMMARY"][:, 1].astype(int).tolist()
    # the plan goes on without a trace; staged stepping stays on run
    p1.step()
    assert lib_rows_state(p1) == _lib.E_STATE
    p1.close()
    p2.close()
    staged = obca.OBCADevicePlanner(a, on_stage=lambda *x: None, **PLANS[name])
    with pytest.raises(ValueError, match="run_traced"):
        staged.run_traced(1)
    staged.close()


def lib_rows_state(pl):
    r = ctypes.c_int32()
    return pl._lib.piadmm_obca_trace_get(pl.batch._h, obca.TRACE_GET["ROWS"][0], ctypes.byref(r), 4)
