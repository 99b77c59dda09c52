"""The tenant ledger of the device OBCA plan (k_ledger_open, k_ledger_step, k_ledger_close and
k_ledger_view in csrc/piadmm_obca_plan_ledger.hip behind piadmm_obca_ledger_begin / _get / _clear / _stats /
_end; OBCADevicePlanner.ledger_begin, ledger_records, ledger_running, ledger_clear, ledger_stats,
ledger_end, and admit / import_tenants under a ledger).

Bars.  Every comparison is bit equality between two device results: a tenant's record against the trace
of a one-scenario clocked plan of the same tenant (same state, reference, row, seed, stream, k0) over
the R = len - 8 - c0 + 1 steps it lives, a plan with a ledger against the same sequence without one.
The statistics are compared with piadmm.obca.ledger_stats_host on the downloaded records: counts, minima
and comparisons, exact.

max_admm_iter <= 2 (the cases of tests/_obca_fleet_cases.py), at most 3 MPC steps.  The lone traced
runs are computed once per tenant and never changed."""
import numpy as np
import pytest

import _obca_fleet_cases as F
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

_bits = P._bits
N_REF = 51
ITEMS = ("STATE", "STATE_PREV", "X", "CTRL", "LAMBDA", "ITERS", "STATUS_MASK", "CLOCK")
C0, RUNS = (0, 2, 1), (2, 1, 3)                     # three tenants that retire at three different shifts
LEN = tuple(c + 8 + r - 1 for c, r in zip(C0, RUNS))
PLANT = np.stack([obca.feedback_row(method=s % 2, n_sub=1 + s % 3, gain_a=1.0 - 0.02 * s, lr=(1.0, 1.0 + 0.02 * s))
                  for s in range(4)])
NOISE = np.stack([obca.noise_row(sigma=0.004 * (s + 1), bias=0.0005 * s, trunc=0.0 if s % 2 else 1.5) for s in range(4)])
DELAY = np.stack([obca.delay_row(avg=(0.03, 0.02 + 0.01 * s), std=0.04, tau_max=(0.1, 0.08), trunc=1.5) for s in range(4)])
STREAMS = np.array([5, 2 ** 32 + 1, 2 ** 63 - 1, 9], np.int64)
SEED, K0 = 2 ** 63 + 12345, 7


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


def _kw(cases, **extra):
    return dict(F.fleet_kwargs(list(cases), 0), **extra)


def _clock(c0, length):
    return np.array(list(zip(c0, length)), np.int32)


def _loop(rows):
    rows = list(rows)
    return dict(plant=PLANT[rows], noise=NOISE[rows], delay=DELAY[rows], streams=STREAMS[rows], seed=SEED, k0=K0)


def _expect(code, what, call, *a, **k):
    with pytest.raises(_lib.PiadmmError, match=what) as e:
        call(*a, **k)
    assert f"error {code}:" in str(e.value), str(e.value)


def _items(pl, names=ITEMS):
    return {k: pl.get(k).copy() for k in names}


_LONE = {}


def _lone(ref, case, c0, steps, loop=None, length=N_REF):
    """The trace of a one-scenario clocked plan of this tenant over `steps` steps from clock c0.  loop:
    (plant, noise, delay, stream) or None."""
    key = (case, c0, steps, length, None if loop is None else tuple(np.asarray(x).tobytes() for x in loop))
    if key not in _LONE:
        more = {} if loop is None else dict(loop=dict(plant=loop[0], noise=loop[1], delay=loop[2],
                                                      streams=[int(loop[3])], seed=SEED, k0=K0))
        pl = obca.OBCADevicePlanner(ref, clock=_clock([c0], [length]), **more, **_kw([case]))
        _LONE[key] = pl.run_traced(steps, keep_lambda=False)
        pl.close()
    assert _LONE[key].iters.shape[0] == steps
    return _LONE[key]


def _against_trace(rec, tr, what):
    """One record (appended or open) against the lone trace of the steps it has closed."""
    R = int(rec["steps"])
    assert R == tr.iters.shape[0], (what, R, tr.iters.shape)
    _bits(rec["min_clearance"], tr.min_clearance[0], f"{what}: the plain minimum")
    _bits(rec["min_clearance_tight"], tr.min_clearance_tight[0], f"{what}: the tightened minimum")
    assert int(rec["c_min"]) - int(rec["c_first"]) == int(tr.min_row[0]), what
    assert int(rec["iter_sum"]) == int(tr.iters_sum[0]) == int(tr.iters[:, 0].sum()), what
    assert int(rec["iter_max"]) == int(tr.iters[:, 0].max()), what
    assert int(rec["local_status_mask"]) == int(np.bitwise_or.reduce(tr.status_mask[:, 0, 0])), what
    assert int(rec["edge_status_mask"]) == int(np.bitwise_or.reduce(tr.status_mask[:, 0, 1])), what
    _bits(rec["primal"], tr.primal[R - 1, 0], f"{what}: the primal residual")
    _bits(rec["dual"], tr.dual[R - 1, 0], f"{what}: the dual residual")
    _bits(rec["state"], tr.states[R, 0], f"{what}: the last state")
    # the minima are those of the trace's own clearances
    _bits(rec["min_clearance"], tr.clearance[:, 0, 0].min(), f"{what}: the minimum of the rows")


# ---------------------------------------------------------------------------------------------
# 1. retiring: every record is the tenant's lone traced run
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("loop", (False, True))
def test_retirees_equal_their_lone_traced_runs(batches, loop):
    b, ref = batches
    more = dict(loop=_loop(range(3))) if loop else {}
    pl = obca.OBCADevicePlanner(b, clock=_clock(C0, LEN), **more, **_kw([0, 1, 2]))
    pl.ledger_begin(8)
    run = pl.ledger_running()
    assert run["id"].tolist() == [0, 1, 2] and run["slot"].tolist() == [0, 1, 2] and run["c_first"].tolist() == list(C0)
    assert run["reason"].tolist() == [0] * 3 and run["t_step"].tolist() == [-1] * 3 and not run["steps"].any()
    assert run["stream"].tolist() == ([int(v) for v in STREAMS[:3]] if loop else [-1] * 3)
    _bits(run["state"], pl.get("STATE")[:, 546:].reshape(3, 2, 5), "the entry states")
    _bits(np.stack((run["min_clearance"], run["min_clearance_tight"]), axis=1),
          b.clearance(run["state"], np.asarray(pl.prob, np.int32)), "the entry clearances")
    assert pl.ledger_count() == 0 and pl.ledger_next_id() == 3 and len(pl.ledger_records()) == 0
    order = (1, 0, 2)                               # the slot that retires at shift 1, 2, 3
    for step in range(3):
        pl.step()
        assert pl.ledger_count() == step + 1
    assert not pl.alive().any()
    rec = pl.ledger_records()
    assert rec["id"].tolist() == list(order) and rec["slot"].tolist() == list(order) and rec["reason"].tolist() == [1] * 3
    assert rec["t_step"].tolist() == [0, 1, 2] and rec["steps"].tolist() == [RUNS[s] for s in order]
    assert rec["c_first"].tolist() == [C0[s] for s in order] and not rec["reserved"].any()
    assert rec["stream"].tolist() == ([int(STREAMS[s]) for s in order] if loop else [-1] * 3)
    for k, s in enumerate(order):
        tr = _lone(ref, s, C0[s], RUNS[s], (PLANT[s], NOISE[s], DELAY[s], STREAMS[s]) if loop else None, LEN[s])
        _against_trace(rec[k], tr, f"scenario {s}")
    assert pl.ledger_running()["id"].tolist() == [-1] * 3 and pl.ledger_next_id() == 3
    pl.close()


# ---------------------------------------------------------------------------------------------
# 2. positions across a workgroup boundary; the statistics; clear
# ---------------------------------------------------------------------------------------------
def test_positions_statistics_and_clear_at_130_slots(batches):
    b, ref = batches
    n = 130                                           # slot 128 and 129: past a 128-scenario group and a PW workgroup
    cases = [s % 4 for s in range(n)]
    length = [8 + s % 2 for s in range(n)]            # the even slots retire at the first shift, the odd at the second
    pl = obca.OBCADevicePlanner(b, clock=_clock([0] * n, length), **_kw(cases))
    pl.ledger_begin(n)
    pl.step()
    even, odd = list(range(0, n, 2)), list(range(1, n, 2))
    assert pl.ledger_count() == 65 == int((~pl.alive()).sum())
    rec = pl.ledger_records()
    assert rec["slot"].tolist() == even and rec["id"].tolist() == even and rec["reason"].tolist() == [1] * 65
    assert rec["steps"].tolist() == [1] * 65 and rec["t_step"].tolist() == [0] * 65
    run = pl.ledger_running()
    assert run["reason"].tolist() == [0] * n and run["id"].tolist() == [-1 if s % 2 == 0 else s for s in range(n)]
    assert run["steps"][odd].tolist() == [1] * 65
    # the statistics of the appended records, on the device in place, against NumPy on the download
    x = np.sort(rec["min_clearance"])
    edges = [float(x[10]), float(x[40]) + 1e-9, float(x[-1]) + 1.0]
    st, want = pl.ledger_stats(edges, worst=4), obca.ledger_stats_host(rec, edges, K=4)
    for name in ("hist", "nonfinite", "fleet_min", "fleet_arg", "mask_or", "worst"):
        _bits(getattr(st, name), getattr(want, name), name)
    assert (st.iter_sum, st.iter_max, st.flagged) == (want.iter_sum, want.iter_max, want.flagged)
    assert st.hist.sum() == 130 and st.iter_sum == int(rec["iter_sum"].sum()) > 0 and len(set(st.worst.tolist())) == 4
    # clear: the count starts again, the ids go on
    pl.ledger_clear()
    assert pl.ledger_count() == 0 and len(pl.ledger_records()) == 0 and pl.ledger_next_id() == n
    _expect(-3, "obca_ledger_stats: the ledger holds no record", pl.ledger_stats, edges, 1)
    pl.step()
    assert pl.ledger_count() == 65 and not pl.alive().any()
    rec2 = pl.ledger_records()
    assert rec2["slot"].tolist() == odd and rec2["id"].tolist() == odd and rec2["steps"].tolist() == [2] * 65
    assert rec2["t_step"].tolist() == [1] * 65
    run = pl.ledger_running()
    assert run["reason"].tolist() == [0] * n and run["id"].tolist() == [-1] * n
    # the same tenant in another slot has the same record; the first four against their lone traces
    skip = ("id", "slot")
    for recs, slots in ((rec, even), (rec2, odd)):
        for k, s in enumerate(slots):
            first = k % 2                             # the cases alternate along either list
            for name in recs.dtype.names:
                if name not in skip:
                    _bits(recs[k][name], recs[first][name], f"slot {s} against slot {slots[first]}: {name}")
    for s in range(4):
        tr = _lone(ref, s, 0, 1 + s % 2, None, 8 + s % 2)
        _against_trace((rec2 if s % 2 else rec)[s // 2], tr, f"slot {s}")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 3. admission under the loop
# ---------------------------------------------------------------------------------------------
def _admission(pl, ledger):
    """Three tenants, one step (slot 1 retires), then case 2 into the retired slot 1 and case 0 over the
    alive slot 0, under loop rows 3 and 0 and new stream ids.  The open record of slot 0 before that."""
    if ledger:
        pl.ledger_begin(8)
    pl.step()
    assert pl.alive().tolist() == [True, False, True]
    before = pl.ledger_running()[0] if ledger else None
    rows = [3, 0]
    pl.admit([1, 0], _clock([4, 1], [N_REF, 10]), specs=[F.SPECS[2], F.SPECS[0]], par=pl.get("PAR")[[2, 0]].copy(),
             prob=[F.ROWS["prob"][2], F.ROWS["prob"][0]], primal_thres=np.array([0.01, 0.01]),
             dual_thres=np.array([0.01, 0.01]),
             loop=dict(plant=PLANT[rows], noise=NOISE[rows], delay=DELAY[rows], streams=[2 ** 50 + 1, 77]))
    return before


def test_admission_over_an_alive_and_a_retired_slot(batches):
    b, ref = batches
    clock = _clock(C0, (N_REF, 10, N_REF))
    twin = obca.OBCADevicePlanner(ref, clock=clock, loop=_loop(range(3)), **_kw([0, 1, 2]))
    _admission(twin, False)
    twin.step()
    twin.step()
    want = _items(twin)
    want_tau = twin.loop_tau()
    twin.close()
    pl = obca.OBCADevicePlanner(b, clock=clock, loop=_loop(range(3)), **_kw([0, 1, 2]))
    before = _admission(pl, True)
    assert before["id"] == 0 and before["steps"] == 1
    rec = pl.ledger_records()
    # slot 1 retired at the first shift; slot 0's tenant was replaced: reason 2, its step so far, its old stream
    assert rec["id"].tolist() == [1, 0] and rec["reason"].tolist() == [1, 2] and rec["steps"].tolist() == [1, 1]
    assert rec["t_step"].tolist() == [0, 1] and rec["stream"].tolist() == [int(STREAMS[1]), int(STREAMS[0])]
    for name in rec.dtype.names:
        if name not in ("reason", "t_step"):
            _bits(rec[1][name], before[name], f"the replaced tenant's record: {name}")
    run = pl.ledger_running()
    assert run["id"].tolist() == [4, 3, 2] and run["c_first"].tolist() == [1, 4, 1] and run["steps"].tolist() == [0, 0, 1]
    assert run["stream"].tolist() == [77, 2 ** 50 + 1, int(STREAMS[2])] and pl.ledger_next_id() == 5
    # clear, then further retirements: the count starts again, the ids go on
    pl.ledger_clear()
    pl.step()
    pl.step()
    got = _items(pl)
    for k in ITEMS:
        _bits(got[k], want[k], f"{k} against the same sequence without a ledger")
    _bits(pl.loop_tau(), want_tau, "the latencies against the same sequence without a ledger")
    assert pl.ledger_count() == 1 and pl.ledger_next_id() == 5
    rec = pl.ledger_records()
    assert (rec["id"][0], rec["slot"][0], rec["reason"][0], rec["t_step"][0], rec["stream"][0]) == (4, 0, 1, 2, 77)
    _against_trace(rec[0], _lone(ref, 0, 1, 2, (PLANT[0], NOISE[0], DELAY[0], 77), 10), "the admitted tenant that retired")
    run = pl.ledger_running()
    assert run["id"].tolist() == [-1, 3, 2] and run["steps"].tolist()[1:] == [2, 3]
    _against_trace(run[1], _lone(ref, 2, 4, 2, (PLANT[3], NOISE[3], DELAY[3], 2 ** 50 + 1)), "the admitted tenant that runs")
    _against_trace(run[2], _lone(ref, 2, 1, 3, (PLANT[2], NOISE[2], DELAY[2], STREAMS[2])), "the tenant that was never touched")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 4. import under the ledger
# ---------------------------------------------------------------------------------------------
def test_import_replaces_with_reason_3_and_opens_a_fresh_record(batches):
    b, ref = batches
    pl = obca.OBCADevicePlanner(b, clock=_clock(C0, (N_REF,) * 3), loop=_loop(range(3)), **_kw([0, 1, 2]))
    pl.ledger_begin(4)
    pl.step()
    before = pl.ledger_running()
    blob = pl.export_tenants([0])
    pl.import_tenants([2], blob)
    rec = pl.ledger_records()
    assert len(rec) == 1 and (rec["id"][0], rec["slot"][0], rec["reason"][0], rec["steps"][0], rec["t_step"][0]) == (2, 2, 3, 1, 1)
    assert rec["stream"][0] == STREAMS[2]
    for name in rec.dtype.names:
        if name not in ("reason", "t_step"):
            _bits(rec[0][name], before[2][name], f"the replaced tenant's record: {name}")
    run = pl.ledger_running()
    assert run["id"].tolist() == [0, 1, 3] and pl.ledger_next_id() == 4
    fresh = run[2]
    assert (fresh["slot"], fresh["c_first"], fresh["steps"], fresh["c_min"], fresh["stream"]) == (2, 1, 0, 1, int(STREAMS[0]))
    assert fresh["iter_sum"] == 0 and fresh["iter_max"] == 0 and fresh["primal"] == 0.0 and fresh["t_step"] == -1
    _bits(fresh["state"], before[0]["state"], "the imported tenant's entry state")
    _bits(np.array([fresh["min_clearance"], fresh["min_clearance_tight"]]),
          b.clearance(fresh["state"][None], np.array([pl.prob[2]], np.int32))[0], "its entry clearances")
    for name in run.dtype.names:
        _bits(run[0][name], before[0][name], f"the exported tenant's own record stays: {name}")
    pl.step()
    run = pl.ledger_running()
    # the tenant and its copy go on alike
    assert run["steps"].tolist() == [2, 2, 1]
    for name in ("state", "primal", "dual", "stream"):
        _bits(run[2][name], run[0][name], f"the copy one step on: {name}")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 5. the refusals
# ---------------------------------------------------------------------------------------------
def _ledger_state(pl):
    out = _items(pl, ("STATE", "LAMBDA", "CLOCK"))
    out.update(RUNNING=pl.ledger_running(), RECORDS=pl.ledger_records(), NEXT=np.array([pl.ledger_next_id()]))
    return out


def _unchanged(pl, before, what):
    for k, v in _ledger_state(pl).items():
        _bits(v, before[k], f"{k} after the refusal: {what}")


def test_refusals_leave_plan_and_ledger_unchanged(batches):
    b, ref = batches
    bare = obca.OBCADevicePlanner(b, **_kw([0, 1]))
    _expect(-3, "obca_ledger_begin: no clock attached", bare.ledger_begin, 4)
    _expect(-3, "obca_ledger_get: no ledger attached", bare.ledger_count)
    bare.close()
    # two tenants that retire at the same shift, one that lives on
    pl = obca.OBCADevicePlanner(b, clock=_clock((0, 0, 0), (8, 8, N_REF)), loop=_loop(range(3)), **_kw([0, 1, 2]))
    _expect(-1, "obca_ledger_begin: 1 <= cap_tenants", pl.ledger_begin, 0)
    _expect(-1, "obca_ledger_begin: 1 <= cap_tenants", pl.ledger_begin, 2 ** 20 + 1)
    _expect(-1, "obca_ledger_begin: flags must be 0", pl.ledger_begin, 4, 1)
    pl.trace_begin(2)
    _expect(-3, "obca_ledger_begin: a trace is attached", pl.ledger_begin, 4)
    pl.trace_end()
    pl.ledger_begin(1)
    before = _ledger_state(pl)
    _expect(-3, "obca_trace_begin: a ledger is attached", pl.trace_begin, 2)
    _expect(-3, "obca_clock_plan: a ledger is attached", pl.clear_clock)
    _expect(-3, "obca_clock_plan: a ledger is attached", pl.set_clock, _clock((0, 0, 0), (N_REF,) * 3))
    _expect(-3, "obca_ledger_stats: the ledger holds no record", pl.ledger_stats, [0.5], 1)
    for what, nbytes in ((0, 8), (1, 176), (2, 3 * 176 - 1), (3, 4)):
        out = np.zeros(1024, np.uint8)
        assert pl._lib.piadmm_obca_ledger_get(b._h, what, out.ctypes.data, nbytes) == -1 and not out.any()
    out = np.zeros(8, np.uint8)
    assert pl._lib.piadmm_obca_ledger_get(b._h, 4, out.ctypes.data, 8) == -1
    # two retirees do not fit a ledger of one record: the step, and the shift after its iterates
    _expect(-3, "obca_plan_step: ledger full", pl.step)
    _unchanged(pl, before, "the step")
    while pl.iterate():
        pass
    _expect(-3, "obca_ledger_begin: only at a step boundary", pl.ledger_begin, 4)
    mid = _ledger_state(pl)
    _expect(-3, "obca_plan_shift: ledger full", pl.shift)
    _unchanged(pl, mid, "the shift")
    _bits(mid["RUNNING"], before["RUNNING"], "the open records mid-step")
    pl.close()
    # an admission over an alive slot into a full ledger
    pl = obca.OBCADevicePlanner(b, clock=_clock((0, 0, 0), (8, N_REF, N_REF)), loop=_loop(range(3)), **_kw([0, 1, 2]))
    pl.ledger_begin(1)
    pl.step()
    assert pl.ledger_count() == 1
    before = _ledger_state(pl)
    _expect(-3, "obca_clock_admit: ledger full", pl.admit, [1], _clock([0], [N_REF]), specs=[F.SPECS[1]])
    _expect(-3, "obca_tenant_import: ledger full", pl.import_tenants, [1], pl.export_tenants([2]))
    _unchanged(pl, before, "the admission")
    # over the retired slot nothing is appended: it fits
    pl.admit([0], _clock([0], [N_REF]), specs=[F.SPECS[0]])
    assert pl.ledger_count() == 1 and pl.ledger_running()["id"].tolist() == [3, 1, 2]
    pl.ledger_end()
    _expect(-3, "obca_ledger_get: no ledger attached", pl.ledger_count)
    pl.ledger_end()                                   # a second end is a no-op
    pl.close()


# ---------------------------------------------------------------------------------------------
# 6. without a ledger: the bits the plan computed before
# ---------------------------------------------------------------------------------------------
def test_a_plan_without_a_ledger_is_the_plan_it_was(batches):
    b, ref = batches
    clock = _clock(C0, (N_REF, 10, N_REF))
    never = obca.OBCADevicePlanner(ref, clock=clock, loop=_loop(range(3)), **_kw([0, 1, 2]))
    never.step()
    ended = obca.OBCADevicePlanner(b, clock=clock, loop=_loop(range(3)), **_kw([0, 1, 2]))
    ended.ledger_begin(4)
    ended.ledger_end()
    ended.step()
    with_one = _items(ended)
    for k, v in _items(never).items():
        _bits(with_one[k], v, f"{k}: attached and ended against never attached")
    _bits(ended.loop_tau(), never.loop_tau(), "the latencies")
    # and a ledger that stays attached changes nothing of the plan either
    ended.close()
    kept = obca.OBCADevicePlanner(b, clock=clock, loop=_loop(range(3)), **_kw([0, 1, 2]))
    kept.ledger_begin(4)
    kept.step()
    for k, v in _items(never).items():
        _bits(_items(kept)[k], v, f"{k}: with a ledger against without")
    kept.close()
    never.close()
