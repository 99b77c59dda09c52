"""Fleet risk statistics and the worst-case gather of the device-resident OBCA plan (k_stats_fleet,
k_stats_rows, k_stats_worst and k_trace_gather in csrc/piadmm_obca_plan_trace.hip behind
piadmm_obca_fleet_stats / piadmm_obca_stats_trace / piadmm_obca_gather_trace; OBCABatch.fleet_stats,
OBCADevicePlanner.trace_stats, trace_gather, trace_worst).

Bars.  Every result is an integer count, a minimum of doubles or a copy, so every comparison is bit
equality: the kernels against obca.fleet_stats_host on the same arrays, the gathered record against
fancy-indexed slices of trace_get.  There is no tolerance here.

The in-plan tests run the 3-scenario fleet of tests/test_gpu_obca_feedback.py (different
OvertakeSpecs, max_admm_iter <= 2, t_step0 = 12, PAR and the 2-row TAPE) for 2 MPC steps, once."""
import numpy as np
import pytest

import _obca_clock_cases as CK
import _obca_fleet_cases as F
import _obca_stats_cases as C
import test_gpu_obca_feedback as FB
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

_bits = P._bits
CASES, T0, N = FB.CASES, FB.T0, FB.N
TRACE_ITEMS = ("STATES", "CLEARANCE", "ITERS", "STATUS_MASK", "PRIMAL", "DUAL", "SUMMARY", "LAMBDA")
PLAN_ITEMS = ("STATE", "STATE_PREV", "CTRL", "CTRL_PREV", "X", "ITERS", "ACTIVE", "PRIMAL", "DUAL", "STOP", "CONVERGE",
              "LOCAL_REC", "LOCAL_OUT", "LOCAL_IST", "EDGE_REC", "EDGE_OUT", "EDGE_IST", "T_STEP", "LAMBDA", "COUNTS",
              "STATUS_MASK", "REF", "PAR", "PRIMAL_THRES", "DUAL_THRES", "PROB", "FEEDBACK_PAR", "FEEDBACK_STEPS")


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


def _trace_items(pl, lamb=True):
    return {k: pl.trace_get(k) for k in TRACE_ITEMS if lamb or k != "LAMBDA"}


def _all_items(pl, lamb=True, plan_items=PLAN_ITEMS):
    out = {"plan " + k: pl.get(k) for k in plan_items}
    out.update({"trace " + k: v for k, v in _trace_items(pl, lamb).items()})
    out["trace ROWS"] = np.array([pl.trace_rows()], np.int32)
    return out


def _unchanged(before, after):
    assert set(before) == set(after)
    for k in before:
        _bits(after[k], before[k], k)


def _host(items, edges, K):
    return obca.fleet_stats_host(items["CLEARANCE"], items["SUMMARY"], items["ITERS"], items["STATUS_MASK"], edges, K)


def _edges_of(items):
    """Edges from the measured clearances: the midpoints between the sorted distinct plain minima (one
    of them separates the scenarios, and two bins of the minima are then not empty), and one of the
    minima itself, which must land in the upper bin."""
    mins = np.unique(items["SUMMARY"][:, 0])
    assert len(mins) >= 2, mins
    mid = (mins[:-1] + mins[1:]) / 2
    edges = np.unique(np.concatenate((mid, mins[:1])))
    return edges


def _expect(code, what, call, *a, **k):
    with pytest.raises(_lib.PiadmmError, match=what) as e:
        call(*a, **k)
    assert f"error {code}:" in str(e.value), str(e.value)


@pytest.fixture(scope="module")
def traced(batches):
    """The feedback fleet with a trace that keeps LAMBDA, after 2 steps; the planner stays open."""
    b, _ = batches
    pl = obca.OBCADevicePlanner(b, feedback=dict(par=FB.PAR, tape=FB.TAPE), **dict(F.fleet_kwargs(CASES, T0)))
    pl.trace_begin(4, keep_lambda=True)
    assert pl.trace_run(2) == 2
    yield pl
    pl.close()


# ---------------------------------------------------------------------------------------------
# the kernels alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("R", C.ROWS)
@pytest.mark.parametrize("n", C.SIZES)
def test_kernels_alone(batches, n, R):
    b, _ = batches
    clear, summary, iters, mask = C.kernel_case(n, R)
    keep = [a.copy() for a in (clear, summary, iters, mask)]
    for B, edges in C.EDGES.items():
        for K in sorted({1, min(64, n)}):
            got = b.fleet_stats(clear, summary, iters if R else None, mask if R else None, edges, worst=K)
            want = obca.fleet_stats_host(clear, summary, iters, mask, edges, K)
            C.same(got, want, (n, R, B, K))
            assert int(got.hist[0].sum()) + int(got.nonfinite[0]) == n
    # a 32-bit accumulator would have wrapped
    assert got.iter_sum == sum(2 ** 31 - 1 - (s % 7) for s in range(n)) and (n < 3 or got.iter_sum > 2 ** 32)
    # the same on a second run, and the inputs are as they were
    C.same(b.fleet_stats(clear, summary, iters if R else None, mask if R else None, edges, worst=K), got, "repeat")
    for a, k in zip((clear, summary, iters, mask), keep):
        assert a.tobytes() == k.tobytes()


@pytest.mark.parametrize("variant", ["tail", "nonfinite"])
@pytest.mark.parametrize("n", C.SIZES)
def test_kernels_alone_tail_and_empty(batches, n, variant):
    """tail: the minimum sits in the last lane of the last workgroup alone.  nonfinite: no value is
    finite, so every minimum is +inf with scenario -1, every count is 0 and `worst` is 0, 1, 2, ..."""
    b, _ = batches
    for R in (0, 3):
        clear, summary, iters, mask = C.kernel_case(n, R, variant)
        K = min(64, n)
        got = b.fleet_stats(clear, summary, iters if R else None, mask if R else None, C.EDGES[5], worst=K)
        C.same(got, obca.fleet_stats_host(clear, summary, iters, mask, C.EDGES[5], K), (n, R, variant))
        if variant == "tail":
            assert got.fleet_arg.tolist() == [n - 1] * 2 and (got.row_arg == n - 1).all() and got.worst[0] == n - 1
            assert (got.row_min == -2.0).all()
        else:
            assert got.fleet_arg.tolist() == [-1, -1] and np.isposinf(got.fleet_min).all() and not got.hist.any()
            assert (got.row_arg == -1).all() and np.isposinf(got.row_min).all() and not got.row_below.any()
            assert got.worst.tolist() == list(range(K)) and got.nonfinite.tolist() == [n, n]


def test_kernels_alone_many_workgroups(batches):
    """547 workgroups of partials: the second launch strides over its records, and k_stats_worst needs
    four merge levels at K = 64 (547 lists -> 69 -> 9 -> 2 -> 1) and two at K = 1."""
    b, _ = batches
    n = 70001
    clear, summary, iters, mask = C.kernel_case(n, 1)
    assert -(-n // C.ST) == 547
    for K in (1, 64):
        got = b.fleet_stats(clear, summary, iters, mask, C.EDGES[5], worst=K)
        C.same(got, obca.fleet_stats_host(clear, summary, iters, mask, C.EDGES[5], K), K)
    assert got.iter_sum > 2 ** 47


def test_kernels_alone_refusals(batches):
    b, _ = batches
    clear, summary, iters, mask = C.kernel_case(5, 1)
    ok = C.EDGES[5]
    _expect(-1, "1 <= B <= 64", b.fleet_stats, clear, summary, iters, mask, [], worst=1)
    _expect(-1, "1 <= B <= 64", b.fleet_stats, clear, summary, iters, mask, np.arange(65.0), worst=1)
    _expect(-1, "obca_fleet_stats: edge 2: .*ascending", b.fleet_stats, clear, summary, iters, mask, [0.0, 2.0, 1.0], worst=1)
    _expect(-1, "obca_fleet_stats: edge 1: .*ascending", b.fleet_stats, clear, summary, iters, mask, [1.0, 1.0], worst=1)
    _expect(-1, "obca_fleet_stats: edge 1: not finite", b.fleet_stats, clear, summary, iters, mask, [0.0, np.nan], worst=1)
    _expect(-1, "obca_fleet_stats: edge 0: not finite", b.fleet_stats, clear, summary, iters, mask, [np.inf], worst=1)
    _expect(-1, "1 <= K <= min", b.fleet_stats, clear, summary, iters, mask, ok, worst=0)
    _expect(-1, "1 <= K <= min", b.fleet_stats, clear, summary, iters, mask, ok, worst=6)
    big = C.kernel_case(70, 0)
    _expect(-1, "1 <= K <= min", b.fleet_stats, big[0], big[1], None, None, ok, worst=65)
    _expect(-1, "null argument", b.fleet_stats, clear, summary, None, None, ok, worst=1)       # R = 1 needs both
    for bad in (-1.0, 0.5, np.nan, 2.0 ** 41):
        s2 = summary.copy()
        s2[3, 3] = bad
        _expect(-1, "obca_fleet_stats: row 3: ", b.fleet_stats, clear, s2, iters, mask, ok, worst=1)
    _expect(-1, "1 <= n", b.fleet_stats, clear[:, :0], summary[:0], iters[:, :0], mask[:, :0], ok, worst=1)


# ---------------------------------------------------------------------------------------------
# in the plan
# ---------------------------------------------------------------------------------------------
def test_trace_stats_is_the_host_statement_and_changes_nothing(traced):
    pl = traced
    before = _all_items(pl)
    items = _trace_items(pl)
    assert items["ITERS"].shape == (2, N) and (items["ITERS"] > 0).all()
    edges = _edges_of(items)
    got = pl.trace_stats(edges, worst=N)
    want = _host(items, edges, N)
    C.same(got, want, "trace_stats")
    # the edges do what they were chosen for: two bins of the minima hold something, one edge separates
    # the scenarios, and the minimum that is an edge went to the upper bin
    assert (got.hist[0] > 0).sum() >= 2 and int(got.hist[0].sum()) == N and not got.nonfinite.any()
    assert 0 < (items["SUMMARY"][:, 0] < edges[1]).sum() < N
    assert got.hist[0][0] == 0 and got.hist[0][1] >= 1
    assert got.iter_sum == int(items["ITERS"].sum()) and got.iter_max == int(items["ITERS"].max())
    assert got.worst.tolist() == np.lexsort((np.arange(N), items["SUMMARY"][:, 0])).tolist()
    # other B and K on the same trace
    for e, K in ((edges[:1], 1), (np.linspace(0.0, float(items["CLEARANCE"].max()), 64), 2)):
        C.same(pl.trace_stats(e, worst=K), _host(items, e, K), f"B = {len(e)}")
    _unchanged(before, _all_items(pl))


@pytest.mark.parametrize("slots", [[2, 0], [1]])
def test_gather_is_the_slice_of_trace_get(traced, slots):
    pl = traced
    before = _all_items(pl)
    items = _trace_items(pl)
    got = pl.trace_gather(slots)
    assert set(got) == set(TRACE_ITEMS)
    R, m = 2, len(slots)
    assert pl.trace_gather_bytes(m) == obca.trace_gather_layout(R, m, True)[1]
    for name in TRACE_ITEMS:
        want = items[name][slots] if name == "SUMMARY" else items[name][:, slots]
        _bits(got[name], want, name)
    _unchanged(before, _all_items(pl))


def test_trace_worst(traced):
    pl = traced
    items = _trace_items(pl)
    edges = _edges_of(items)
    st, rec = pl.trace_worst(edges, 2)
    want = _host(items, edges, 2)
    C.same(st, want, "trace_worst")
    worst = want.worst.tolist()
    assert worst == obca.stats_order(items["SUMMARY"][:, 0])[:2].tolist()
    for name in TRACE_ITEMS:
        _bits(rec[name], items[name][worst] if name == "SUMMARY" else items[name][:, worst], name)


def test_refusals_leave_the_trace_as_it_was(traced):
    pl = traced
    before = _all_items(pl)
    ok = _edges_of(_trace_items(pl))
    _expect(-1, "1 <= B <= 64", pl.trace_stats, [], worst=1)
    _expect(-1, "1 <= B <= 64", pl.trace_stats, np.arange(65.0), worst=1)
    _expect(-1, "obca_stats_trace: edge 1: .*ascending", pl.trace_stats, [2.0, 1.0], worst=1)
    _expect(-1, "obca_stats_trace: edge 1: not finite", pl.trace_stats, [0.0, np.nan], worst=1)
    _expect(-1, "1 <= K <= min", pl.trace_stats, ok, worst=0)
    _expect(-1, "1 <= K <= min", pl.trace_stats, ok, worst=N + 1)
    _expect(-1, "slots\\[1\\]", pl.trace_gather, [1, 1])
    _expect(-1, "slots\\[0\\]", pl.trace_gather, [N])
    _expect(-1, "slots\\[1\\]", pl.trace_gather, [0, -1])
    _expect(-1, "1 <= m", pl.trace_gather, [])
    _expect(-1, "1 <= m", pl.trace_gather, [0, 1, 2, 0])
    size = pl.trace_gather_bytes(2)
    for wrong in (size - 8, size + 8, 0):
        _expect(-1, f"the blob is {size} bytes", pl.trace_gather, [2, 0], nbytes=wrong)
    _expect(-1, "1 <= m", pl.trace_gather_bytes, 0)
    _expect(-1, "1 <= m", pl.trace_gather_bytes, N + 1)
    _unchanged(before, _all_items(pl))


def test_stand_alone_call_next_to_an_open_plan(batches, traced):
    b, _ = batches
    pl = traced
    assert pl.batch is b
    before = _all_items(pl)
    clear, summary, iters, mask = C.kernel_case(130, 3)
    C.same(b.fleet_stats(clear, summary, iters, mask, C.EDGES[5], worst=64),
           obca.fleet_stats_host(clear, summary, iters, mask, C.EDGES[5], 64), "next to a plan")
    _expect(-1, "1 <= B <= 64", b.fleet_stats, clear, summary, iters, mask, [], worst=1)
    _unchanged(before, _all_items(pl))
    # and the plan goes on: the statistics of the trace are what they were
    edges = _edges_of(_trace_items(pl))
    C.same(pl.trace_stats(edges, worst=1), _host(_trace_items(pl), edges, 1), "after")


def test_without_a_trace_and_without_a_plan(batches):
    _, ref = batches
    pl = obca.OBCADevicePlanner(ref, **F.fleet_kwargs(CASES, T0))
    plan_items = tuple(k for k in PLAN_ITEMS if not k.startswith("FEEDBACK"))
    before = {k: pl.get(k) for k in plan_items}
    _expect(-3, "obca_stats_trace: no trace attached", pl.trace_stats, [1.0], worst=1)
    _expect(-3, "obca_gather_trace_bytes: no trace attached", pl.trace_gather_bytes, 1)
    _expect(-3, "obca_gather_trace: no trace attached", pl.trace_gather, [0], nbytes=8)
    _unchanged(before, {k: pl.get(k) for k in plan_items})
    # without LAMBDA the record ends behind STATUS_MASK
    pl.trace_begin(3, keep_lambda=False)
    assert pl.trace_run(1) == 1
    items = _trace_items(pl, lamb=False)
    for slots in ([2, 0], [1]):
        got = pl.trace_gather(slots)
        assert set(got) == set(TRACE_ITEMS) - {"LAMBDA"}
        assert pl.trace_gather_bytes(len(slots)) == obca.trace_gather_layout(1, len(slots), False)[1]
        for name in got:
            _bits(got[name], items[name][slots] if name == "SUMMARY" else items[name][:, slots], name)
    pl.trace_end()
    _expect(-3, "no trace attached", pl.trace_stats, [1.0], worst=1)
    pl.close()
    _expect(-3, "obca_stats_trace: no open plan", pl.trace_stats, [1.0], worst=1)
    _expect(-3, "obca_gather_trace: no open plan", pl.trace_gather, [0], nbytes=8)
    _expect(-3, "obca_gather_trace_bytes: no open plan", pl.trace_gather_bytes, 1)


def test_under_a_clock_the_frozen_rows_count_as_they_stand(batches):
    """Scenario 1's reference ends after step 1: its second row repeats the frozen state and clearance
    with iterate 0 and masks 0, and the statistics are taken over the trace as it stands."""
    _, ref = batches
    rows = np.array([[T0, CK.N_REF], [T0, T0 + 8], [T0, CK.N_REF]], np.int32)
    pl = obca.OBCADevicePlanner(ref, clock=rows, **F.fleet_kwargs(CASES, T0))
    pl.trace_begin(4, keep_lambda=True)
    assert pl.trace_run(2) == 2
    assert pl.alive().tolist() == [True, False, True]
    items = _trace_items(pl)
    assert items["ITERS"][1, 1] == 0 and not items["STATUS_MASK"][1, 1].any() and (items["ITERS"][0] > 0).all()
    _bits(items["CLEARANCE"][2, 1], items["CLEARANCE"][1, 1], "the retired scenario's repeated row")
    _bits(items["STATES"][2, 1], items["STATES"][1, 1], "the retired scenario's repeated state")
    before = _all_items(pl, plan_items=("STATE", "STATE_PREV", "X", "CTRL", "ITERS", "STATUS_MASK", "LAMBDA", "CLOCK",
                                        "WINDOW", "T_STEP", "COUNTS"))
    edges = _edges_of(items)
    got = pl.trace_stats(edges, worst=N)
    C.same(got, _host(items, edges, N), "clocked")
    assert got.iter_sum == int(items["ITERS"].sum())
    rec = pl.trace_gather([1, 2])
    for name in TRACE_ITEMS:
        _bits(rec[name], items[name][[1, 2]] if name == "SUMMARY" else items[name][:, [1, 2]], name)
    _unchanged(before, _all_items(pl, plan_items=("STATE", "STATE_PREV", "X", "CTRL", "ITERS", "STATUS_MASK", "LAMBDA",
                                                  "CLOCK", "WINDOW", "T_STEP", "COUNTS")))
    pl.close()
