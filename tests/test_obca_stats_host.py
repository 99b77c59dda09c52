"""Host side of the fleet statistics and the worst-case gather (piadmm_obca_fleet_stats,
piadmm_obca_stats_trace, piadmm_obca_gather_trace, include/piadmm.h): the header's constants and the
result struct against the Python ones, the bindings, the NumPy statement obca.fleet_stats_host on
hand-made arrays, and the gathered record's layout.  No kernel runs here; a handle needs a device, so
the library's refusals are in tests/test_gpu_obca_stats.py."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_stats_cases as C
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
SYMBOLS = ("piadmm_obca_stats_size", "piadmm_obca_fleet_stats", "piadmm_obca_stats_trace",
           "piadmm_obca_gather_trace_bytes", "piadmm_obca_gather_trace")
INF, NAN = np.inf, np.nan


def _define(src, name):
    m = re.search(rf"^#define {name} (-?\d+)\s*$", src, re.M)
    assert m, name
    return int(m.group(1))


def test_header_constants_match_python():
    src = open(HEADER).read()
    assert _define(src, "PIADMM_OBCA_STATS_EDGES") == obca.STATS_EDGES == _lib.STATS_EDGES == 64
    assert _define(src, "PIADMM_OBCA_STATS_WORST") == obca.STATS_WORST == _lib.STATS_WORST == 64
    assert _define(src, "PIADMM_OBCA_CONVERGED") == obca.STATUS_CONVERGED == 0
    # purely additive: no new item of piadmm_obca_trace_get / _plan_get
    assert len(re.findall(r"^#define PIADMM_OBCA_TRACE_GET_\w+ \d+\s*$", src, re.M)) == len(obca.TRACE_GET) == 9
    assert len(re.findall(r"^#define PIADMM_OBCA_PLAN_GET_\w+ \d+\s*$", src, re.M)) == len(obca.PLAN_GET) == 36


def test_symbols_are_bound_and_exported_and_the_abi_stays():
    bound = {n for n, _, _ in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int32_t\s+(piadmm_obca_\w+)\s*\(", src, re.M))
    for name in SYMBOLS:
        assert name in declared and name in bound and hasattr(lib, name), name
    assert _lib.load().piadmm_abi_version() == 7 and _define(src, "PIADMM_ABI_VERSION") == 7


def test_result_struct_matches_the_header():
    src = open(HEADER).read()
    body = re.search(r"typedef struct \{([^}]*)\} piadmm_obca_stats_t;", src).group(1)
    fields = [(t, n.strip()) for t, names in re.findall(r"(int64_t|int32_t|double) ([^;]+);", body)
              for n in names.split(",")]
    ctype = {"int64_t": ctypes.c_int64, "int32_t": ctypes.c_int32, "double": ctypes.c_double}
    want = []
    for t, n in fields:
        m = re.fullmatch(r"(\w+)\[(\d+)\]", n)
        want.append((m.group(1), ctype[t] * int(m.group(2))) if m else (n, ctype[t]))
    assert [(n, t) for n, t in _lib.ObcaStatsC._fields_] == want
    assert _lib.load().piadmm_obca_stats_size() == ctypes.sizeof(_lib.ObcaStatsC) == 72


def _arrays(plain, tight=None, clear=None, iters=None, mask=None, sums=None):
    """Inputs of fleet_stats_host from the minima alone; the rest defaults to something harmless."""
    plain = np.asarray(plain, np.float64)
    n = len(plain)
    summary = np.zeros((n, 4))
    summary[:, 0] = plain
    summary[:, 2] = plain if tight is None else tight
    summary[:, 3] = 0 if sums is None else sums
    clear = np.zeros((1, n, 2)) if clear is None else np.asarray(clear, np.float64)
    return clear, summary, iters, mask


def test_a_value_on_an_edge_goes_to_the_upper_bin():
    st = obca.fleet_stats_host(*_arrays([0.25, 0.5, 0.5, 0.75, 1.0, 2.0, -1.0]), edges=[0.5, 1.0], K=1)
    assert st.hist.dtype == np.int64 and st.hist[0].tolist() == [2, 3, 2]
    assert st.hist[1].tolist() == [2, 3, 2] and st.nonfinite.tolist() == [0, 0]
    # the rows count strictly below, cumulatively
    clear = np.array([[[0.5, 1.0], [0.25, 0.5], [1.0, 0.75]]])
    st = obca.fleet_stats_host(*_arrays([0.0] * 3, clear=clear), edges=[0.5, 1.0], K=1)
    assert st.row_below.dtype == np.int32 and st.row_below.tolist() == [[[1, 2], [0, 2]]]


def test_ties_pick_the_lowest_scenario_and_keep_its_bits():
    st = obca.fleet_stats_host(*_arrays([1.0, 0.5, 2.0, 0.5, 0.5], [3.0, 0.0, -0.0, 0.0, 9.0]), edges=[1.0], K=5)
    assert st.fleet_min.tolist() == [0.5, 0.0] and st.fleet_arg.tolist() == [1, 1]
    assert st.worst.tolist() == [1, 3, 4, 0, 2]
    # -0.0 ties with 0.0: the lower scenario wins and the value is its own
    st = obca.fleet_stats_host(*_arrays([0.0, -0.0], [-0.0, 0.0]), edges=[1.0], K=2)
    assert st.fleet_arg.tolist() == [0, 0] and np.signbit(st.fleet_min).tolist() == [False, True]
    assert st.worst.tolist() == [0, 1]
    clear = np.array([[[2.0, 1.0], [1.0, 1.0], [1.0, 3.0]], [[5.0, NAN], [5.0, 4.0], [5.0, 4.0]]])
    st = obca.fleet_stats_host(*_arrays([0.0] * 3, clear=clear, iters=np.zeros((1, 3), np.int32),
                                        mask=np.zeros((1, 3, 2), np.int32)), edges=[1.0], K=1)
    assert st.row_min.tolist() == [[1.0, 1.0], [5.0, 4.0]] and st.row_arg.tolist() == [[1, 0], [0, 1]]


def test_not_finite_minima_are_counted_apart_and_are_in_no_bin():
    plain = [NAN, 0.5, INF, -INF, 1.5, NAN]
    st = obca.fleet_stats_host(*_arrays(plain, [0.5] * 6), edges=[1.0], K=6)
    assert st.nonfinite.tolist() == [4, 0] and st.hist.tolist() == [[1, 1], [6, 0]]
    assert int(st.hist[0].sum()) + int(st.nonfinite[0]) == 6
    assert st.fleet_min[0] == 0.5 and st.fleet_arg[0] == 1
    # finite by value then scenario, then the ones that are not finite by scenario: -inf is not "smallest"
    assert st.worst.tolist() == [1, 4, 0, 2, 3, 5]
    clear = np.array([[[NAN, -INF], [INF, 0.25], [0.5, NAN]]])
    st = obca.fleet_stats_host(*_arrays([0.0] * 3, clear=clear), edges=[0.5, 1.0], K=1)
    assert st.row_min.tolist() == [[0.5, 0.25]] and st.row_arg.tolist() == [[2, 1]]
    assert st.row_below.tolist() == [[[0, 1], [1, 1]]]


def test_all_not_finite_gives_inf_and_minus_one():
    clear = np.full((2, 3, 2), NAN)
    clear[1, :, 1] = [INF, -INF, NAN]
    st = obca.fleet_stats_host(*_arrays([NAN, INF, -INF], clear=clear, iters=np.zeros((1, 3), np.int32),
                                        mask=np.zeros((1, 3, 2), np.int32)), edges=[0.0, 1.0], K=3)
    assert st.fleet_min.tolist() == [INF, INF] and st.fleet_arg.tolist() == [-1, -1]
    assert st.row_min.tolist() == [[INF, INF]] * 2 and st.row_arg.tolist() == [[-1, -1]] * 2
    assert not st.hist.any() and not st.row_below.any() and st.nonfinite.tolist() == [3, 3]
    assert st.worst.tolist() == [0, 1, 2]


def test_flagged_counts_a_scenario_once_and_the_iterates_are_summed_exactly():
    # scenario 0: converged alone in every row; 1: another bit in both masks of two rows; 2: no solve at all;
    # 3: another bit next to converged in one edge mask
    mask = np.array([[[1, 1], [3, 2], [0, 0], [1, 1]],
                     [[1, 1], [4, 8], [0, 0], [1, 5]]], np.int32)
    iters = np.array([[3, 1, 0, 2], [2, 7, 0, 2]], np.int32)
    sums = [2.0 ** 31 - 1, 2.0 ** 31 - 2, 0.0, 2.0 ** 40]
    st = obca.fleet_stats_host(*_arrays([0.0] * 4, clear=np.zeros((3, 4, 2)), iters=iters, mask=mask, sums=sums),
                               edges=[1.0], K=1)
    assert st.flagged == 2 and st.mask_or.tolist() == [7, 15] and st.mask_or.dtype == np.int32
    assert st.iter_max == 7 and st.iter_sum == 2 ** 31 - 1 + 2 ** 31 - 2 + 2 ** 40 and type(st.iter_sum) is int
    # no recorded step: nothing flagged, no iterate
    st = obca.fleet_stats_host(*_arrays([0.0] * 4), edges=[1.0], K=1)
    assert st.flagged == 0 and st.iter_max == 0 and st.mask_or.tolist() == [0, 0] and st.row_min.shape == (1, 2)


def test_argument_checks_of_the_host_statement():
    a = _arrays([0.0, 1.0, 2.0])
    for edges, word in (([], "1 <= B"), (np.arange(65.0), "1 <= B"), ([1.0, 1.0], "edge 1"), ([2.0, 1.0], "edge 1"),
                        ([0.0, NAN], "edge 1"), ([INF], "edge 0")):
        with pytest.raises(ValueError, match=word):
            obca.fleet_stats_host(*a, edges=edges, K=1)
    for K in (0, 4):
        with pytest.raises(ValueError, match="1 <= K"):
            obca.fleet_stats_host(*a, edges=[1.0], K=K)
    with pytest.raises(ValueError, match="1 <= K"):
        obca.fleet_stats_host(*_arrays(np.zeros(70)), edges=[1.0], K=65)


@pytest.mark.parametrize("n", C.SIZES)
def test_the_kernel_cases_are_what_they_claim(n):
    """The GPU file's inputs: ties across the workgroup boundary, values on edges, the tail case's
    minimum in the last scenario alone, a sum of iterates past 32 bits."""
    for R in C.ROWS:
        clear, summary, iters, mask = C.kernel_case(n, R)
        assert clear.shape == (R + 1, n, 2) and iters.shape == (R, n) and mask.shape == (R, n, 2)
        st = obca.fleet_stats_host(clear, summary, iters, mask, C.EDGES[5], min(64, n))
        assert (st.iter_sum > 2 ** 32) == (n >= 3)
        if n == 1000:
            assert 0 < st.nonfinite[0] < n and st.iter_sum >= 2 ** 40
            x = summary[:, 0]
            for lo in range(0, n, C.ST):                 # the fleet minimum's value occurs in several workgroups
                assert (x[lo:lo + C.ST] == st.fleet_min[0]).any()
            assert np.isin(x[np.isfinite(x)], C.EDGES[5]).sum() > n // 4
        clear, summary, iters, mask = C.kernel_case(n, R, "tail")
        st = obca.fleet_stats_host(clear, summary, iters, mask, C.EDGES[1], 1)
        assert st.fleet_arg.tolist() == [n - 1] * 2 and (st.row_arg == n - 1).all() and st.worst.tolist() == [n - 1]
        clear, summary, iters, mask = C.kernel_case(n, R, "nonfinite")
        st = obca.fleet_stats_host(clear, summary, iters, mask, C.EDGES[64], 1)
        assert st.nonfinite.tolist() == [n, n] and (st.row_arg == -1).all() and st.worst.tolist() == [0]


def test_an_obcarunrecord_is_accepted():
    """The statement on an OBCARunRecord (per-step status entries, as the device planner keeps them, and
    per-iterate ones, as the host planner does) is the statement on `record_arrays` of it."""
    rec = obca.OBCARunRecord()
    for t in (8.0, 16.0, 24.0):
        rec.state_record.append(np.stack([np.stack([obca.executed_path(v, t * obca.DT, sp) for v in (0, 1)])
                                          for sp in (None, obca.OvertakeSpec(18, 12, 15, 3.5))]))
    rec.iter_num_record = [np.array([3, 2]), np.array([1, 4])]
    rec.status_record = [dict(t_step=8, iters=None, local_status_mask=np.array([1, 3]), edge_status_mask=np.array([1, 1])),
                         dict(t_step=9, i_iter=1, scenarios=[1], local_status=np.array([0, 1]),
                              edge_status=np.array([[0, 0, 0, 3, 0, 0, 0]]))]
    clear, summary, iters, mask = obca.record_arrays(rec, prob=[1, 0])
    assert clear.shape == (3, 2, 2) and np.array_equal(clear[:, 1, 0], clear[:, 1, 1]) and (clear >= 0).all()
    assert iters.tolist() == [[3, 2], [1, 4]] and summary[:, 3].tolist() == [4.0, 6.0]
    assert mask.tolist() == [[[1, 1], [3, 1]], [[0, 0], [3, 9]]]
    assert np.array_equal(summary[:, 0], clear[:, :, 0].min(axis=0))
    edges = [float(np.median(clear[:, :, 0]))]
    C.same(obca.fleet_stats_host(rec, edges=edges, K=2, prob=[1, 0]),
           obca.fleet_stats_host(clear, summary, iters, mask, edges, 2))
    assert obca.fleet_stats_host(rec, edges=edges, K=2, prob=[1, 0]).flagged == 1


@pytest.mark.parametrize("R,m,keep", [(0, 1, False), (0, 3, True), (1, 1, True), (3, 3, False), (3, 3, True), (2, 5, True)])
def test_gather_layout_and_round_trip(R, m, keep):
    rng = np.random.default_rng(R * 10 + m)
    lay, size = obca.trace_gather_layout(R, m, keep)
    P = R * m
    # the header's offsets, written out
    I = 96 * (R + 1) * m + 16 * P + 32 * m
    L = I + 12 * P + (4 if P % 2 else 0)
    assert {k: v[0] for k, v in lay.items() if k != "LAMBDA"} == dict(
        STATES=0, CLEARANCE=80 * (R + 1) * m, PRIMAL=96 * (R + 1) * m, DUAL=96 * (R + 1) * m + 8 * P,
        SUMMARY=96 * (R + 1) * m + 16 * P, ITERS=I, STATUS_MASK=I + 4 * P)
    assert size == L + (1008 * P if keep else 0) and size % 8 == 0 and ("LAMBDA" in lay) == keep
    if keep:
        assert lay["LAMBDA"][0] == L and L % 8 == 0
    # the segments tile the blob but for the pad word
    spans = sorted((off, off + int(np.prod(shape)) * np.dtype(dt).itemsize) for off, dt, shape in lay.values())
    assert spans[0][0] == 0 and all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))
    assert size - sum(b - a for a, b in spans) == (4 if P % 2 else 0)
    items = {}
    for name, (off, dt, shape) in lay.items():
        items[name] = (rng.integers(-5, 60, shape).astype(dt) if dt == np.int32 else rng.normal(size=shape))
    blob = obca.trace_gather_pack(items)
    assert len(blob) == size
    back = obca.trace_gather_unpack(blob, R, m, keep)
    assert set(back) == set(items)
    if P:                                               # the size tells whether LAMBDA is there
        assert set(obca.trace_gather_unpack(blob, R, m)) == set(items)
    for name in items:
        assert back[name].dtype == items[name].dtype and back[name].tobytes() == items[name].tobytes(), name
    with pytest.raises(ValueError, match="bytes"):
        obca.trace_gather_unpack(blob + b"\0" * 8, R, m)
