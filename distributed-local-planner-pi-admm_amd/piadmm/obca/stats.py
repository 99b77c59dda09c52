"""Run records, the device-side trace, the fleet risk statistics and the worst-case gather, in NumPy."""
import ctypes
import dataclasses

import numpy as np

from .. import _lib
from .._lib import STATS_EDGES, STATS_WORST
from .model import NT, NX, clearance


class OBCARunRecord:
    """state_record / iter_num_record / lambda_record as in the script (:18-20, :100-103), one
    entry per MPC step, stacked over scenarios; status_record keeps, per ADMM iterate, the
    scenarios submitted and every local / edge status (nothing is silent)."""

    def __init__(self):
        self.state_record = []
        self.iter_num_record = []
        self.lambda_record = []
        self.status_record = []


# piadmm_obca_trace_get items: name -> (code, dtype); piadmm_obca_trace_begin's flag
TRACE_GET = {"STATES": (0, np.float64), "CLEARANCE": (1, np.float64), "ITERS": (2, np.int32),
             "STATUS_MASK": (3, np.int32), "PRIMAL": (4, np.float64), "DUAL": (5, np.float64),
             "LAMBDA": (6, np.float64), "SUMMARY": (7, np.float64), "ROWS": (8, np.int32)}
TRACE_LAMBDA = 1


@dataclasses.dataclass
class OBCATrace:
    """The device-side run record of R MPC steps of n scenarios (piadmm_obca_trace_get): states
    (R + 1) x n x 2 x 5 and clearance (R + 1) x n x 2 (plain, tight) with row 0 where the trace was
    attached; iters, primal, dual R x n and status_mask R x n x 2 per step; per scenario the
    smallest plain clearance over the rows, the first row it was reached at and the smallest
    tightened clearance; lamb R x n x 2 x 7 x 9, or None when it was not kept."""
    states: np.ndarray
    clearance: np.ndarray
    iters: np.ndarray
    status_mask: np.ndarray
    primal: np.ndarray
    dual: np.ndarray
    min_clearance: np.ndarray
    min_row: np.ndarray
    min_clearance_tight: np.ndarray
    iters_sum: np.ndarray
    lamb: np.ndarray = None


STATUS_CONVERGED = 0                  # PIADMM_OBCA_CONVERGED


@dataclasses.dataclass
class OBCAFleetStats:
    """What the statistics calls return for n scenarios, R recorded steps and B edges; index 0 is the
    plain clearance, 1 the tightened one.  hist 2 x (B + 1) int64 of the per-scenario minima,
    nonfinite (2,) int64, fleet_min (2,) / fleet_arg (2,) the smallest finite minimum and its
    scenario (+inf / -1 for none), iter_sum, iter_max, mask_or (2,), flagged, row_min / row_arg
    (R + 1) x 2 per row of the record, row_below (R + 1) x 2 x B (cumulative), worst (K,)."""
    edges: np.ndarray
    hist: np.ndarray
    nonfinite: np.ndarray
    fleet_min: np.ndarray
    fleet_arg: np.ndarray
    iter_sum: int
    iter_max: int
    mask_or: np.ndarray
    flagged: int
    row_min: np.ndarray
    row_arg: np.ndarray
    row_below: np.ndarray
    worst: np.ndarray


def stats_order(x):
    """The scenarios of x (n,) under the ordering key: value ascending, then scenario ascending, a
    value that is not finite after every finite one, again by scenario.  -0.0 ties with 0.0."""
    x = np.asarray(x, np.float64).reshape(-1)
    fin = np.isfinite(x)
    return np.lexsort((np.arange(len(x)), np.where(fin, x, 0.0), ~fin))


def _stats_first(x):
    """(value, scenario) first under the key when it is finite, else (+inf, -1)."""
    k = int(stats_order(x)[0])
    return (x[k], k) if np.isfinite(x[k]) else (np.inf, -1)


def _stats_edges(edges):
    edges = np.asarray(edges, np.float64).reshape(-1)
    if not 1 <= len(edges) <= STATS_EDGES:
        raise ValueError("1 <= B <= 64")
    for k, e in enumerate(edges):
        if not np.isfinite(e):
            raise ValueError(f"edge {k}: not finite")
        if k and not e > edges[k - 1]:
            raise ValueError(f"edge {k}: the edges must be strictly ascending")
    return edges


def record_arrays(record, prob):
    """(clear, summary, iters, mask) of an OBCARunRecord, as a trace would hold them: the clearances
    (`clearance`) of every recorded state pair, the summary (min plain, its first row, min tight, sum
    of iterates), the stop iterates and the OR of (1 << status) over each step's local / edge solves
    (from per-iterate or per-step status entries alike)."""
    states = np.stack(record.state_record)
    R, n = len(record.iter_num_record), states.shape[1]
    prob = np.broadcast_to(np.asarray(prob, int), (n,))
    clear = np.array([[clearance(states[r, s], int(prob[s])) for s in range(n)] for r in range(R + 1)],
                     np.float64).reshape(R + 1, n, 2)
    iters = np.asarray(record.iter_num_record, np.int32).reshape(R, n)
    mask = np.zeros((R, n, 2), np.int32)
    t0 = record.status_record[0]["t_step"] if record.status_record else 0
    for e in record.status_record:
        r = int(e["t_step"]) - t0
        if "local_status_mask" in e:
            mask[r, :, 0] |= np.asarray(e["local_status_mask"], np.int32)
            mask[r, :, 1] |= np.asarray(e["edge_status_mask"], np.int32)
            continue
        for k, sc in enumerate(e["scenarios"]):
            for v in (0, 1):
                mask[r, sc, 0] |= 1 << int(e["local_status"][2 * k + v])
            for c in np.asarray(e["edge_status"][k]).reshape(-1):
                mask[r, sc, 1] |= 1 << int(c)
    summary = np.zeros((n, 4))
    summary[:, 0], summary[:, 1] = clear[:, :, 0].min(axis=0), clear[:, :, 0].argmin(axis=0)
    summary[:, 2], summary[:, 3] = clear[:, :, 1].min(axis=0), iters.sum(axis=0)
    return clear, summary, iters, mask


def fleet_stats_host(clear, summary=None, iters=None, mask=None, edges=None, K=1, prob=1):
    """The statistics of include/piadmm.h in NumPy: clear (R + 1) x n x 2, summary n x 4, iters R x n,
    mask R x n x 2 (None for R = 0), ascending edges (B,), K worst.  `clear` may be an OBCARunRecord
    (with `prob` for its clearances): the arrays are then `record_arrays` of it."""
    if isinstance(clear, OBCARunRecord):
        clear, summary, iters, mask = record_arrays(clear, prob)
    clear, summary = np.asarray(clear, np.float64), np.asarray(summary, np.float64)
    R, n = clear.shape[0] - 1, clear.shape[1]
    assert clear.shape == (R + 1, n, 2) and summary.shape == (n, 4), (clear.shape, summary.shape)
    iters = np.zeros((0, n), np.int32) if iters is None else np.asarray(iters, np.int32)
    mask = np.zeros((0, n, 2), np.int32) if mask is None else np.asarray(mask, np.int32)
    assert iters.shape == (R, n) and mask.shape == (R, n, 2), (iters.shape, mask.shape)
    edges = _stats_edges(edges)
    B, K = len(edges), int(K)
    if not 1 <= K <= min(STATS_WORST, n):
        raise ValueError("1 <= K <= min(64, n)")
    hist, nonfinite = np.zeros((2, B + 1), np.int64), np.zeros(2, np.int64)
    fleet_min, fleet_arg = np.zeros(2), np.zeros(2, np.int32)
    for k, col in enumerate((0, 2)):
        x = summary[:, col]
        fin = np.isfinite(x)
        # the number of edges <= x: an x on an edge is in the upper bin
        hist[k] = np.bincount(np.searchsorted(edges, x[fin], side="right"), minlength=B + 1)
        nonfinite[k] = n - int(fin.sum())
        fleet_min[k], fleet_arg[k] = _stats_first(x)
    row_min, row_arg = np.zeros((R + 1, 2)), np.zeros((R + 1, 2), np.int32)
    row_below = np.zeros((R + 1, 2, B), np.int32)
    for r in range(R + 1):
        for k in (0, 1):
            x = clear[r, :, k]
            row_min[r, k], row_arg[r, k] = _stats_first(x)
            fin = x[np.isfinite(x)]
            row_below[r, k] = [int((fin < e).sum()) for e in edges]
    either = np.bitwise_or.reduce(mask, axis=0) if R else np.zeros((n, 2), np.int32)
    flagged = int((((either[:, 0] | either[:, 1]) & ~np.int32(1 << STATUS_CONVERGED)) != 0).sum())
    return OBCAFleetStats(
        edges=edges, hist=hist, nonfinite=nonfinite, fleet_min=fleet_min, fleet_arg=fleet_arg,
        iter_sum=sum(int(v) for v in summary[:, 3]), iter_max=int(iters.max()) if iters.size else 0,
        mask_or=np.bitwise_or.reduce(either, axis=0).astype(np.int32), flagged=flagged, row_min=row_min,
        row_arg=row_arg, row_below=row_below, worst=stats_order(summary[:, 0])[:K].astype(np.int32))


def _stats_call(call, n, R, edges, K):
    """Runs one of the two statistics entry points: call(edges, B, K, *out pointers) -> rc."""
    edges = np.ascontiguousarray(np.asarray(edges, np.float64).reshape(-1))
    B, K = len(edges), int(K)
    st = _lib.ObcaStatsC()
    hist = np.zeros((2, B + 1), np.int64)
    row_min, row_arg = np.zeros((R + 1, 2)), np.zeros((R + 1, 2), np.int32)
    row_below, worst = np.zeros((R + 1, 2, B), np.int32), np.zeros(max(K, 0), np.int32)
    # the library refuses what is out of range; the arrays only have to exist
    rc = call(_lib.dptr(edges) if B else None, B, K, ctypes.byref(st), _lib.i64ptr(hist), _lib.dptr(row_min),
              _lib.iptr(row_arg), _lib.iptr(row_below) if B else None, _lib.iptr(worst) if K > 0 else None)
    if rc != 0:
        return rc, None
    return 0, OBCAFleetStats(
        edges=edges, hist=hist, nonfinite=np.array(list(st.nonfinite), np.int64),
        fleet_min=np.array(list(st.fleet_min), np.float64), fleet_arg=np.array(list(st.fleet_arg), np.int32),
        iter_sum=int(st.iter_sum), iter_max=int(st.iter_max), mask_or=np.array(list(st.mask_or), np.int32),
        flagged=int(st.flagged), row_min=row_min, row_arg=row_arg, row_below=row_below, worst=worst)


def trace_gather_layout(R, m, keep_lambda):
    """name -> (byte offset, dtype, shape) of a gathered record of R steps and m scenarios, and its
    size in bytes (include/piadmm.h)."""
    R, m = int(R), int(m)
    P = R * m
    o_primal = 96 * (R + 1) * m
    o_iters = o_primal + 16 * P + 32 * m
    o_lamb = o_iters + 12 * P + (4 if P % 2 else 0)
    lay = {"STATES": (0, np.float64, (R + 1, m, 2, NX)), "CLEARANCE": (80 * (R + 1) * m, np.float64, (R + 1, m, 2)),
           "PRIMAL": (o_primal, np.float64, (R, m)), "DUAL": (o_primal + 8 * P, np.float64, (R, m)),
           "SUMMARY": (o_primal + 16 * P, np.float64, (m, 4)), "ITERS": (o_iters, np.int32, (R, m)),
           "STATUS_MASK": (o_iters + 4 * P, np.int32, (R, m, 2))}
    if keep_lambda:
        lay["LAMBDA"] = (o_lamb, np.float64, (R, m, 2, NT, 9))
    return lay, o_lamb + (1008 * P if keep_lambda else 0)


def trace_gather_pack(items):
    """The blob piadmm_obca_gather_trace writes for these items (name -> array; LAMBDA optional)."""
    R, m = items["ITERS"].shape
    lay, size = trace_gather_layout(R, m, "LAMBDA" in items)
    blob = np.zeros(size, np.uint8)
    for name, (off, dt, shape) in lay.items():
        a = np.ascontiguousarray(items[name], dt)
        assert a.shape == shape, (name, a.shape, shape)
        blob[off:off + a.nbytes] = a.reshape(-1).view(np.uint8)
    return blob.tobytes()


def trace_gather_unpack(blob, R, m, keep_lambda=None):
    """name -> array of a gathered record of R steps and m scenarios (copies).  keep_lambda None: LAMBDA
    is there when the blob has the size of a record that keeps it (with no step recorded the two sizes
    are one and LAMBDA, empty, is left out)."""
    blob = np.frombuffer(bytes(blob), np.uint8)
    keeps = (True, False) if keep_lambda is None else (bool(keep_lambda),)
    sizes = {trace_gather_layout(R, m, keep)[1]: keep for keep in keeps}
    if len(blob) not in sizes:
        raise ValueError(f"a gathered record of {R} steps and {m} scenarios is {sorted(sizes)} bytes, not {len(blob)}")
    lay, _ = trace_gather_layout(R, m, sizes[len(blob)])
    out = {}
    for name, (off, dt, shape) in lay.items():
        nb = int(np.prod(shape)) * np.dtype(dt).itemsize
        out[name] = blob[off:off + nb].view(dt).reshape(shape).copy()
    return out
