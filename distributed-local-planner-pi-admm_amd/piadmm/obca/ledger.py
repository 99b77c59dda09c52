"""The tenant ledger (csrc/piadmm_obca_plan_ledger.hip, piadmm_obca_ledger_begin): one risk record per
tenant of a clocked plan, opened when the tenant enters its slot, updated by every step it closes and
appended when it leaves -- the record's layout, the statistics' view of the records and the same
bookkeeping in NumPy."""
import numpy as np

from .._lib import LEDGER_REC
from .model import NX, clearance
from .stats import fleet_stats_host

# piadmm_obca_ledger_get items: name -> (code, dtype) (PIADMM_OBCA_LEDGER_GET_*)
LEDGER_GET = {"COUNT": (0, np.int32), "RECORDS": (1, np.uint8), "RUNNING": (2, np.uint8), "NEXT_ID": (3, np.int64)}
# the reasons a record is appended for (0: an open record)
LEDGER_RETIRED, LEDGER_ADMITTED, LEDGER_IMPORTED = 1, 2, 3
# a record, word by word (include/piadmm.h): 22 words of 8 bytes
LEDGER_DTYPE = np.dtype([
    ("id", np.int64), ("stream", np.int64), ("slot", np.int32), ("reason", np.int32), ("c_first", np.int32),
    ("steps", np.int32), ("min_clearance", np.float64), ("min_clearance_tight", np.float64), ("c_min", np.int32),
    ("iter_max", np.int32), ("iter_sum", np.int64), ("local_status_mask", np.int32), ("edge_status_mask", np.int32),
    ("primal", np.float64), ("dual", np.float64), ("t_step", np.int32), ("reserved", np.int32),
    ("state", np.float64, (2, NX))])
assert LEDGER_DTYPE.itemsize == LEDGER_REC


def ledger_unpack(blob):
    """The records of a RECORDS or RUNNING item (bytes, or a uint8 array) as a structured array
    (LEDGER_DTYPE), a copy."""
    blob = np.frombuffer(bytes(blob), np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) \
        else np.ascontiguousarray(blob, np.uint8).reshape(-1)
    if len(blob) % LEDGER_REC:
        raise ValueError(f"a ledger blob is a multiple of {LEDGER_REC} bytes, not {len(blob)}")
    return blob.view(LEDGER_DTYPE).copy()


def ledger_pack(records):
    """The bytes piadmm_obca_ledger_get writes for these records."""
    return np.ascontiguousarray(records, LEDGER_DTYPE).tobytes()


def ledger_view(records):
    """(clear, summary, iters, mask) of the records as a run record of R = 1 step and n = count
    scenarios, what k_ledger_view builds: summary count x 4 (min plain, c_min, min tight, the iterate
    sum), clear 2 x count x 2 (both rows the minima), iters 1 x count (the largest stop iterate), mask
    1 x count x 2 (the two ORs).  A scenario of the view is a record's position."""
    r = np.asarray(records, LEDGER_DTYPE).reshape(-1)
    C = len(r)
    summary = np.zeros((C, 4))
    summary[:, 0], summary[:, 1] = r["min_clearance"], r["c_min"]
    summary[:, 2], summary[:, 3] = r["min_clearance_tight"], r["iter_sum"]
    clear = np.zeros((2, C, 2))
    clear[:, :, 0], clear[:, :, 1] = r["min_clearance"], r["min_clearance_tight"]
    iters = r["iter_max"].astype(np.int32).reshape(1, C)
    mask = np.stack((r["local_status_mask"], r["edge_status_mask"]), axis=1).astype(np.int32).reshape(1, C, 2)
    return clear, summary, iters, mask


def ledger_stats_host(records, edges, K=1):
    """piadmm_obca_ledger_stats in NumPy: `fleet_stats_host` on `ledger_view` of the records."""
    clear, summary, iters, mask = ledger_view(records)
    return fleet_stats_host(clear, summary, iters, mask, edges=edges, K=K)


class OBCALedger:
    """The ledger's bookkeeping on the host, by the rules of include/piadmm.h: `running` the open record
    of every slot (id -1: no tenant), `records` the appended ones, `next_id` the id the next admitted
    tenant takes.  OBCAPlanner(clock=..., ledger=True) drives it; the clearances are `clearance`."""

    def __init__(self, n, cap=None):
        self.n, self.cap = int(n), cap
        self.running = np.zeros(self.n, LEDGER_DTYPE)
        self.running["id"] = -1
        self.running["t_step"] = -1
        self.running["slot"] = np.arange(self.n)
        self.appended = []
        self.next_id = self.n

    @property
    def records(self):
        return np.array(self.appended, LEDGER_DTYPE) if self.appended else np.zeros(0, LEDGER_DTYPE)

    @property
    def count(self):
        return len(self.appended)

    def clear(self):
        self.appended = []

    def open(self, s, ident, c, state, prob, stream=-1):
        """A fresh open record of slot s for tenant `ident` at clock c and entry state `state` (2 x 5)."""
        r = np.zeros((), LEDGER_DTYPE)
        plain, tight = clearance(np.asarray(state, np.float64), int(prob))
        r["id"], r["stream"], r["slot"], r["c_first"], r["c_min"], r["t_step"] = ident, stream, s, c, c, -1
        r["min_clearance"], r["min_clearance_tight"], r["state"] = plain, tight, state
        self.running[s] = r

    def admit(self, s, c, state, prob, stream=-1):
        """`open` with the next id."""
        self.open(s, self.next_id, c, state, prob, stream)
        self.next_id += 1

    def step(self, s, c_new, state, prob, it, local_mask, edge_mask, primal, dual, stream=-1):
        """The open record of slot s takes a closed step: c_new the tenant's clock at the new state."""
        r = self.running[s]
        plain, tight = clearance(np.asarray(state, np.float64), int(prob))
        r["steps"] += 1
        if plain < r["min_clearance"]:
            r["min_clearance"], r["c_min"] = plain, c_new
        if tight < r["min_clearance_tight"]:
            r["min_clearance_tight"] = tight
        r["iter_max"] = max(int(r["iter_max"]), int(it))
        r["iter_sum"] += int(it)
        r["local_status_mask"] |= int(local_mask)
        r["edge_status_mask"] |= int(edge_mask)
        r["primal"], r["dual"], r["state"], r["stream"] = primal, dual, state, stream
        self.running[s] = r

    def close(self, s, reason, t_step, stream=None):
        """Append the open record of slot s (which must hold a tenant); the slot then holds none."""
        assert self.running[s]["id"] >= 0, f"slot {s} holds no tenant"
        if self.cap is not None and self.count >= self.cap:
            raise ValueError("ledger full")
        r = self.running[s].copy()
        r["reason"], r["t_step"] = reason, t_step
        if stream is not None:
            r["stream"] = stream
        self.appended.append(r)
        self.running[s]["id"] = -1
