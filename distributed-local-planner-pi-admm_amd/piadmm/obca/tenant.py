"""A scenario's resident state in the device plan and the tenant record, in NumPy."""
import numpy as np

from .._lib import DELAY_PAR, DUAL_PAR, FEEDBACK_PAR, FLEET_PAR, NOISE_PAR
from .feedback import delay_row_check, feedback_row_check, noise_row_check
from .model import DT, N_HORZ, NT, NU, NX


PLAN_STATE = 556
# the state's fields in order (include/piadmm.h): name, shape
PLAN_FIELDS = (("Z_bar", (2, NT, 9)), ("A", (2, NT, 4, 2)), ("b", (2, NT, 4)), ("lamb_bar", (2, NT, 9)),
               ("lamb_ij", (2, NT, 4)), ("local_x", (2, NT, 5)), ("init_state", (2, 5)))
# piadmm_obca_plan_get items: name -> (code, dtype)
PLAN_GET = {"STATE": (0, np.float64), "STATE_PREV": (1, np.float64), "CTRL": (2, np.float64),
            "CTRL_PREV": (3, np.float64), "X": (4, np.float64), "ITERS": (5, np.int32), "ACTIVE": (6, np.int32),
            "PRIMAL": (7, np.float64), "DUAL": (8, np.float64), "STOP": (9, np.int32), "CONVERGE": (10, np.int32),
            "LOCAL_REC": (11, np.float64), "LOCAL_OUT": (12, np.float64), "LOCAL_IST": (13, np.int32),
            "EDGE_REC": (14, np.float64), "EDGE_OUT": (15, np.float64), "EDGE_IST": (16, np.int32),
            "T_STEP": (17, np.int32), "LAMBDA": (18, np.float64), "COUNTS": (19, np.int32),
            "STATUS_MASK": (20, np.int32), "REF": (21, np.float64), "PAR": (22, np.float64),
            "DUAL_S": (23, np.float64), "DUAL_D": (24, np.float64), "DUAL_PAR": (25, np.float64),
            "WORK": (26, np.int32), "CLOCK": (27, np.int32), "WINDOW": (28, np.float64),
            "PRIMAL_THRES": (29, np.float64), "DUAL_THRES": (30, np.float64), "PROB": (31, np.int32),
            "DUAL_S_PREV": (32, np.float64), "DUAL_D_PREV": (33, np.float64),
            "FEEDBACK_PAR": (34, np.float64), "FEEDBACK_STEPS": (35, np.int32)}


def pack_state(bar, init_state):
    """One scenario's resident state (PLAN_STATE doubles) from a bar_state and its 2 x 5 init_state."""
    parts = dict(bar, init_state=init_state)
    out = np.concatenate([np.asarray(parts[k], np.float64).reshape(-1) for k, _ in PLAN_FIELDS])
    assert out.shape == (PLAN_STATE,)
    return out


def unpack_state(vec):
    """(bar_state, init_state) of one scenario's resident state: copies, the inverse of `pack_state`."""
    vec = np.asarray(vec, np.float64)
    assert vec.shape == (PLAN_STATE,)
    bar, o = {}, 0
    for k, shp in PLAN_FIELDS:
        n = int(np.prod(shp))
        bar[k] = vec[o:o + n].reshape(shp).copy()
        o += n
    init = bar.pop("init_state")
    return bar, init


# the tenant record of piadmm_obca_tenant_export / _import (include/piadmm.h)
TENANT_MAGIC = 0x314E5454
TENANT_ABI = 7
TENANT_HEADER = 64                    # bytes: sixteen int32
TENANT_INTS = 12                      # int32 words behind the fp64 section of a record
TENANT_F64 = 1474                     # fp64 words of a record, + 10 n_ref, + TENANT_F64_LAW with a law
TENANT_F64_LAW = 512
TENANT_F64_LOOP = 50                  # + this with the loop: the rows, the open step's latencies, the stream id
# the loop section: name -> (first word behind the law's section, words); LOOP_STREAMS is the int64's bits
TENANT_LOOP_FIELDS = (("LOOP_PLANT", FEEDBACK_PAR), ("LOOP_NOISE", NOISE_PAR), ("LOOP_DELAY", DELAY_PAR), ("LOOP_TAU", 2),
                      ("LOOP_STREAMS", 1), ("_loop_pad", 1))
# the int32 section: name -> (first word, words)
TENANT_INT_FIELDS = {"ITERS": (0, 1), "STOP": (1, 1), "CONVERGE": (2, 1), "PROB": (3, 1), "STATUS_MASK": (4, 2),
                     "WORK": (6, 2), "CLOCK": (8, 3)}
_TENANT_SHAPES = {"STATE": (PLAN_STATE,), "STATE_PREV": (PLAN_STATE,), "CTRL": (2, NT * NU), "CTRL_PREV": (2, NT * NU),
                  "X": (2, N_HORZ, NX), "LAMBDA": (2, NT, 9), "PRIMAL": (), "DUAL": (), "PRIMAL_THRES": (),
                  "DUAL_THRES": (), "PAR": (FLEET_PAR,), "WINDOW": (2, N_HORZ, NX), "DUAL_S": (2, NT, 9),
                  "DUAL_D": (2, NT, 9), "DUAL_S_PREV": (2, NT, 9), "DUAL_D_PREV": (2, NT, 9), "DUAL_PAR": (DUAL_PAR,),
                  "ITERS": (), "STOP": (), "CONVERGE": (), "PROB": (), "STATUS_MASK": (2,), "WORK": (2,), "CLOCK": (3,),
                  "LOOP_PLANT": (FEEDBACK_PAR,), "LOOP_NOISE": (NOISE_PAR,), "LOOP_DELAY": (DELAY_PAR,), "LOOP_TAU": (2,)}


def tenant_layout(n_ref, law=False, loop=False):
    """The layout of one tenant record: dict(f64={name: (first fp64 word, words)}, F=the fp64 words,
    ints=TENANT_INT_FIELDS, record_bytes=8 F + 48), as the table of include/piadmm.h has it; with
    loop= the loop section (TENANT_LOOP_FIELDS) behind the law's."""
    fields = [("STATE", PLAN_STATE), ("STATE_PREV", PLAN_STATE), ("CTRL", 28), ("CTRL_PREV", 28), ("X", 80),
              ("LAMBDA", 126), ("PRIMAL", 1), ("DUAL", 1), ("PRIMAL_THRES", 1), ("DUAL_THRES", 1), ("PAR", FLEET_PAR),
              ("REF", 10 * int(n_ref)), ("WINDOW", 80)]
    if law:
        fields += [("DUAL_S", 126), ("DUAL_D", 126), ("DUAL_S_PREV", 126), ("DUAL_D_PREV", 126), ("DUAL_PAR", DUAL_PAR)]
    if loop:
        fields += list(TENANT_LOOP_FIELDS)
    f64, o = {}, 0
    for name, words in fields:
        f64[name] = (o, words)
        o += words
    assert o == TENANT_F64 + 10 * int(n_ref) + (TENANT_F64_LAW if law else 0) + (TENANT_F64_LOOP if loop else 0)
    return dict(f64=f64, F=o, ints=dict(TENANT_INT_FIELDS), record_bytes=8 * o + 4 * TENANT_INTS)


def _tenant_row_check(par):
    """What the library's row check refuses of a parameter row (None: the row is good)."""
    rho, _, _, max_x, max_y, r, q, x_bound, mu_max, _, admm, sqp, rnd, start = (float(v) for v in par[:14])

    def integral(v, lo, hi):
        return lo <= v <= hi and v == np.floor(v)
    if not (rho > 0 and r > 0 and q > 0 and max_x > 0 and max_y > 0 and x_bound > 0 and mu_max > 0):
        return "bad parameters (rho, r, q, max_x, max_y, x_bound, mu_max > 0)"
    if not integral(sqp, 1, 1000):
        return "1 <= max_sqp_iter <= 1000, an integer"
    if not integral(start, 0, 1):
        return "start 0 or 1"
    if not integral(rnd, -1, 15):
        return "-1 <= round_decimals <= 15, an integer"
    if not integral(admm, 0, 2 ** 30):
        return "max_admm_iter >= 0 (at most 2^30), an integer"
    return None


def tenant_pack(items, slots, n_ref, update_lamb_ij=0, t_step=0, loop=False):
    """The blob piadmm_obca_tenant_export writes for the scenarios `slots`, from the plan's
    piadmm_obca_plan_get items (name -> array over all n scenarios): STATE, STATE_PREV, CTRL,
    CTRL_PREV, X, LAMBDA, PRIMAL, DUAL, PRIMAL_THRES, DUAL_THRES, PAR, REF, ITERS, STOP, CONVERGE, PROB,
    STATUS_MASK; with a law DUAL_S, DUAL_D, DUAL_S_PREV, DUAL_D_PREV and DUAL_PAR; with the order WORK;
    with a clock CLOCK and WINDOW.  PAR, REF and DUAL_PAR of one row are shared: the row goes into
    every record.  Without CLOCK the record's clock is (t_step, n_ref, 1) and its window the 8
    reference rows at t_step (zeros past the end).  With loop=True the loop section and the header's
    words 11-14: LOOP_PLANT, LOOP_TAU, LOOP_STREAMS and LOOP_SEED (seed, k0, flags), and LOOP_NOISE /
    LOOP_DELAY where the flags say the kind is present (zeros otherwise); a row kind of one row is
    shared.  Returns a uint8 array."""
    slots = [int(s) for s in np.asarray(slots).reshape(-1)]
    m, n_ref = len(slots), int(n_ref)
    law, order, clocked = "DUAL_S" in items, "WORK" in items, "CLOCK" in items
    lay = tenant_layout(n_ref, law, loop)
    flags = int(items["LOOP_SEED"][2]) if loop else 0
    n = np.asarray(items["STATE"]).reshape(-1, PLAN_STATE).shape[0]
    f64 = np.zeros((m, lay["F"]))
    ints = np.zeros((m, TENANT_INTS), np.int32)
    for name, (o, words) in lay["f64"].items():
        if name == "WINDOW" and not clocked:
            ref = np.ascontiguousarray(items["REF"], np.float64).reshape(-1, 2, n_ref, NX)
            for k, s in enumerate(slots):
                if 0 <= t_step and t_step + N_HORZ <= n_ref:
                    f64[k, o:o + words] = ref[s if len(ref) > 1 else 0][:, t_step:t_step + N_HORZ].reshape(-1)
            continue
        if name == "_loop_pad" or (name == "LOOP_NOISE" and not flags & 2) or (name == "LOOP_DELAY" and not flags & 4):
            continue
        if name == "LOOP_STREAMS":
            f64[:, o] = np.ascontiguousarray(items[name], np.int64).reshape(n)[slots].view(np.float64)
            continue
        a = np.ascontiguousarray(items[name], np.float64).reshape(-1, words)
        assert len(a) in (1, n), (name, a.shape)
        for k, s in enumerate(slots):
            f64[k, o:o + words] = a[s if len(a) > 1 else 0]
    for name, (o, words) in lay["ints"].items():
        if name == "WORK" and not order:
            continue
        if name == "CLOCK" and not clocked:
            ints[:, o:o + 3] = (int(t_step), n_ref, 1)
            continue
        a = np.ascontiguousarray(items[name], np.int32).reshape(n, words)
        for k, s in enumerate(slots):
            ints[k, o:o + words] = a[s]
    hdr = np.zeros(TENANT_HEADER // 4, np.int32)
    hdr[:11] = (TENANT_MAGIC, TENANT_ABI, m, n_ref, int(update_lamb_ij), int(law), int(order), lay["F"], TENANT_INTS,
                lay["record_bytes"], TENANT_HEADER)
    if loop:
        seed, k0 = int(items["LOOP_SEED"][0]), int(items["LOOP_SEED"][1])
        hdr[11:15] = np.array([flags, seed & 0xFFFFFFFF, seed >> 32, k0], np.uint32).view(np.int32)
    body = np.concatenate((f64.view(np.uint8).reshape(m, -1), ints.view(np.uint8).reshape(m, -1)), axis=1)
    return np.concatenate((hdr.view(np.uint8), body.reshape(-1)))


def tenant_unpack(blob):
    """The tenants of a blob: dict(m, n_ref, update_lamb_ij, law, order, loop (its flags, 0 without), and
    per field of the record an array over the m tenants -- copies; with the loop also LOOP_SEED = (seed,
    k0, flags) and per record the rows, a tau in [0, DT] and a stream id >= 0 are checked).  ValueError for what piadmm_obca_tenant_import refuses of the
    blob alone: a short or corrupted header, a size that does not follow from it, and per record
    ("row k: ...") a bad parameter row, prob not 0 / 1, a clock with c < 0 or len outside [8, n_ref]."""
    raw = np.frombuffer(blob, np.uint8) if isinstance(blob, (bytes, bytearray, memoryview)) else np.asarray(blob, np.uint8)
    raw = raw.reshape(-1)
    if raw.size < TENANT_HEADER:
        raise ValueError("tenant blob: shorter than its header")
    hdr = raw[:TENANT_HEADER].copy().view(np.int32)
    magic, abi, m, n_ref, ulij, law, order, F, n_int, rec_bytes, hdr_bytes = (int(v) for v in hdr[:11])
    if magic != TENANT_MAGIC:
        raise ValueError("tenant blob: bad magic")
    if abi != TENANT_ABI:
        raise ValueError(f"tenant blob: ABI {abi}, not {TENANT_ABI}")
    loop = int(hdr[11])
    loop_ok = hdr[15] == 0 and ((loop & 1 and not loop & ~7 and hdr[14] >= 0) if loop else not hdr[12:15].any())
    if m < 1 or n_ref < N_HORZ or ulij not in (0, 1) or law not in (0, 1) or order not in (0, 1) or not loop_ok:
        raise ValueError("tenant blob: bad header (counts or flags)")
    lay = tenant_layout(n_ref, bool(law), bool(loop))
    if (F, n_int, rec_bytes, hdr_bytes) != (lay["F"], TENANT_INTS, lay["record_bytes"], TENANT_HEADER):
        raise ValueError("tenant blob: bad header (section sizes)")
    if raw.size != TENANT_HEADER + m * rec_bytes:
        raise ValueError(f"tenant blob: {raw.size} bytes, not the {TENANT_HEADER + m * rec_bytes} of its header (truncated?)")
    body = raw[TENANT_HEADER:].reshape(m, rec_bytes)
    f64 = np.ascontiguousarray(body[:, :8 * F]).view(np.float64).reshape(m, F)
    ints = np.ascontiguousarray(body[:, 8 * F:]).view(np.int32).reshape(m, TENANT_INTS)
    out = dict(m=m, n_ref=n_ref, update_lamb_ij=ulij, law=bool(law), order=bool(order), loop=loop)
    if loop:
        w = hdr[12:15].copy().view(np.uint32).astype(np.uint64)
        out["LOOP_SEED"] = np.array([w[0] | (w[1] << np.uint64(32)), w[2], loop], np.uint64)
    for name, (o, words) in lay["f64"].items():
        if name == "_loop_pad":
            continue
        if name == "LOOP_STREAMS":
            out[name] = f64[:, o].copy().view(np.int64)
            continue
        shape = (2, n_ref, NX) if name == "REF" else _TENANT_SHAPES[name]
        out[name] = f64[:, o:o + words].reshape((m,) + shape).copy()
    for name, (o, words) in lay["ints"].items():
        out[name] = ints[:, o:o + words].reshape((m,) + _TENANT_SHAPES[name]).copy()
    for k in range(m):
        why = _tenant_row_check(out["PAR"][k])
        if why is None and out["PROB"][k] not in (0, 1):
            why = "prob must be 0 or 1"
        c, length = int(out["CLOCK"][k, 0]), int(out["CLOCK"][k, 1])
        if why is None and c < 0:
            why = "c >= 0"
        if why is None and not N_HORZ <= length <= n_ref:
            why = "8 <= len <= n_ref"
        if why is None and loop:
            for kind, check in (("plant", feedback_row_check), ("noise", noise_row_check), ("delay", delay_row_check)):
                bad = check(out["LOOP_" + kind.upper()][k])
                if why is None and bad is not None:
                    why = f"{kind}: {bad}"
            if why is None and not ((out["LOOP_TAU"][k] >= 0.0) & (out["LOOP_TAU"][k] <= DT)).all():
                why = "tau must be in [0, DT]"
            if why is None and out["LOOP_STREAMS"][k] < 0:
                why = "the stream id must be >= 0"
        if why is not None:
            raise ValueError(f"tenant blob: row {k}: {why}")
    return out
