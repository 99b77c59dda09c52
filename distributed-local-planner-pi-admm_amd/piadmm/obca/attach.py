"""What csrc/piadmm_obca_plan_attach.hip attaches to a plan, in NumPy: the PI dual law, the order, the clocks."""
import types

import numpy as np

from .._lib import DUAL_PAR
from .model import N_HORZ, NT, NX, _per_scenario, local_z


# a gains row of the PI anti-windup dual law (piadmm_obca_dual_plan, include/piadmm.h); the rest is zero
DUAL_ROW = ("kP", "kI", "windup_sat", "d_gain", "windup")
_DUAL_DEFAULT = dict(kP=0.0, kI=1.0, windup_sat=0.0, d_gain=0.0, windup=0)


def dual_row(gains):
    """One gains row (DUAL_PAR doubles) from a dict of DUAL_ROW names (absent: kP 0, kI 1,
    windup_sat 0, d_gain 0, windup 0) or from a row."""
    if isinstance(gains, dict):
        assert set(gains) <= set(DUAL_ROW), set(gains) - set(DUAL_ROW)
        row = np.zeros(DUAL_PAR)
        row[:len(DUAL_ROW)] = [float(gains.get(k, _DUAL_DEFAULT[k])) for k in DUAL_ROW]
        return row
    row = np.asarray(gains, np.float64)
    assert row.shape == (DUAL_PAR,), row.shape
    return row


def dual_rows(n, dual):
    """The gains rows of a plan from dual = dict(kP=, kI=, windup_sat=, d_gain=, windup=), each a
    scalar or a length-n sequence: one shared row, or n rows when any is a sequence."""
    assert set(dual) <= set(DUAL_ROW), set(dual) - set(DUAL_ROW)
    ns = types.SimpleNamespace()
    each = _per_scenario(ns, n, **{k: dual.get(k, _DUAL_DEFAULT[k]) for k in DUAL_ROW})
    rows = np.zeros((n, DUAL_PAR))
    for j, k in enumerate(DUAL_ROW):
        rows[:, j] = getattr(ns, k + "_s")
    return np.ascontiguousarray(rows if each else rows[:1])


def lambda_update_pi(bar, S, D, gains, wrote):
    """The PI anti-windup dual law on the consensus error, host restatement of k_plan_dual_pi
    (csrc/piadmm_obca_plan_attach.hip) with the same statements in the same order: for every entry of a
    slot t with wrote[t]
        e = w - Z_bar;  S' = S + kI e + d_gain D;  raw = S' + kP e;
        lam' = windup ? min(sat, max(raw, -sat)) : raw;  D' = windup ? lam' - raw : 0
    with w = [local_x, lamb_ij]; every other slot keeps lamb_bar, S and D.  bar holds the iterate's
    local_x, lamb_ij, the new Z_bar and the old lamb_bar; gains is a dict of DUAL_ROW names or a
    row; wrote 7 booleans.  Returns (bar with the new lamb_bar, S', D', dres): dres[t] = slot t's
    sum |lam' - lam| over its 18 entries, vehicle 0's 9 and then vehicle 1's 9."""
    g = dual_row(gains)
    kP, kI, sat, d_gain, windup = g[0], g[1], g[2], g[3], g[4] != 0.0
    S, D = np.asarray(S, np.float64), np.asarray(D, np.float64)
    lam = np.asarray(bar["lamb_bar"], np.float64)
    wrote = np.asarray(wrote, bool).reshape(NT)
    e = local_z(bar)[:2] - bar["Z_bar"]
    S1 = S + kI * e + d_gain * D
    raw = S1 + kP * e
    lam1 = np.minimum(sat, np.maximum(raw, -sat)) if windup else raw
    D1 = lam1 - raw if windup else np.zeros_like(raw)
    m = wrote[None, :, None]
    lam1, S1, D1 = np.where(m, lam1, lam), np.where(m, S1, S), np.where(m, D1, D)
    dr = np.abs(lam1 - lam)
    dres = np.zeros(NT)
    for v in (0, 1):
        for li in range(9):
            dres = dres + dr[v, :, li]
    out = {k: v.copy() for k, v in bar.items()}
    out["lamb_bar"] = lam1
    return out, S1, D1, dres


def shift_dual(S, D):
    """The receding-horizon shift of the integrator: S and D drop slot 0 and repeat their last
    slot, as `iterate_next_state` shifts lamb_bar."""
    return tuple(np.concatenate((a[:, 1:], a[:, -1:]), axis=1) for a in (np.asarray(S), np.asarray(D)))


# the longest-first order of a plan (piadmm_obca_order_plan, include/piadmm.h): Q and I are compared
# after clamping to ORDER_CLAMP, the 21 bits each has in the device's key
ORDER_CLAMP = (1 << 21) - 1


def plan_order(lst, work):
    """The order k_plan_order (csrc/piadmm_obca_plan_attach.hip) puts a list of scenarios in: by
    work[s] = (Q, I), Q descending, then I descending, then scenario ascending, Q and I clamped to
    [0, ORDER_CLAMP].  A function of the set in `lst` and of `work` (n x 2) alone."""
    lst = np.asarray(lst, np.int64).reshape(-1)
    w = np.clip(np.asarray(work, np.int64).reshape(-1, 2), 0, ORDER_CLAMP)
    idx = np.lexsort((lst, -w[lst, 1], -w[lst, 0]))
    return lst[idx].astype(np.int32)


def plan_work(local_ist, edge_ist):
    """The work record k_plan_work keeps of one iterate: for the m scenarios submitted, (Q, I) =
    (the largest QP step count ist[.][2], the largest SQP iteration count ist[.][1]) over the
    scenario's 2 local (local_ist 2m x 3, record 2k + v) and 7 edge solves (edge_ist m x 7 x 3)."""
    li, ei = np.asarray(local_ist, np.int32), np.asarray(edge_ist, np.int32)
    m = ei.shape[0]
    assert li.shape == (2 * m, 3) and ei.shape == (m, NT, 3), (li.shape, ei.shape)
    both = np.concatenate((li.reshape(m, 2, 3), ei), axis=1)
    return np.ascontiguousarray(np.stack((both[:, :, 2].max(axis=1), both[:, :, 1].max(axis=1)), axis=1), np.int32)


def clock_tick(clock, ran):
    """The tick of k_plan_clock (csrc/piadmm_obca_plan_attach.hip) on the record clock[s] = (c, len, alive),
    n x 3: c += 1 for the scenarios flagged in `ran` (n, 0 / 1: the ones the step ran), then
    alive = (c + 8 <= len).  Returns the new record (int32); the argument stays."""
    out = np.array(clock, np.int32).reshape(-1, 3)
    ran = np.asarray(ran).reshape(-1)
    assert ran.shape == (out.shape[0],), (ran.shape, out.shape)
    out[:, 0] += (ran != 0).astype(np.int32)
    out[:, 2] = out[:, 0] + N_HORZ <= out[:, 1]
    return out


def clock_window(ref, clock):
    """The reference windows k_plan_clock copies: window[s] = ref_s[v][c : c + 8] (n x 2 x 8 x 5)
    of every scenario with clock[s] = (c, len, alive) alive, zeros for the others.  ref: one
    reference for all (2 x n_ref x 5) or one per scenario (n x 2 x n_ref x 5)."""
    clock = np.asarray(clock, np.int32).reshape(-1, 3)
    ref = np.asarray(ref, np.float64)
    n = clock.shape[0]
    ref = np.broadcast_to(ref, (n,) + ref.shape[-3:])
    out = np.zeros((n, 2, N_HORZ, NX))
    for s, (c, _, alive) in enumerate(clock):
        if alive:
            out[s] = ref[s, :, c:c + N_HORZ]
    return out


def clock_rows(n, clock, t_step, n_ref):
    """The n x 2 (c0, len) rows of a planner's clock argument: True is everyone at the plan's step
    over the whole reference (what a NULL clock_init attaches), else the rows themselves."""
    if clock is True:
        return np.tile(np.array([[t_step, n_ref]], np.int32), (n, 1))
    rows = np.ascontiguousarray(clock, np.int32)
    assert rows.shape == (n, 2), rows.shape
    return rows
