"""NumPy restatement of the OBCA-ADMM edge (RSU) step -- TEST INFRASTRUCTURE ONLY.

The slot problem of DESIGN.md section 9 ("The edge step"): one horizon slot of the reference's
edge NLP (optimizer.py:239-328), 18 variables z = [s_0 (5), mu_0 (4), s_1 (5), mu_1 (4)],

    minimise  -z . lamb_bar + rho/2 |w - z|^2                         (:298-307)
    s.t.      A(s_0)' mu_0 + A(s_1)' mu_1 = 0                          (:276-279)
              min_dis <= -b(s_0)' mu_0 - b(s_1)' mu_1 <= g_max         (:280-283)
              |s| <= x_bound, 0 <= mu <= mu_max                        (:285-295, quirk B12)

* `solve_slot` is the SQP of csrc/piadmm_obca_edge.hip, statement by statement (the QP by
  oracle.obca_oracle.gi_qp, the algorithm the kernel's active-set code runs).
* `kkt_residual_edge` is written from the NLP above -- the halfspaces of piadmm.obca.halfspaces'
  closed form in complex arithmetic, differentiated by the complex step -- and not from the SQP's
  analytic derivatives: the independent certificate.
* `edge_step` is the whole edge stage of one record (solve, rounding, lambda_update, the
  dual-residual partials).
* `planner` is the loop of decentralized_overtaking_ADMM.py:18-103 on the CPU for one scenario, the
  local stage by oracle.obca_oracle.solve_local; `OracleBatch` lets piadmm.obca.OBCAPlanner's host
  logic run against the restatements, and `check_planner_structure` ties a run's recorded stages
  together (resubmission, the :87 shift, the hand-over to the next step).
"""
import functools
import math

import numpy as np

from oracle import obca_oracle as O
from piadmm import obca

NE = 18
CONVERGED, MAX_ITER, QP_INFEASIBLE, LINESEARCH_FAIL, HESSIAN_FAIL = 0, 1, 2, 3, 4
WRITES_ITERATE = (CONVERGED, MAX_ITER, LINESEARCH_FAIL)
OPT = O.Options()


class Slot:
    """One slot problem of an edge record."""

    def __init__(self, rec, t):
        d = obca.edge_unpack(rec)
        self.w = np.concatenate([d["local_x"][0, t], d["lamb_ij"][0, t], d["local_x"][1, t], d["lamb_ij"][1, t]])
        self.lb = np.concatenate([d["lamb_bar"][0, t], d["lamb_bar"][1, t]])
        self.rho, self.min_dis, self.g_max = d["rho"], d["min_dis"], d["g_max"]
        self.prob, self.max_iter, self.start, self.round_decimals = d["prob"], d["max_iter"], d["start"], d["round_decimals"]
        one = np.concatenate([d["x_bound"] * np.ones(5), d["mu_max"] * np.ones(4)])
        self.hi = np.concatenate([one, one])
        lo1 = np.concatenate([-d["x_bound"] * np.ones(5), np.zeros(4)])
        self.lo = np.concatenate([lo1, lo1])


class SlotResult:
    def __init__(self, z, y_eq, y_in, y_bnd, status, iters, qp_steps, cost):
        self.z, self.y_eq, self.y_in, self.y_bnd = z, y_eq, y_in, y_bnd
        self.status, self.iters, self.qp_steps, self.cost = status, iters, qp_steps, cost


def cost(p, z):
    return float(-z @ p.lb + 0.5 * p.rho * (p.w - z) @ (p.w - z))


def constraints(z, prob, hess=False):
    """g_eq (2), its Jacobian (2 x 18), g_in, its gradient (18) [and the Hessians] from the
    analytic forms the local oracle uses for (5a)/(5b)."""
    g_eq, Jeq, g_in, gin = np.zeros(2), np.zeros((2, NE)), 0.0, np.zeros(NE)
    Heq, Hin = np.zeros((2, NE, NE)), np.zeros((NE, NE))
    for v in (0, 1):
        s, mu = z[9 * v:9 * v + 5], z[9 * v + 5:9 * v + 9]
        va, ga, Ha = O.ga_eval(s, mu, 0.0, prob)
        vb, Jb, Hb = O.gb_eval(s, mu, np.zeros(2), prob)
        g_eq = g_eq + vb
        Jeq[:, 9 * v:9 * v + 9] = Jb
        g_in += va
        gin[9 * v:9 * v + 9] = ga
        Heq[:, 9 * v:9 * v + 9, 9 * v:9 * v + 9] = Hb
        Hin[9 * v:9 * v + 9, 9 * v:9 * v + 9] = Ha
    if hess:
        return g_eq, Jeq, g_in, gin, Heq, Hin
    return g_eq, Jeq, g_in, gin


def violation(p, z):
    g_eq, _, g_in, _ = constraints(z, p.prob)
    v = abs(g_eq[0]) + abs(g_eq[1])
    v += max(0.0, p.min_dis - g_in) + max(0.0, g_in - p.g_max)
    for j in range(NE):
        v += max(0.0, p.lo[j] - z[j]) + max(0.0, z[j] - p.hi[j])
    return v


def solve_slot(p, opt=OPT, trace=None):
    """The edge SQP.  `trace` (a list, optional) receives one dict per SQP
    iteration that reached the QP or failed the modification: mod = ("none" | "sigma" | "tau" |
    "fail", rung), n_prev (previously active rows that entered Ga), qst (the QP's status), active
    (the inequality rows active at the QP's solution), drops / partial (rows the QP dropped, and
    those of them after a partial step), halvings (of the line search; -1 = none was run).  The
    trace is written only: the result is the same with and without it."""
    z = np.zeros(NE) if p.start == 0 else np.minimum(np.maximum(p.w, p.lo), p.hi)
    y_eq, y_in, y_bnd = np.zeros(2), 0.0, np.zeros(NE)
    mu = 0.0
    qp_total = 0
    prev_act = None
    status, it = MAX_ITER, 0
    for it in range(p.max_iter):
        g_eq, Jeq, g_in, gin, Heq, Hin = constraints(z, p.prob, hess=True)
        gf = -p.lb - p.rho * (p.w - z)
        H = p.rho * np.eye(NE) - y_eq[0] * Heq[0] - y_eq[1] * Heq[1] - y_in * Hin
        # rows: C d >= din; 0/1 the range row, then lower / upper bound per variable
        Cin = np.zeros((2 + 2 * NE, NE))
        din = np.zeros(2 + 2 * NE)
        Cin[0], din[0] = gin, p.min_dis - g_in
        Cin[1], din[1] = -gin, g_in - p.g_max
        for j in range(NE):
            Cin[2 + 2 * j, j], din[2 + 2 * j] = 1.0, p.lo[j] - z[j]
            Cin[3 + 2 * j, j], din[3 + 2 * j] = -1.0, z[j] - p.hi[j]
        Ceq, deq = Jeq, -g_eq
        # Hessian modification: sigma sum a a' over the equality rows and the rows active in the
        # previous QP (normalised), then tau diag(|H_ii|)
        Hm, gm = H, gf
        mod, n_prev = ("none", 0), 0
        if not O._is_pd(Hm):
            n_prev = len(prev_act) if prev_act is not None else 0
            rows = [Ceq[0], Ceq[1]] + ([Cin[k] for k in prev_act] if prev_act is not None else [])
            rhs = [deq[0], deq[1]] + ([din[k] for k in prev_act] if prev_act is not None else [])
            Ga, ga_ = np.zeros((NE, NE)), np.zeros(NE)
            for a, b in zip(rows, rhs):
                nrm = max(math.sqrt(float(a @ a)), 1e-300)
                an = a / nrm
                Ga += np.outer(an, an)
                ga_ += an * (b / nrm)
            hmax = float(np.max(np.abs(np.diag(H))))
            sig = 1e-4 * hmax
            for k in range(8):
                Hm = H + sig * Ga
                gm = gf - sig * ga_
                mod = ("sigma", k)
                if O._is_pd(Hm):
                    break
                sig *= 10.0
        if not O._is_pd(Hm):
            Dg = np.diag(np.maximum(np.abs(np.diag(Hm)), 1e-12))
            H0, tau = Hm, 0.0
            for k in range(16):
                tau = 1e-6 if tau == 0.0 else tau * 10.0
                Hm = H0 + tau * Dg
                mod = ("tau", k)
                if O._is_pd(Hm):
                    break
            else:
                status = HESSIAN_FAIL
                if trace is not None:
                    trace.append(dict(mod=("fail", 16), n_prev=n_prev, qst=-1, active=(), drops=0, partial=0, halvings=-1))
                break
        count = {} if trace is not None else None
        d, ueq, uin, qst, qsteps = O.gi_qp(Hm, gm, Ceq, deq, Cin, din, count=count)
        qp_total += qsteps
        if trace is not None:
            rec_ = dict(mod=mod, n_prev=n_prev, qst=qst, active=tuple(int(c) for c in np.nonzero(uin > 0)[0]) if qst == 0 else (),
                        drops=count.get("drops", 0), partial=count.get("partial", 0), halvings=-1)
            trace.append(rec_)
        prev_act = np.nonzero(uin > 0)[0] if qst == 0 else None
        if qst != 0:
            status = QP_INFEASIBLE if qst == 2 else MAX_ITER
            break
        ny_eq = ueq
        ny_in = uin[0] - uin[1]
        ny_bnd = uin[2::2] - uin[3::2]
        viol = violation(p, z)
        step = float(np.max(np.abs(d)))
        if step <= opt.tol_step and viol <= opt.tol_feas:
            z = z + d
            y_eq, y_in, y_bnd = ny_eq, ny_in, ny_bnd
            status = CONVERGED
            break
        mmax = max(float(np.max(np.abs(ny_eq))), abs(ny_in), float(np.max(np.abs(ny_bnd))))
        mu = max(mu, 1.01 * mmax + 1e-6)
        phi0 = cost(p, z) + mu * viol
        D = float(gf @ d) - mu * viol
        alpha, ok = 1.0, False
        for k in range(opt.max_halvings + 1):
            zn = z + alpha * d
            phi = cost(p, zn) + mu * violation(p, zn)
            if trace is not None:
                rec_["halvings"] = k
            if phi <= phi0 + opt.armijo * alpha * D:
                ok = True
                break
            alpha *= 0.5
        if not ok:
            status = LINESEARCH_FAIL
            break
        z = zn
        y_eq = y_eq + alpha * (ny_eq - y_eq)
        y_in = y_in + alpha * (ny_in - y_in)
        y_bnd = y_bnd + alpha * (ny_bnd - y_bnd)
    return SlotResult(z, y_eq, y_in, y_bnd, status, it + 1, qp_total, cost(p, z))


@functools.lru_cache(maxsize=None)
def _solve(raw, t):
    p = Slot(np.frombuffer(raw, np.float64), t)
    tr = []
    r = solve_slot(p, trace=tr)
    r.trace = tr
    return p, r


def solve_record(rec):
    """[(Slot, SlotResult)] x 7 of one edge record (each distinct record solved once per process);
    SlotResult.trace is solve_slot's trace."""
    raw = np.ascontiguousarray(rec, np.float64).tobytes()
    return [_solve(raw, t) for t in range(obca.NT)]


def around(x, d):
    """np.round semantics, the QP path's rule: rint(x 10^d) / 10^d; d < 0 = off."""
    if d < 0:
        return np.array(x, np.float64)
    f = 10.0 ** d
    return np.rint(np.asarray(x) * f) / f


def edge_step(rec):
    """The whole edge step of one record from the restatement: dict of Z, Z_bar, lamb_bar (new),
    dres (7), status (7), in the layout of OBCAEdgeResult."""
    d = obca.edge_unpack(rec)
    Z = np.zeros((2, obca.NT, 9))
    st = np.zeros(obca.NT, int)
    for t, (p, r) in enumerate(solve_record(rec)):
        Z[0, t], Z[1, t] = r.z[:9], r.z[9:]
        st[t] = r.status
    Zb = around(Z, d["round_decimals"])
    w = np.concatenate([d["local_x"], d["lamb_ij"]], axis=2)
    lbn = d["lamb_bar"].copy()
    dres = np.zeros(obca.NT)
    for t in range(obca.NT):
        if st[t] in WRITES_ITERATE:
            lbn[:, t] = d["lamb_bar"][:, t] + d["rho"] * (w[:, t] - Zb[:, t])
            dres[t] = np.abs(lbn[:, t] - d["lamb_bar"][:, t]).sum()
    return dict(Z=Z, Z_bar=Zb, lamb_bar=lbn, dres=dres, status=st)


# ---------------------------------------------------------------------------------------------
# the independent certificate
# ---------------------------------------------------------------------------------------------
def _halfspaces_c(s, prob):
    """piadmm.obca.halfspaces' closed form (util.py:12-101) on complex input."""
    x, y, v, th = s[0], s[1], s[2], s[3]
    c, sn = np.cos(th), np.sin(th)
    e, n = np.array([c, sn]), np.array([-sn, c])
    if prob:
        A = np.stack([e, n, -e, -n])
        sig = math.sqrt(obca.DELAY_PROB / (1.0 - obca.DELAY_PROB))
        dl = np.array([obca.AVG_DELAY * v * c + sig * (obca.VAR_DELAY * v * c) ** 2,
                       obca.AVG_DELAY * v * sn + sig * (obca.VAR_DELAY * v * sn) ** 2])
    else:
        A = np.stack([e, -n, -e, n])
        dl = np.zeros(2, complex)
    b0 = np.array([obca.LENGTH / 2, obca.WIDTH / 2, obca.LENGTH / 2, obca.WIDTH / 2])
    return A, b0 + A @ (np.array([x, y]) + dl)


def _g_c(z, prob):
    A0, b0 = _halfspaces_c(z[0:5], prob)
    A1, b1 = _halfspaces_c(z[9:14], prob)
    m0, m1 = z[5:9], z[14:18]
    g_eq = A0.T @ m0 + A1.T @ m1
    g_in = -(b0 @ m0) - (b1 @ m1)
    return np.array([g_eq[0], g_eq[1], g_in])


def kkt_residual_edge(p, z, y_eq, y_in, y_bnd):
    """First-order conditions of the slot NLP at z with multipliers (Lagrangian
    f - y_eq.g_eq - y_in g_in - y_bnd.z; y > 0 at a lower bound, < 0 at an upper): max
    |stationarity|, max infeasibility, max complementarity / sign error.  The constraint values
    agree with piadmm.obca.halfspaces (asserted); gradients are complex-step derivatives."""
    z = np.asarray(z, np.float64)
    g = _g_c(z.astype(complex), p.prob).real
    A0, b0 = obca.halfspaces(z[0:5], p.prob)
    A1, b1 = obca.halfspaces(z[9:14], p.prob)
    ref = np.concatenate([A0.T @ z[5:9] + A1.T @ z[14:18], [-b0 @ z[5:9] - b1 @ z[14:18]]])
    assert np.allclose(g, ref, rtol=1e-12, atol=1e-12)
    J = np.zeros((3, NE))
    h = 1e-30
    for j in range(NE):
        zc = z.astype(complex)
        zc[j] += 1j * h
        J[:, j] = _g_c(zc, p.prob).imag / h
    gf = -p.lb - p.rho * (p.w - z)
    r = gf - y_eq[0] * J[0] - y_eq[1] * J[1] - y_in * J[2] - y_bnd
    stat = float(np.abs(r).max())
    feas = max(abs(g[0]), abs(g[1]), p.min_dis - g[2], g[2] - p.g_max, float((p.lo - z).max()), float((z - p.hi).max()), 0.0)

    def sgn_err(y, val, lo, hi):
        e = 0.0
        if y > 0:
            e = max(e, min(y, abs(val - lo)))
        if y < 0:
            e = max(e, min(-y, abs(hi - val)))
        return e

    comp = sgn_err(y_in, g[2], p.min_dis, p.g_max)
    for j in range(NE):
        comp = max(comp, sgn_err(y_bnd[j], z[j], p.lo[j], p.hi[j]))
    gscale = 1.0 + float(np.abs(gf).max())
    return dict(stat=stat, feas=feas, comp=comp, gscale=gscale)


# ---------------------------------------------------------------------------------------------
# case sets
# ---------------------------------------------------------------------------------------------
T_STEPS = (2, 8, 14, 20, 29, 35)
PRESS = 0.3


@functools.lru_cache(maxsize=None)
def _sets():
    import _obca_cases as C
    out = {}
    cons = []
    for prob in (1, 0):
        for ts in T_STEPS:
            cons.append(obca.edge_record(obca.seeded_bar_state(ts, prob), prob=prob))
    out["consistent"] = np.stack(cons)
    # the two vehicles' independently solved local plans and their own Lambda (the records of
    # _obca_cases.exchanged), vehicle 0 from one bar_state variant and vehicle 1 from the next: each
    # plan satisfies its own (5b) against a different exchanged direction, so A_0' mu_0 + A_1' mu_1
    # is not zero at w and the edge equality has to move the pair
    ex = C.exchanged()
    sols = C.oracle(ex)
    keys = []
    for prob in (1, 0):
        for ts in C.EXCHANGED_T:
            for var in C.VARIANTS:
                idx = [C.KEYS.index((prob, ts, veh, var)) for veh in (0, 1)]
                if all(r.status == O.CONVERGED for _, r in C.oracle([C.BASE[i] for i in idx])):
                    keys += [(prob, ts, var, 0), (prob, ts, var, 1)]
    assert len(keys) == len(ex)
    exch = []
    for prob in (1, 0):
        for ts in C.EXCHANGED_T:
            for k, var in enumerate(C.VARIANTS):
                var1 = C.VARIANTS[(k + 1) % 3]
                if (prob, ts, var, 0) not in keys or (prob, ts, var1, 1) not in keys:
                    continue
                pick = [keys.index((prob, ts, var, 0)), keys.index((prob, ts, var1, 1))]
                if any(sols[i][1].status != O.CONVERGED for i in pick):
                    continue
                fullx = [np.concatenate([sols[i][1].X[1:], sols[i][1].Lam], axis=1) for i in pick]
                bar = obca.bar_state_update(obca.create_bar_state(), fullx, prob=prob)
                bar["lamb_ij"] = np.stack([f[:, 5:] for f in fullx])
                bar["lamb_bar"] = np.stack([obca.unpack(ex[i])["lamb_bar"] for i in pick])
                exch.append(obca.edge_record(bar, prob=prob))
    out["exchanged"] = np.stack(exch)
    # vehicle 0 shifted toward vehicle 1 along the centre line until the range row is short of
    # min_dis by PRESS at w (the row falls by alpha = 0.9 per metre of approach)
    pres = []
    for prob in (1, 0):
        for ts in (8, 14, 20):
            bar = obca.seeded_bar_state(ts, prob)
            for t in range(obca.NT):
                zw = np.concatenate([bar["local_x"][0, t], bar["lamb_ij"][0, t], bar["local_x"][1, t], bar["lamb_ij"][1, t]])
                g_in = constraints(zw, prob)[2]
                dvec = bar["local_x"][1, t, :2] - bar["local_x"][0, t, :2]
                bar["local_x"][0, t, :2] += dvec / np.linalg.norm(dvec) * (g_in - 0.1 + PRESS) / 0.9
            pres.append(obca.edge_record(bar, prob=prob))
    out["pressed"] = np.stack(pres)
    bnd = []
    for prob in (1, 0):
        for ts in (8, 20):
            bnd.append(obca.edge_record(obca.seeded_bar_state(ts, prob), prob=prob, mu_max=0.5))
            bnd.append(obca.edge_record(obca.seeded_bar_state(ts, prob), prob=prob, x_bound=15.0))
    out["bounds"] = np.stack(bnd)
    tr = []
    for k in (1, 2):
        for rec in out["exchanged"][:6]:
            r = rec.copy()
            r[obca._E_PAR + 3] = float(k)
            tr.append(r)
    out["truncated"] = np.stack(tr)
    zs = []
    for rec in list(out["consistent"][:4]) + list(out["exchanged"][:4]):
        r = rec.copy()
        r[obca._E_PAR + 5] = 0.0
        zs.append(r)
    out["zero_start"] = np.stack(zs)
    return out


SET_NAMES = ("consistent", "exchanged", "pressed", "bounds", "truncated", "zero_start")
CERTIFIED = ("consistent", "exchanged", "pressed", "bounds")


def case_set(name):
    return np.ascontiguousarray(_sets()[name].copy())


# ---------------------------------------------------------------------------------------------
# the planner loop on the CPU (decentralized_overtaking_ADMM.py:18-103), one scenario, written
# from the script line by line; the local stage by oracle.obca_oracle.solve_local
# ---------------------------------------------------------------------------------------------
def _copy(bar):
    return {k: v.copy() for k, v in bar.items()}


def planner(n_steps, prob, t_step0, max_admm_iter=50, primal_thres=0.01, dual_thres=0.01, rho=1.0, min_dis=0.1,
            round_decimals=4, update_lamb_ij=0, max_iter=60):
    """dict of state_record, iter_num_record, lambda_record, shift_in (the bar_state each step's
    :87 shifted) and status (every local / edge status met)."""
    refs = obca.ref_traj_gen()
    init_state = np.stack([obca.executed_path(v, t_step0 * obca.DT) for v in (0, 1)])
    out = dict(state_record=[init_state], iter_num_record=[], lambda_record=[], shift_in=[], status=[])
    bar_state_prev = obca.seeded_bar_state(t_step0, prob)                     # :30 (a runnable start)
    for t_step in range(t_step0, t_step0 + n_steps):                          # :31
        bar_state = _copy(bar_state_prev)                                     # :37
        bar_ctrl_prev = np.zeros((2, 14))                                     # :38
        i_iter = 0
        while True:
            i_iter += 1                                                       # :41
            sol = []
            for i_veh in (0, 1):                                              # :49-63
                rec = obca.local_record(bar_state, i_veh, t_step, init_state[i_veh], refs, rho=rho, min_dis=min_dis,
                                        prob=prob, max_iter=max_iter)
                p, opt = O.from_record(rec)
                sol.append(O.solve_local(p, opt))
            bar_x = [r.X for r in sol]
            bar_ctrl = np.stack([np.append(r.U[:, 0], r.U[:, 1]) for r in sol])   # :61
            bar_fullx = [np.concatenate([r.X[1:], r.Lam], axis=1) for r in sol]
            bar_state = obca.bar_state_update(bar_state, bar_fullx, prob=prob)    # :66
            if update_lamb_ij:                                                # :220, when not commented out
                bar_state["lamb_ij"] = np.stack([f[:, 5:] for f in bar_fullx])
            st = edge_step(obca.edge_record(bar_state, rho=rho, min_dis=min_dis, prob=prob, max_iter=max_iter,
                                            round_decimals=round_decimals))   # :71-79
            bar_state["Z_bar"], bar_state["lamb_bar"] = st["Z_bar"], st["lamb_bar"]
            out["status"].append(([r.status for r in sol], st["status"]))
            primal_res = np.abs(bar_ctrl - bar_ctrl_prev).sum()               # :82-83
            dual_res = np.abs(bar_state["lamb_bar"] - bar_state_prev["lamb_bar"]).sum()   # :84-85
            if (primal_res <= primal_thres and dual_res <= dual_thres) or i_iter > max_admm_iter:   # :86
                out["shift_in"].append(_copy(bar_state_prev))
                bar_state_prev = obca.iterate_next_state(bar_state_prev)      # :87 (quirk B16)
                break
            bar_state_prev = _copy(bar_state)                                 # :94
            bar_ctrl_prev = bar_ctrl.copy()                                   # :96
        init_state = np.stack([bar_x[0][1], bar_x[1][1]])                     # :99
        out["state_record"].append(init_state)
        out["iter_num_record"].append(i_iter)
        out["lambda_record"].append(bar_state["lamb_bar"].copy())             # :103
    return out


class OracleBatch:
    """The two launches of piadmm.obca.OBCABatch answered by the restatements: OBCAPlanner's host
    logic (loop control, exchange, shift, records) runs on the CPU against it."""

    def solve(self, recs):
        import _obca_cases as C
        out = np.zeros((len(recs), obca.OUT))
        ist = np.zeros((len(recs), 3), np.int32)
        for k, (_, r) in enumerate(C.oracle(recs)):
            out[k, :40], out[k, 40:54], out[k, 54:82] = r.X.ravel(), r.U.ravel(), r.Lam.ravel()
            ist[k] = (r.status, r.iters, r.qp_iters)
        return obca.OBCAResult(out, ist)

    def solve_edge(self, recs):
        out = np.zeros((len(recs), obca.EDGE_OUT))
        ist = np.zeros((len(recs), obca.NT, 3), np.int32)
        for k, rec in enumerate(recs):
            st = edge_step(rec)
            out[k, obca._EO_Z:obca._EO_Z + 126] = st["Z"].ravel()
            out[k, obca._EO_ZB:obca._EO_ZB + 126] = st["Z_bar"].ravel()
            out[k, obca._EO_LBN:obca._EO_LBN + 126] = st["lamb_bar"].ravel()
            out[k, obca._EO_DRES:obca._EO_DRES + 7] = st["dres"]
            ist[k, :, 0] = st["status"]
        return obca.OBCAEdgeResult(out, ist)


def check_planner_structure(pl, stages, rec, t_step0):
    """What ties the recorded stages of an OBCAPlanner run together, from the stages alone:
    * a scenario that stopped is absent from every later launch of the step;
    * the bar_state that :87 shifts is the one of the PREVIOUS iterate (quirk B16): the state after
      the edge stage of iterate i - 1 (A, b, local_x, lamb_ij of that exchange output, Z_bar and
      lamb_bar of that edge output), or the start-of-step state when the scenario stopped at
      iterate 1 -- and not the last iterate's state;
    * init_state = X[1] of the scenario's last local solve (:99);
    * the next step's first local records are built from the shifted state and init_state.
    Returns the stop iterate of every scenario per step (steps x scenarios)."""
    n = pl.n
    start = [obca.seeded_bar_state(t_step0, p) for p in pl.prob]
    init = [np.stack([obca.executed_path(v, t_step0 * obca.DT) for v in (0, 1)]) for _ in range(n)]
    after = [dict() for _ in range(n)]        # scenario -> {iterate: bar_state after its edge stage}
    stopped, stop_iter, exch, scen, i_iter = set(), {}, None, None, 0
    all_iters = []
    for name, inp, outp in stages:
        if name == "local":
            scen, i_iter = list(inp["scenarios"]), inp["i_iter"]
            assert not stopped & set(scen), (stopped, scen)        # a stopped scenario is not resubmitted
            assert len(inp["recs"]) == 2 * len(scen)
            if i_iter == 1:
                assert scen == list(range(n))
                want = np.stack([obca.local_record(start[s], v, inp["t_step"], init[s][v], pl.ref_traj, rho=pl.rho,
                                                   min_dis=pl.min_dis, prob=pl.prob[s], max_iter=pl.max_iter)
                                 for s in scen for v in (0, 1)])
                np.testing.assert_array_equal(inp["recs"], want)
        elif name == "exchange":
            assert list(inp["scenarios"]) == scen
            exch = outp["bar"]
        elif name == "edge":
            for k, s in enumerate(scen):
                b = _copy(exch[k])
                b["Z_bar"], b["lamb_bar"] = outp["result"].Z_bar[k].copy(), outp["result"].lamb_bar[k].copy()
                after[s][i_iter] = b
        elif name == "residual":
            for k, s in enumerate(scen):
                if outp["stop"][k]:
                    stopped.add(s)
                    stop_iter[s] = i_iter
        elif name == "shift":
            assert stopped == set(range(n))
            np.testing.assert_array_equal(inp["iters"], [stop_iter[s] for s in range(n)])
            for s in range(n):
                i = stop_iter[s]
                want = start[s] if i == 1 else after[s][i - 1]
                last = after[s][i]
                for key in want:
                    np.testing.assert_array_equal(inp["bar_prev"][s][key], want[key], err_msg=f"{key} {s}")
                assert not np.array_equal(inp["bar_prev"][s]["lamb_bar"], last["lamb_bar"])
                assert not np.array_equal(inp["bar_prev"][s]["Z_bar"], last["Z_bar"])
                nxt = obca.iterate_next_state(want)
                for key in nxt:
                    np.testing.assert_array_equal(outp["bar_next"][s][key], nxt[key])
                np.testing.assert_array_equal(outp["init_state"][s], np.stack([inp["X"][s][0][1], inp["X"][s][1][1]]))
            start = [_copy(b) for b in outp["bar_next"]]
            init = [x.copy() for x in outp["init_state"]]
            all_iters.append([stop_iter[s] for s in range(n)])
            after = [dict() for _ in range(n)]
            stopped, stop_iter = set(), {}
    np.testing.assert_array_equal(np.asarray(rec.iter_num_record), np.asarray(all_iters))
    return np.asarray(all_iters)
