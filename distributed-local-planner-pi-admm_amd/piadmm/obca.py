"""OBCA local subproblem on the GPU: batched SQP (csrc/piadmm_obca.hip) behind
``piadmm_obca_solve`` (include/piadmm.h).

Mirrors the vehicle side of ``OBCAOptimizer`` (Distributed_planner/decentralized/optimizer.py):
``local_initialize`` + ``local_build_model`` + ``local_generate_constrain`` +
``local_generate_variable`` + ``local_generate_object`` + ``local_solve`` (:40-201) become one
record per (vehicle, ADMM iterate) and one batched call; ``bar_state`` keeps the reference's
arrays (``Z_bar``, ``A``, ``b``, ``lamb_bar``, ``lamb_ij``, ``local_x``, :351-373) and
``iterate_next_state`` (:337-344) shifts them.

Record layout (float64, ``REC`` per problem) -- what the reference's local NLP reads:
  init 5 | ref 8x5 (ref_traj[veh][t_step + k], also the initial X guess) | A_o 7x4x2 | b_o 7x4 |
  lamb_ij_o 7x4 (the other vehicle's bar_state slots) | lamb_bar 7x9 | Z_bar 7x9 |
  rho, min_dis, max_x, max_y, r, q, prob, max_iter | pad
Output (float64, ``OUT`` per problem): X 8x5 | U 7x2 | Lambda 7x4 | y_a 7 | y_b 7x2 | y_n 7 |
  y_x 7x5 | pi 7x5 | y_u 14 | y_l 28 | cost | pad;  status / SQP iterations / QP steps (int32 x 3).
"""
from __future__ import annotations

import ctypes
import dataclasses
import math

import numpy as np

N_HORZ, NX, NU, NL = 8, 5, 2, 4
NT = N_HORZ - 1
REC = 296
OUT = 224
_O_INIT, _O_REF, _O_AO, _O_BO, _O_LIJ, _O_LB, _O_ZB, _O_PAR = 0, 5, 45, 101, 129, 157, 220, 283

STATUS = {0: "converged", 1: "max_iter", 2: "qp_infeasible", 3: "linesearch_fail", 4: "hessian_fail"}

# VehicleConfig (veh_config.py:7-27)
LENGTH, WIDTH = 3.5, 2.0
DT, T_PERIOD = 0.1, 5.0
AVG_DELAY, VAR_DELAY, DELAY_PROB = 0.05, 0.025, 0.95


@dataclasses.dataclass(frozen=True)
class OvertakeSpec:
    """One overtaking manoeuvre: vehicle 0 at v0 m/s from x = 0, vehicle 1 at v1 m/s from x = gap;
    vehicle 0 changes to y = +lane between t_out and t_out + ramp (s) and back between t_back and
    t_back + ramp.  The defaults are the reference's scenario (veh_config.py:30-47) and the
    manoeuvre `executed_path` always drove.  v0 above 20 (the vehicle's max_v) makes the local NLP
    infeasible."""
    v0: float = 20.0
    v1: float = 10.0
    gap: float = 20.0
    lane: float = 4.0
    t_out: float = 0.2
    t_back: float = 3.0
    ramp: float = 0.6


def _spec(spec):
    """`spec` with float fields; None is the default manoeuvre."""
    if spec is None:
        return OvertakeSpec()
    return OvertakeSpec(*(float(getattr(spec, f.name)) for f in dataclasses.fields(OvertakeSpec)))


def ref_traj_gen(spec=None):
    """The overtaking scenario's references (veh_config.py:30-47)."""
    sp = _spec(spec)
    n = int(T_PERIOD / DT) + 1
    out = []
    for v, x0 in ((sp.v0, 0.0), (sp.v1, sp.gap)):
        x = np.linspace(x0, x0 + v * T_PERIOD, n)
        out.append(np.vstack((x, np.zeros_like(x), v * np.ones_like(x), np.zeros_like(x), np.zeros_like(x))).T)
    return out


def halfspaces(state, prob):
    """(A, b) of a vehicle at `state` -- the halfspaces bar_state_update exchanges
    (optimizer.py:205-222 via util.py:12-101)."""
    x, y, v, th = state[0], state[1], state[2], state[3]
    c, s = math.cos(th), math.sin(th)
    e, n = np.array([c, s]), np.array([-s, c])
    if prob:
        A = np.vstack([e, n, -e, -n])
        sig = math.sqrt(DELAY_PROB / (1.0 - DELAY_PROB))
        d = np.array([AVG_DELAY * v * c + sig * (VAR_DELAY * v * c) ** 2,
                      AVG_DELAY * v * s + sig * (VAR_DELAY * v * s) ** 2])
    else:
        A = np.vstack([e, -n, -e, n])
        d = np.zeros(2)
    b0 = np.array([LENGTH / 2, WIDTH / 2, LENGTH / 2, WIDTH / 2])
    return A, b0 + A @ (np.array([x, y]) + d)


def vehicle_box(state, prob=0, tight=False):
    """(cx, cy, cos, sin) of a vehicle's rectangle at `state` (generate_vehicle_vertices,
    util.py:34-42).  tight with prob: the centre moved as `halfspaces` moves it (the delay-tightened
    box of compute_square_halfspaces_ca_prob, util.py:83-99); the products in the order
    csrc/piadmm_obca_plan.hip forms them."""
    x, y, v, th = float(state[0]), float(state[1]), float(state[2]), float(state[3])
    c, s = math.cos(th), math.sin(th)
    if tight and prob:
        sig = math.sqrt(DELAY_PROB / (1.0 - DELAY_PROB))
        qx, qy = VAR_DELAY * v * c, VAR_DELAY * v * s
        dx = AVG_DELAY * v * c + sig * (qx * qx)
        dy = AVG_DELAY * v * s + sig * (qy * qy)
        x, y = x + dx, y + dy
    return x, y, c, s


def _box_vertex(box, i):
    """Vertex i of a box: centre + sl e + sw n with the signs (+, +), (+, -), (-, -), (-, +)."""
    cx, cy, c, s = box
    sl = LENGTH / 2 if i < 2 else -(LENGTH / 2)
    sw = WIDTH / 2 if i in (0, 3) else -(WIDTH / 2)
    return cx + sl * c - sw * s, cy + sl * s + sw * c


def box_clearance(box0, box1):
    """(distance, gap) of two boxes of `vehicle_box`: gap is the largest separation along the 4
    edge normals (SAT, exact for two rectangles); the distance is 0 when gap <= 0, else the minimum
    of the 32 vertex-to-edge distances.  The statements of k_plan_clearance, one lane at a time."""
    boxes = (box0, box1)
    hl, hw = LENGTH / 2, WIDTH / 2
    gap, dist = -math.inf, math.inf
    for dr in (0, 1):
        a, o = boxes[dr], boxes[1 - dr]
        ax, ay, ca, sa = a
        ox, oy, co, so = o
        for vi in range(4):
            px, py = _box_vertex(a, vi)
            for ej in range(4):
                e0x, e0y = _box_vertex(o, ej)
                e1x, e1y = _box_vertex(o, (ej + 1) & 3)
                abx, aby, apx, apy = e1x - e0x, e1y - e0y, px - e0x, py - e0y
                t = (apx * abx + apy * aby) / (abx * abx + aby * aby)
                t = min(max(t, 0.0), 1.0)
                rx, ry = apx - t * abx, apy - t * aby
                dist = min(dist, math.sqrt(rx * rx + ry * ry))
                lateral = ej & 1
                ux, uy = (-so, co) if lateral else (co, so)
                cdx, cdy = ax - ox, ay - oy
                pc = abs(cdx * ux + cdy * uy)
                pe, pn = abs(ca * ux + sa * uy), abs(ca * uy - sa * ux)
                gap = max(gap, pc - ((hw if lateral else hl) + (hl * pe + hw * pn)))
    return (dist if gap > 0.0 else 0.0), gap


def clearance(state_pair, prob):
    """(plain, tight): the minimum distance between the two vehicles' rectangles at the state pair
    (2 x 5), and between their delay-tightened boxes (prob = 0: the plain value twice).  Host
    restatement of k_plan_clearance (csrc/piadmm_obca_plan_trace.hip)."""
    sp = np.asarray(state_pair, np.float64).reshape(2, NX)
    plain = box_clearance(vehicle_box(sp[0]), vehicle_box(sp[1]))[0]
    tight = box_clearance(vehicle_box(sp[0], prob, True), vehicle_box(sp[1], prob, True))[0]
    return plain, tight


def separating_duals(A_o, u, alpha):
    """lamb_ij of the other vehicle with A_o' lamb_ij = alpha * u (u a unit vector pointing from
    the other vehicle towards this one), the smallest such non-negative vector."""
    lam = np.zeros(4)
    # rows come in opposite pairs (0, 2) and (1, 3)
    for r0, r1 in ((0, 2), (1, 3)):
        comp = float(A_o[r0] @ u)
        lam[r0] = alpha * max(comp, 0.0)
        lam[r1] = alpha * max(-comp, 0.0)
    return lam


def pack(init, ref, A_o, b_o, lamb_ij_o, lamb_bar, Z_bar, rho=1.0, min_dis=0.1, max_x=150.0, max_y=20.0,
         r=1e4, q=1e5, prob=1, max_iter=60):
    rec = np.zeros(REC)
    rec[_O_INIT:_O_INIT + 5] = init
    rec[_O_REF:_O_REF + 40] = np.asarray(ref, np.float64).ravel()
    rec[_O_AO:_O_AO + 56] = np.asarray(A_o, np.float64).ravel()
    rec[_O_BO:_O_BO + 28] = np.asarray(b_o, np.float64).ravel()
    rec[_O_LIJ:_O_LIJ + 28] = np.asarray(lamb_ij_o, np.float64).ravel()
    rec[_O_LB:_O_LB + 63] = np.asarray(lamb_bar, np.float64).ravel()
    rec[_O_ZB:_O_ZB + 63] = np.asarray(Z_bar, np.float64).ravel()
    rec[_O_PAR:_O_PAR + 8] = [rho, min_dis, max_x, max_y, r, q, float(prob), float(max_iter)]
    return rec


def unpack(rec):
    """dict of the record's fields (the oracle builds its LocalProblem from this)."""
    rec = np.asarray(rec, np.float64)
    par = rec[_O_PAR:_O_PAR + 8]
    return dict(init=rec[_O_INIT:_O_INIT + 5].copy(), ref=rec[_O_REF:_O_REF + 40].reshape(8, 5).copy(),
                A_o=rec[_O_AO:_O_AO + 56].reshape(7, 4, 2).copy(), b_o=rec[_O_BO:_O_BO + 28].reshape(7, 4).copy(),
                lamb_ij_o=rec[_O_LIJ:_O_LIJ + 28].reshape(7, 4).copy(),
                lamb_bar=rec[_O_LB:_O_LB + 63].reshape(7, 9).copy(), Z_bar=rec[_O_ZB:_O_ZB + 63].reshape(7, 9).copy(),
                rho=par[0], min_dis=par[1], max_x=par[2], max_y=par[3], r=par[4], q=par[5], prob=int(par[6]),
                max_iter=int(par[7]))


def executed_path(veh, tau, spec=None):
    """Collision-free executed states of the overtaking manoeuvre at time tau (s): vehicle 1 on
    its reference (veh_config.py:41-45); vehicle 0 at 20 m/s changing to y = +lane between
    0.2 s and 0.8 s and back between 3.0 s and 3.6 s (smoothstep profiles, heading = path
    tangent) -- or the speeds, gap, lane and times of `spec`.  The reference's own references run
    vehicle 0 through vehicle 1; these are the states a converged run would exchange."""
    sp = _spec(spec)
    if veh == 1:
        return np.array([sp.gap + sp.v1 * tau, 0.0, sp.v1, 0.0, 0.0])
    lane = sp.lane

    def sstep(u):
        u = min(max(u, 0.0), 1.0)
        return u * u * (3 - 2 * u), 6 * u * (1 - u)

    a, da = sstep((tau - sp.t_out) / sp.ramp)
    b, db = sstep((tau - sp.t_back) / sp.ramp)
    y = lane * (a - b)
    dy = lane * (da - db) / sp.ramp
    return np.array([sp.v0 * tau, y, sp.v0, math.atan2(dy, sp.v0), 0.0])


def overtaking_problem(t_step, veh, variant="initial", prob=1, seed=0, alpha=0.9, spec=None):
    """One local problem of the two-vehicle overtaking scenario (decentralized_overtaking_ADMM.py:
    22-42: VehicleConfig references, N_horz 8, min_dis 0.1, max_x 150, max_y 20, rho 1).

    ref = the vehicle's reference window ref_traj[veh][t_step:t_step+8] (local_initialize,
    optimizer.py:51-53); init = its executed state (`executed_path`); the other vehicle's
    bar_state slots are the halfspaces of ITS executed states (what bar_state_update exchanges,
    :205-222) and duals lamb_ij separating the two boxes along the centre-to-centre direction.
    variant:
      "initial"   lamb_bar = 1e-3, Z_bar = 0 (the reference's mid_state values, :353-356);
      "consensus" Z_bar = [executed state; 0.5], lamb_bar random (an ADMM iterate's shape);
      "perturbed" like consensus with a perturbed initial state.
    """
    rng = np.random.default_rng(seed * 7919 + t_step * 31 + veh)
    refs = ref_traj_gen(spec)
    o = 1 - veh
    ref = refs[veh][t_step:t_step + N_HORZ].copy()
    init = executed_path(veh, t_step * DT, spec)
    A_o = np.zeros((NT, 4, 2))
    b_o = np.zeros((NT, 4))
    lij = np.zeros((NT, 4))
    mine = np.stack([executed_path(veh, (t_step + t) * DT, spec) for t in range(1, N_HORZ)])
    for t in range(1, N_HORZ):
        so = executed_path(o, (t_step + t) * DT, spec)
        A, b = halfspaces(so, prob)
        A_o[t - 1], b_o[t - 1] = A, b
        dvec = mine[t - 1][:2] - so[:2]
        lij[t - 1] = separating_duals(A, dvec / np.linalg.norm(dvec), alpha)
    if variant == "initial":
        lamb_bar = 1e-3 * np.ones((NT, 9))
        Z_bar = np.zeros((NT, 9))
    else:
        lamb_bar = 0.1 * rng.standard_normal((NT, 9))
        Z_bar = np.concatenate([mine, 0.5 * np.ones((NT, 4))], axis=1)
        Z_bar[:, :5] += 0.05 * rng.standard_normal((NT, 5))
    if variant == "perturbed":
        init = init + np.array([0.2, 0.1, -1.0, 0.02, 0.02]) * rng.uniform(-1, 1, 5)
        init[2] = min(init[2], 20.0 - 0.5)
    return pack(init, ref, A_o, b_o, lij, lamb_bar, Z_bar, prob=prob)


MID_LAMB_IJ = np.stack([
    np.array([[1.49, 0.566, 0.566, 1.49], [1.438, 0.514, 0.514, 1.438], [1.387, 0.462, 0.462, 1.387],
              [1.336, 0.411, 0.411, 1.336], [1.287, 0.361, 0.361, 1.287], [1.238, 0.312, 0.312, 1.238],
              [1.191, 0.263, 0.263, 1.191]]),
    np.repeat(np.array([1.436, 1.325, 1.213, 1.1, 0.986, 0.871, 0.755])[:, None], 4, axis=1)])


def create_bar_state(num_veh=2):
    """The initial bar_state (`mid_state`, optimizer.py:351-373): Z_bar, A, b, local_x zero,
    lamb_bar 1e-3, lamb_ij the hard-coded values of the reference."""
    return dict(Z_bar=np.zeros((num_veh, NT, 9)), A=np.zeros((num_veh, NT, 4, 2)), b=np.zeros((num_veh, NT, 4)),
                lamb_bar=1e-3 * np.ones((num_veh, NT, 9)), lamb_ij=MID_LAMB_IJ[:num_veh].copy(),
                local_x=np.zeros((num_veh, NT, 5)))


def iterate_next_state(bar):
    """Receding-horizon shift (optimizer.py:337-344): every array drops slot 0 and repeats its
    last slot."""
    out = dict(bar)
    for k in ("Z_bar", "A", "b", "lamb_bar", "lamb_ij", "local_x"):
        a = bar[k]
        out[k] = np.concatenate((a[:, 1:], a[:, -1:]), axis=1)
    return out


def stale_states(X, tau):
    """The states a vehicle's message describes when it arrives tau late: X (..., 8, 5) the local
    solve's states (X[0] is init_state), tau (...) the latency in [0, DT]; (..., 7, 5) with slot t =
    X[t+1] where tau == 0 (bit for bit) and X[t+1] + (tau / DT) (X[t] - X[t+1]) otherwise, all five
    entries, theta linearly, no wrap.  The statements of stale_state (csrc/piadmm_obca_plan.h) in
    the same order; every operation is exact IEEE arithmetic, so the device gives the same bits."""
    X = np.asarray(X, np.float64)
    assert X.shape[-2:] == (N_HORZ, NX), X.shape
    tau = np.broadcast_to(np.asarray(tau, np.float64), X.shape[:-2])[..., None, None]
    x0, x1 = X[..., :-1, :], X[..., 1:, :]
    f = tau / DT
    return np.where(tau == 0.0, x1, x1 + f * (x0 - x1))


def bar_state_update(bar, bar_fullx, prob=1, tau=None, fullX=None):
    """`bar_state_update` (optimizer.py:205-222): each vehicle's halfspaces at its new local
    states (the lamb_ij update stays commented out, as in the reference, :220).  With tau (one
    latency per vehicle) and fullX (each vehicle's 8 x 5 states, X[0] = init_state) the message is
    stale: the states are `stale_states(fullX[v], tau[v])` in place of the local ones."""
    out = {k: v.copy() for k, v in bar.items()}
    assert (tau is None) == (fullX is None), "tau and fullX go together"
    sent = None if tau is None else [stale_states(fullX[v], tau[v]) for v in range(len(bar_fullx))]
    for t in range(NT):
        for v in range(len(bar_fullx)):
            st = np.asarray(bar_fullx[v])[t, :5] if sent is None else sent[v][t]
            A, b = halfspaces(st, prob)
            out["A"][v, t] = A
            out["b"][v, t] = b
            out["local_x"][v, t] = st
    return out


def local_record(bar, veh, t_step, init_state, ref_traj, rho=1.0, min_dis=0.1, prob=1, max_x=150.0, max_y=20.0,
                 r=1e4, q=1e5, max_iter=60):
    """The record of vehicle `veh`'s local NLP: what local_initialize (:40-58) +
    local_generate_constrain (:84-129, the OTHER vehicle's bar_state slots) +
    local_generate_variable + local_generate_object (:150-168, this vehicle's lamb_bar and Z_bar)
    read, for one batched `OBCABatch.solve`."""
    o = 1 - veh
    ref = np.asarray(ref_traj[veh], np.float64)[t_step:t_step + N_HORZ]
    return pack(np.asarray(init_state, np.float64).ravel(), ref, bar["A"][o], bar["b"][o], bar["lamb_ij"][o],
                bar["lamb_bar"][veh], bar["Z_bar"][veh], rho=rho, min_dis=min_dis, max_x=max_x, max_y=max_y, r=r,
                q=q, prob=prob, max_iter=max_iter)


def as_written_problem(t_step=0, veh=0, prob=1, spec=None):
    """The reference's first ADMM iterate as written: bar_state = mid_state (A = b = 0, the
    hard-coded lamb_ij, lamb_bar = 1e-3, Z_bar = 0; optimizer.py:351-373).  (5b) then forces
    A(X_t)' Lambda_t = 0, so (5a) reads -b0' Lambda >= 0.1 with Lambda >= 0: infeasible."""
    refs = ref_traj_gen(spec)
    return local_record(create_bar_state(), veh, t_step, refs[veh][t_step], refs, prob=prob)


def scenario_batch(n, prob=1, seed=0):
    """n local problems cycling over (t_step 0..41, vehicle, variant) of the overtaking scenario."""
    recs = []
    variants = ("initial", "consensus", "perturbed")
    k = 0
    while len(recs) < n:
        t_step = k % 42
        veh = (k // 42) % 2
        var = variants[(k // 84) % 3]
        recs.append(overtaking_problem(t_step, veh, var, prob=prob, seed=seed + k // 252))
        k += 1
    return np.ascontiguousarray(np.stack(recs))


# ---------------------------------------------------------------------------------------------
# The coordinator (RSU) half of an ADMM iterate: the edge NLP on the consensus variable Z
# (optimizer.py:239-328), lambda_update (:330-335) and check_converge (:225-235).
#
# Edge record (float64, ``EDGE_REC`` per vehicle pair):
#   local_x 2x7x5 | lamb_ij 2x7x4 | lamb_bar 2x7x9 |
#   rho, min_dis, prob, max_iter, round_decimals, start, x_bound, mu_max, g_max | pad
# Edge output (float64, ``EDGE_OUT`` per pair): Z 2x7x9 (unrounded) | Z_bar 2x7x9 |
#   lamb_bar_new 2x7x9 | y_eq 7x2 | y_in 7 | y_bnd 7x18 | cost 7 | dres 7 | pad;
#   status / SQP iterations / QP steps per slot (int32, 7 x 3).
# ---------------------------------------------------------------------------------------------
EDGE_REC = 264
EDGE_OUT = 544
NE = 2 * (NX + NL)                   # variables of one slot problem: [s_0, mu_0, s_1, mu_1]
_E_LX, _E_LIJ, _E_LB, _E_PAR = 0, 70, 126, 252
_EO_Z, _EO_ZB, _EO_LBN, _EO_YEQ, _EO_YIN, _EO_YBND, _EO_COST, _EO_DRES = 0, 126, 252, 378, 392, 399, 525, 532
EDGE_WRITES_ITERATE = (0, 1, 3)      # converged, max_iter, linesearch_fail (the last accepted iterate)


def edge_record(bar, rho=1.0, min_dis=0.1, prob=1, max_iter=60, round_decimals=4, start=1, x_bound=1000.0,
                mu_max=100000.0, g_max=1000.0):
    """The record of one vehicle pair's edge NLP: what edge_generate_object (optimizer.py:297-307)
    reads of bar_state, and the bounds of :282-295 as record fields.  start: 0 = the reference's
    zeros (:249-250), 1 = w = [local_x, lamb_ij] clipped into the bounds."""
    rec = np.zeros(EDGE_REC)
    rec[_E_LX:_E_LX + 70] = np.asarray(bar["local_x"], np.float64)[:2].ravel()
    rec[_E_LIJ:_E_LIJ + 56] = np.asarray(bar["lamb_ij"], np.float64)[:2].ravel()
    rec[_E_LB:_E_LB + 126] = np.asarray(bar["lamb_bar"], np.float64)[:2].ravel()
    rec[_E_PAR:_E_PAR + 9] = [rho, min_dis, float(prob), float(max_iter), float(round_decimals), float(start),
                              x_bound, mu_max, g_max]
    return rec


def edge_unpack(rec):
    """dict of an edge record's fields."""
    rec = np.asarray(rec, np.float64)
    par = rec[_E_PAR:_E_PAR + 9]
    return dict(local_x=rec[_E_LX:_E_LX + 70].reshape(2, NT, NX).copy(),
                lamb_ij=rec[_E_LIJ:_E_LIJ + 56].reshape(2, NT, NL).copy(),
                lamb_bar=rec[_E_LB:_E_LB + 126].reshape(2, NT, 9).copy(),
                rho=par[0], min_dis=par[1], prob=int(par[2]), max_iter=int(par[3]), round_decimals=int(par[4]),
                start=int(par[5]), x_bound=par[6], mu_max=par[7], g_max=par[8])


def local_z(bar):
    """w = [local_x, lamb_ij] (num_veh x 7 x 9), the local side of the consensus (optimizer.py:303-304, :333)."""
    return np.concatenate([bar["local_x"], bar["lamb_ij"]], axis=2)


def lambda_update(bar, rho):
    """`lambda_update` (optimizer.py:330-335): lamb_bar += rho (w - Z_bar).  Host form of the
    update the edge kernel fuses behind its solve."""
    out = {k: v.copy() for k, v in bar.items()}
    out["lamb_bar"] = bar["lamb_bar"] + rho * (local_z(bar) - bar["Z_bar"])
    return out


# a gains row of the PI anti-windup dual law (piadmm_obca_dual_plan, include/piadmm.h)
DUAL_ROW = ("kP", "kI", "windup_sat", "d_gain", "windup")
DUAL_PAR = 8                          # doubles per row (PIADMM_OBCA_DUAL_PAR); the rest is zero
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
    import types
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


# a plant row of the closed-loop feedback (piadmm_obca_feedback_plan / piadmm_obca_propagate,
# include/piadmm.h): these 8 doubles per vehicle, vehicle 0 first
FEEDBACK_ROW = ("method", "n_sub", "lr", "lf", "gain_a", "gain_w", "a_max", "w_max")
FEEDBACK_PAR = 16                     # doubles per row (PIADMM_OBCA_FEEDBACK_PAR)
FEEDBACK_N_SUB_MAX = 64
MAX_STEER = 0.6                       # max_front_wheel_angle (veh_config.py)
# the nominal plant: the NLP's own transition st + dt f(st, con) (optimizer.py:92-96)
_FEEDBACK_DEFAULT = dict(method=0, n_sub=1, lr=1.0, lf=1.5, gain_a=1.0, gain_w=1.0, a_max=5.0, w_max=20.0)


def feedback_row(**kw):
    """One plant row (FEEDBACK_PAR doubles) from FEEDBACK_ROW names, each one value for both vehicles
    or a pair (vehicle 0, vehicle 1); absent: the nominal plant (Euler, n_sub 1, lr 1.0, lf 1.5,
    gains 1, a_max 5, w_max 20)."""
    assert set(kw) <= set(FEEDBACK_ROW), set(kw) - set(FEEDBACK_ROW)
    row = np.zeros((2, len(FEEDBACK_ROW)))
    for j, k in enumerate(FEEDBACK_ROW):
        row[:, j] = np.broadcast_to(np.asarray(kw.get(k, _FEEDBACK_DEFAULT[k]), np.float64), (2,))
    return row.reshape(FEEDBACK_PAR)


def feedback_row_check(row):
    """None when the plant row is good, else what is wrong with it: the library's check."""
    row = np.asarray(row, np.float64).reshape(2, len(FEEDBACK_ROW))
    if not np.isfinite(row).all():
        return "every entry finite"
    for method, n_sub, lr, lf, _, _, a_max, w_max in row:
        if method not in (0.0, 1.0):
            return "method 0 (Euler) or 1 (RK4)"
        if not (1.0 <= n_sub <= FEEDBACK_N_SUB_MAX and n_sub == math.floor(n_sub)):
            return "1 <= n_sub <= 64, an integer"
        if not (lr > 0.0 and lf > 0.0):
            return "lr, lf > 0"
        if not (a_max > 0.0 and w_max > 0.0):
            return "a_max, w_max > 0"
    return None


def _plant_rhs(x, a_eff, w_eff, lr, lf):
    """The reference's right-hand side (optimizer.py:75-77) of the states x (..., 5)."""
    beta = np.arctan(lr * np.tan(x[..., 4]) / (lr + lf))
    ph = x[..., 3] + beta
    v = x[..., 2]
    return np.stack((v * np.cos(ph), v * np.sin(ph), a_eff, v / lr * np.sin(beta), w_eff), axis=-1)


def propagate(states, ctrl, par, w=None):
    """One plant step of length DT per vehicle, host restatement of k_plan_propagate
    (csrc/piadmm_obca_plan_feedback.hip) with the same statements in the same order: states n x 2 x 5
    (x, y, v, theta, delta), ctrl n x 2 x 2 the held (a, omega), par one plant row for all or n rows
    (`feedback_row`), w n x 2 x 5 the disturbance or None.  n_sub substeps of DT / n_sub of
        beta = atan(lr tan(delta) / (lr + lf))
        rhs = (v cos(theta + beta), v sin(theta + beta), a_eff, v / lr sin(beta), w_eff)
    with a_eff = clip(gain_a a, +-a_max), w_eff = clip(gain_w omega, +-w_max): explicit Euler
    (method 0) or classical RK4 (method 1), delta clipped to +-MAX_STEER after every substep, w added
    after the last.  The nominal row with w = None is st + DT f(st, con)."""
    x = np.array(states, np.float64)
    n = x.shape[0] if x.ndim == 3 else 0
    ctrl = np.asarray(ctrl, np.float64)
    assert x.shape == (n, 2, NX) and ctrl.shape == (n, 2, NU), (x.shape, ctrl.shape)
    P = np.broadcast_to(np.asarray(par, np.float64).reshape(-1, 2, len(FEEDBACK_ROW)), (n, 2, len(FEEDBACK_ROW)))
    for k in range(n):
        why = feedback_row_check(P[k])
        if why is not None:
            raise ValueError(f"obca.propagate: row {k}: {why}")
    rk4, n_sub, lr, lf = P[..., 0] != 0.0, P[..., 1].astype(np.int64), P[..., 2], P[..., 3]
    a_eff = np.minimum(P[..., 6], np.maximum(P[..., 4] * ctrl[..., 0], -P[..., 6]))
    w_eff = np.minimum(P[..., 7], np.maximum(P[..., 5] * ctrl[..., 1], -P[..., 7]))
    hs = (DT / n_sub.astype(np.float64))[..., None]
    for sub in range(int(n_sub.max()) if n else 0):
        k1 = _plant_rhs(x, a_eff, w_eff, lr, lf)
        nxt = x + hs * k1
        if rk4.any():
            k2 = _plant_rhs(x + (0.5 * hs) * k1, a_eff, w_eff, lr, lf)
            k3 = _plant_rhs(x + (0.5 * hs) * k2, a_eff, w_eff, lr, lf)
            k4 = _plant_rhs(x + hs * k3, a_eff, w_eff, lr, lf)
            acc = k1 + 2.0 * k2 + 2.0 * k3 + k4
            nxt = np.where(rk4[..., None], x + (hs / 6.0) * acc, nxt)
        nxt[..., 4] = np.minimum(MAX_STEER, np.maximum(nxt[..., 4], -MAX_STEER))
        x = np.where((sub < n_sub)[..., None], nxt, x)
    if w is not None:
        w = np.asarray(w, np.float64)
        assert w.shape == x.shape, (w.shape, x.shape)
        x = x + w
    return x


def feedback_args(n, feedback):
    """(par, tape) of a planner's feedback argument dict(par=, tape=): par one plant row or n rows
    (None: the nominal row), as rows x FEEDBACK_PAR; tape n x cap x 2 x 5 or None."""
    assert set(feedback) <= {"par", "tape"}, set(feedback)
    par, tape = feedback.get("par"), feedback.get("tape")
    par = feedback_row() if par is None else par
    par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, FEEDBACK_PAR))
    assert par.shape[0] in (1, n), par.shape
    if tape is not None:
        tape = np.ascontiguousarray(tape, np.float64)
        assert tape.ndim == 4 and tape.shape[0] == n and tape.shape[2:] == (2, NX), tape.shape
    return par, tape


# the device-side disturbance noise (piadmm_obca_noise_plan / piadmm_obca_noise_tape,
# include/piadmm.h): a noise row is sigma[2][5], bias[2][5], trunc and one reserved zero
NOISE_PAR = 22                        # doubles per row (PIADMM_OBCA_NOISE_PAR)
NOISE_K_MAX = 1 << 31                 # step indices stay below it
# the noise items of piadmm_obca_plan_get: name -> (code, dtype) (PIADMM_OBCA_NOISE_GET_*)
NOISE_GET = {"NOISE_PAR": (36, np.float64), "NOISE_STREAMS": (37, np.int64), "NOISE_SEED": (38, np.uint64)}
_PHILOX_M = (np.uint64(0xD2511F53), np.uint64(0xCD9E8D57))
_PHILOX_W = (np.uint64(0x9E3779B9), np.uint64(0xBB67AE85))
_U32 = np.uint64(0xFFFFFFFF)


def philox4x32(counter, key):
    """Philox4x32-10 (Salmon, Moraes, Dror, Shaw, SC'11), vectorised over leading axes: counter
    (..., 4) and key (..., 2) 32-bit words (broadcast against each other), the result (..., 4)
    uint32.  Ten rounds; a round takes the 64-bit products of the multipliers 0xD2511F53 with c0 and
    0xCD9E8D57 with c2 to (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0), the key bumped by 0x9E3779B9 and
    0xBB67AE85 between rounds.  k_plan_noise runs the same statements in 32-bit registers."""
    c = np.asarray(counter).astype(np.uint64) & _U32
    k = np.asarray(key).astype(np.uint64) & _U32
    assert c.shape[-1] == 4 and k.shape[-1] == 2, (c.shape, k.shape)
    lead = np.broadcast_shapes(c.shape[:-1], k.shape[:-1])
    c0, c1, c2, c3 = (np.broadcast_to(c[..., i], lead) for i in range(4))
    k0, k1 = (np.broadcast_to(k[..., i], lead) for i in range(2))
    for _ in range(10):
        p0, p1 = _PHILOX_M[0] * c0, _PHILOX_M[1] * c2
        c0, c1, c2, c3 = (p1 >> np.uint64(32)) ^ c1 ^ k0, p1 & _U32, (p0 >> np.uint64(32)) ^ c3 ^ k1, p0 & _U32
        k0, k1 = (k0 + _PHILOX_W[0]) & _U32, (k1 + _PHILOX_W[1]) & _U32
    return np.stack((c0, c1, c2, c3), axis=-1).astype(np.uint32)


def noise_raw(seed, streams, k, calls=(0, 1, 2)):
    """The generator's words of the streams `streams` (m int64, >= 0) at step index k: m x 2 x 3 x 4
    uint32, the call j of vehicle v at counter (k, 4 v + j, t & 0xffffffff, t >> 32) under the key
    (seed & 0xffffffff, seed >> 32).  calls: the call indices j (each below 4), the third axis; the
    noise's are 0, 1, 2 and the communication delay's is 3 (`delay_tau`)."""
    t = np.asarray(streams, np.int64).reshape(-1)
    seed, k = int(seed), int(k)
    calls = np.asarray(calls, np.int64).reshape(-1)
    assert (t >= 0).all() and 0 <= seed < 1 << 64 and 0 <= k < NOISE_K_MAX, (seed, k)
    assert ((calls >= 0) & (calls < 4)).all(), calls
    t = t.astype(np.uint64)
    counter = np.zeros((len(t), 2, len(calls), 4), np.uint64)
    counter[..., 0] = k
    counter[..., 1] = (4 * np.arange(2)[:, None] + calls[None, :])[None]
    counter[..., 2] = (t & _U32)[:, None, None]
    counter[..., 3] = (t >> np.uint64(32))[:, None, None]
    return philox4x32(counter, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def noise_uniform(seed, streams, k, calls=(0, 1, 2)):
    """The uniforms of `noise_raw`: m x 2 x 3 x 2 fp64, (u1, u2) of every call,
    u = (((hi << 32 | lo) >> 12) + 0.5) 2^-52 -- 52 bits and the half, exact in fp64 and strictly
    inside (0, 1)."""
    r = noise_raw(seed, streams, k, calls).astype(np.uint64)
    a = (r[..., 0::2] << np.uint64(32) | r[..., 1::2]) >> np.uint64(12)
    return (a.astype(np.float64) + 0.5) * 2.0 ** -52


def noise_normal(seed, streams, k):
    """The standard normals of the streams at step index k: m x 2 x 5, by Box-Muller from
    `noise_uniform` -- rad = sqrt(-2 log(u1)), z[2 j] = rad cos(2 pi u2), z[2 j + 1] = rad sin(2 pi u2)
    -- for (x, y, v, theta, delta) of each vehicle; the sixth is discarded."""
    u = noise_uniform(seed, streams, k)
    rad = np.sqrt(-2.0 * np.log(u[..., 0]))
    ang = (2.0 * np.pi) * u[..., 1]
    z = np.stack((rad * np.cos(ang), rad * np.sin(ang)), axis=-1)
    return z.reshape(z.shape[0], 2, 6)[..., :NX]


def noise_row(sigma=0.0, bias=0.0, trunc=0.0):
    """One noise row (NOISE_PAR doubles): sigma and bias each one value, five (x, y, v, theta, delta;
    both vehicles) or 2 x 5; trunc 0 for none, else z is clipped to +-trunc before it is scaled."""
    row = np.zeros(NOISE_PAR)
    row[0:10] = np.broadcast_to(np.asarray(sigma, np.float64), (2, NX)).reshape(10)
    row[10:20] = np.broadcast_to(np.asarray(bias, np.float64), (2, NX)).reshape(10)
    row[20] = float(trunc)
    return row


def noise_row_check(row):
    """None when the noise row is good, else what is wrong with it: the library's check."""
    row = np.asarray(row, np.float64).reshape(NOISE_PAR)
    if not np.isfinite(row).all():
        return "every entry finite"
    if not (row[0:10] >= 0.0).all():
        return "sigma >= 0"
    if not row[20] >= 0.0:
        return "trunc 0 (none) or > 0"
    if row[21] != 0.0:
        return "the reserved entry must be 0"
    return None


def noise_args(n, par=None, streams=None, seed=0, k0=0):
    """(par, streams, seed, k0) of a noise argument: par one noise row or n rows (None: the zero
    row), as rows x NOISE_PAR; streams n int64 (None: 0 .. n-1); checked as the library checks."""
    par = noise_row() if par is None else par
    par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, NOISE_PAR))
    if par.shape[0] not in (1, n):
        raise ValueError(f"obca.noise: rows must be 1 or n ({n})")
    for k, row in enumerate(par):
        why = noise_row_check(row)
        if why is not None:
            raise ValueError(f"obca.noise: row {k}: {why}")
    streams = np.arange(n, dtype=np.int64) if streams is None else np.ascontiguousarray(streams, np.int64).reshape(-1)
    if streams.shape != (n,) or (streams < 0).any():
        raise ValueError(f"obca.noise: streams must be {n} ids >= 0")
    seed, k0 = int(seed), int(k0)
    if not (0 <= seed < 1 << 64 and 0 <= k0 < NOISE_K_MAX):
        raise ValueError("obca.noise: seed a uint64 and 0 <= k0 < 2^31")
    return par, streams, seed, k0


def noise_tape(n, cap, par, streams=None, seed=0, k0=0):
    """The disturbance rows k_plan_noise draws, host restatement with the same statements in the
    same order: n x cap x 2 x 5, row [s][i] = bias + sigma * clip(z, +-trunc) with z the normals of
    stream streams[s] (None: s) at step index k0 + i (`noise_normal`) under par (one noise row or
    n).  A pure function of (seed, stream, step index): any row can be drawn alone."""
    n, cap = int(n), int(cap)
    par, streams, seed, k0 = noise_args(n, par, streams, seed, k0)
    if k0 + cap > NOISE_K_MAX:
        raise ValueError("obca.noise_tape: every step index below 2^31")
    P = np.broadcast_to(par, (n, NOISE_PAR))
    sigma, bias, trunc = P[:, 0:10].reshape(n, 2, NX), P[:, 10:20].reshape(n, 2, NX), P[:, 20][:, None, None]
    out = np.zeros((n, cap, 2, NX))
    for i in range(cap):
        z = noise_normal(seed, streams, k0 + i)
        z = np.where(trunc != 0.0, np.minimum(trunc, np.maximum(z, -trunc)), z)
        out[:, i] = bias + sigma * z
    return out


# the communication delay of the plan's exchange (piadmm_obca_delay_plan / piadmm_obca_delay_tau /
# piadmm_obca_delay_exchange, include/piadmm.h): a delay row is avg[2], std[2], tau_max[2], trunc and
# one reserved zero
DELAY_PAR = 8                         # doubles per row (PIADMM_OBCA_DELAY_PAR)
DELAY_CALL = 3                        # the Philox call index of the latency: the one the noise leaves free
# the delay items of piadmm_obca_plan_get: name -> (code, dtype) (PIADMM_OBCA_DELAY_GET_*)
DELAY_GET = {"DELAY_PAR": (39, np.float64), "DELAY_TAU": (40, np.float64), "DELAY_STREAMS": (41, np.int64),
             "DELAY_SEED": (42, np.uint64)}


def delay_row(avg=0.0, std=0.0, tau_max=DT, trunc=0.0):
    """One delay row (DELAY_PAR doubles): avg, std and tau_max each one value or one per vehicle;
    trunc 0 for none, else z is clipped to +-trunc before it is scaled.  The default row draws
    tau = 0 always: the plain exchange."""
    row = np.zeros(DELAY_PAR)
    row[0:2] = np.broadcast_to(np.asarray(avg, np.float64), (2,))
    row[2:4] = np.broadcast_to(np.asarray(std, np.float64), (2,))
    row[4:6] = np.broadcast_to(np.asarray(tau_max, np.float64), (2,))
    row[6] = float(trunc)
    return row


def delay_row_check(row):
    """None when the delay row is good, else what is wrong with it: the library's check."""
    row = np.asarray(row, np.float64).reshape(DELAY_PAR)
    if not np.isfinite(row).all():
        return "every entry finite"
    for v in (0, 1):
        if not row[0 + v] >= 0.0:
            return "avg >= 0"
        if not row[2 + v] >= 0.0:
            return "std >= 0"
        if not 0.0 <= row[4 + v] <= DT:
            return "0 <= tau_max <= DT"
    if not row[6] >= 0.0:
        return "trunc 0 (none) or > 0"
    if row[7] != 0.0:
        return "the reserved entry must be 0"
    return None


def delay_args(n, par=None, streams=None, seed=0, k0=0, tape=None):
    """(par, streams, seed, k0, tape) of a delay argument: par one delay row or n rows (None: the
    default row), as rows x DELAY_PAR; streams n int64 (None: 0 .. n-1); tape n x cap x 2 finite
    recorded latencies or None; checked as the library checks."""
    par = delay_row() if par is None else par
    par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, DELAY_PAR))
    if par.shape[0] not in (1, n):
        raise ValueError(f"obca.delay: rows must be 1 or n ({n})")
    for k, row in enumerate(par):
        why = delay_row_check(row)
        if why is not None:
            raise ValueError(f"obca.delay: row {k}: {why}")
    streams = np.arange(n, dtype=np.int64) if streams is None else np.ascontiguousarray(streams, np.int64).reshape(-1)
    if streams.shape != (n,) or (streams < 0).any():
        raise ValueError(f"obca.delay: streams must be {n} ids >= 0")
    seed, k0 = int(seed), int(k0)
    if not (0 <= seed < 1 << 64 and 0 <= k0 < NOISE_K_MAX):
        raise ValueError("obca.delay: seed a uint64 and 0 <= k0 < 2^31")
    if tape is not None:
        tape = np.ascontiguousarray(tape, np.float64)
        if tape.ndim != 3 or tape.shape[0] != n or tape.shape[2] != 2 or not np.isfinite(tape).all():
            raise ValueError(f"obca.delay: the tape must be {n} x cap x 2 and finite")
    return par, streams, seed, k0, tape


def delay_tau(n, cap, par, streams=None, seed=0, k0=0, tape=None):
    """The latencies k_plan_delay draws, host restatement with the same statements in the same
    order: n x cap x 2, entry [s][i][v] = min(tau_max[v], max(0, tape[s][i][v] + (avg[v] + std[v] *
    clip(z, +-trunc)))) with z = sqrt(-2 log u1) cos(2 pi u2) of the Philox call DELAY_CALL of
    vehicle v of stream streams[s] (None: s) at step index k0 + i (`noise_uniform`), under par (one
    delay row or n); tape the recorded latencies (None: 0).  A pure function of (seed, stream, step
    index); the noise's calls are 0, 1, 2, so the same seed and streams give independent draws."""
    n, cap = int(n), int(cap)
    par, streams, seed, k0, tape = delay_args(n, par, streams, seed, k0, tape)
    if k0 + cap > NOISE_K_MAX:
        raise ValueError("obca.delay_tau: every step index below 2^31")
    if tape is not None and tape.shape[1] != cap:
        raise ValueError(f"obca.delay_tau: the tape must be {n} x {cap} x 2")
    P = np.broadcast_to(par, (n, DELAY_PAR))
    avg, std, tau_max, trunc = P[:, 0:2], P[:, 2:4], P[:, 4:6], P[:, 6][:, None]
    out = np.zeros((n, cap, 2))
    for i in range(cap):
        u = noise_uniform(seed, streams, k0 + i, calls=(DELAY_CALL,))[:, :, 0]
        rad = np.sqrt(-2.0 * np.log(u[..., 0]))
        ang = (2.0 * np.pi) * u[..., 1]
        z = rad * np.cos(ang)
        z = np.where(trunc != 0.0, np.minimum(trunc, np.maximum(z, -trunc)), z)
        x = (0.0 if tape is None else tape[:, i]) + (avg + std * z)
        lo = np.where(x > 0.0, x, 0.0)
        out[:, i] = np.where(lo < tau_max, lo, tau_max)
    return out


def check_converge(bar, thres, min_dis):
    """`check_converge` (optimizer.py:225-235): the coupled constraints at the exchanged
    halfspaces and lamb_ij."""
    eq = np.einsum("tij,ti->tj", bar["A"][0], bar["lamb_ij"][0]) + np.einsum("tij,ti->tj", bar["A"][1], bar["lamb_ij"][1])
    ueq = -np.einsum("ti,ti->t", bar["b"][0], bar["lamb_ij"][0]) - np.einsum("ti,ti->t", bar["b"][1], bar["lamb_ij"][1])
    return bool((np.abs(eq) <= thres).all() and (ueq >= min_dis).all())


def seeded_bar_state(t_step, prob=1, alpha=0.9, spec=None):
    """A runnable initial bar_state at MPC step t_step: A, b, local_x from `executed_path`
    (slots t_step + 1 .. t_step + 7), lamb_ij each vehicle's own `separating_duals` along the
    direction to the other vehicle (so A_0' lamb_0 + A_1' lamb_1 = 0), Z_bar = [local_x, lamb_ij],
    lamb_bar = 1e-3 (mid_state's value, optimizer.py:356).  The reference's mid_state (create_bar_state) is infeasible as written
    (`as_written_problem`)."""
    bar = create_bar_state()
    for t in range(NT):
        st = [executed_path(v, (t_step + t + 1) * DT, spec) for v in (0, 1)]
        for v in (0, 1):
            A, b = halfspaces(st[v], prob)
            dvec = st[1 - v][:2] - st[v][:2]
            bar["A"][v, t], bar["b"][v, t] = A, b
            bar["local_x"][v, t] = st[v]
            bar["lamb_ij"][v, t] = separating_duals(A, dvec / np.linalg.norm(dvec), alpha)
    bar["Z_bar"] = local_z(bar)
    bar["lamb_bar"] = 1e-3 * np.ones((2, NT, 9))
    return bar


def overtaking_fleet(n, seed=0):
    """n different overtakes for one batch: (specs, params) with params = dict(rho=, min_dis=)
    of length-n arrays, for `OBCAPlanner(batch, n, specs=specs, **params)` and OBCADevicePlanner
    alike.  Uniform draws: v0 in [16, 20] (20 is the vehicle's max_v; above it the local NLP is
    infeasible), v1 in [8, 12], gap in [12, 20], lane in [3, 4], rho in [0.5, 2], min_dis in
    [0.05, 0.3].  The CPU restatement of both solves converges on these ranges while vehicle 0 is
    behind or ahead (16 draws of seed 0 at MPC steps 5 and 8: 1 solve of 288 not CONVERGED); at the
    steps where the vehicles are alongside (step 12) a draw with a lane below about 3.6 m can
    end a solve on another status, which the planners record like every status."""
    rng = np.random.default_rng(seed)
    u = rng.uniform(size=(int(n), 6))
    specs = [OvertakeSpec(v0=16.0 + 4.0 * a[0], v1=8.0 + 4.0 * a[1], gap=12.0 + 8.0 * a[2], lane=3.0 + a[3]) for a in u]
    return specs, dict(rho=0.5 + 1.5 * u[:, 4], min_dis=0.05 + 0.25 * u[:, 5])


class OBCAEdgeResult:
    """Decoded output of an edge batch (pairs x ...)."""

    def __init__(self, out, ist):
        n = out.shape[0]
        self.raw = out
        self.Z = out[:, _EO_Z:_EO_Z + 126].reshape(n, 2, NT, 9)
        self.Z_bar = out[:, _EO_ZB:_EO_ZB + 126].reshape(n, 2, NT, 9)
        self.lamb_bar = out[:, _EO_LBN:_EO_LBN + 126].reshape(n, 2, NT, 9)
        self.y_eq = out[:, _EO_YEQ:_EO_YEQ + 14].reshape(n, NT, 2)
        self.y_in = out[:, _EO_YIN:_EO_YIN + 7]
        self.y_bnd = out[:, _EO_YBND:_EO_YBND + 126].reshape(n, NT, NE)
        self.cost = out[:, _EO_COST:_EO_COST + 7]
        self.dres = out[:, _EO_DRES:_EO_DRES + 7]
        self.status = ist[:, :, 0]
        self.iters = ist[:, :, 1]
        self.qp_steps = ist[:, :, 2]

    def z(self, k, t):
        """The 18 variables [s_0, mu_0, s_1, mu_1] of pair k, slot t."""
        return np.concatenate([self.Z[k, 0, t], self.Z[k, 1, t]])

    def dual_residual(self):
        """sum |lamb_bar_new - lamb_bar| per pair: the 7 slot partials added in index order."""
        s = np.zeros(self.dres.shape[0])
        for t in range(NT):
            s = s + self.dres[:, t]
        return s


class OBCAResult:
    """Decoded output of a batch (fields as in the reference's local_solve, :183-201)."""

    def __init__(self, out, ist):
        self.raw = out
        self.X = out[:, :40].reshape(-1, 8, 5)
        self.U = out[:, 40:54].reshape(-1, 7, 2)
        self.Lam = out[:, 54:82].reshape(-1, 7, 4)
        self.y_a = out[:, 82:89]
        self.y_b = out[:, 89:103].reshape(-1, 7, 2)
        self.y_n = out[:, 103:110]
        self.y_x = out[:, 110:145].reshape(-1, 7, 5)
        self.pi = out[:, 145:180].reshape(-1, 7, 5)
        self.y_u = out[:, 180:194]
        self.y_l = out[:, 194:222]
        self.cost = out[:, 222]
        self.status = ist[:, 0]
        self.iters = ist[:, 1]
        self.qp_steps = ist[:, 2]

    def bar_fullx(self, k):
        """N_horz-1 x 9 [X_t, Lambda_t] of problem k (optimizer.py:201)."""
        return np.concatenate([self.X[k, 1:], self.Lam[k]], axis=1)


class OBCABatch:
    """Device-resident batch of local problems.  ``solve`` runs one launch of the batched SQP
    (one wave per problem) and returns an OBCAResult; there is no CPU path."""

    def __init__(self, device: int = 0):
        from . import _lib
        self._lib = _lib.load()
        self._h = ctypes.c_void_p()
        rc = self._lib.piadmm_obca_create(int(device), ctypes.byref(self._h))
        if rc != 0:
            raise _lib.PiadmmError(f"piadmm_obca_create failed ({rc})")

    def _check(self, rc):
        from . import _lib
        if rc != 0:
            msg = self._lib.piadmm_obca_last_error(self._h)
            raise _lib.PiadmmError(f"libpiadmm error {rc}: {msg.decode() if msg else ''}")

    def close(self):
        if self._h:
            self._lib.piadmm_obca_destroy(self._h)
            self._h = ctypes.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def solve(self, recs: np.ndarray) -> OBCAResult:
        from . import _lib
        recs = np.ascontiguousarray(recs, np.float64)
        n = recs.shape[0]
        assert recs.shape == (n, REC)
        out = np.zeros((n, OUT))
        ist = np.zeros((n, 3), np.int32)
        self._check(self._lib.piadmm_obca_solve(self._h, _lib.dptr(recs), n, _lib.dptr(out), _lib.iptr(ist)))
        return OBCAResult(out, ist)

    def solve_edge(self, recs: np.ndarray) -> OBCAEdgeResult:
        """One launch of the edge SQP (one wave per slot problem, 7 per pair) with the fused
        lambda_update; separate device buffers from the local batch."""
        from . import _lib
        recs = np.ascontiguousarray(recs, np.float64)
        n = recs.shape[0]
        assert recs.shape == (n, EDGE_REC)
        out = np.zeros((n, EDGE_OUT))
        ist = np.zeros((n, NT, 3), np.int32)
        self._check(self._lib.piadmm_obca_edge_solve(self._h, _lib.dptr(recs), n, _lib.dptr(out), _lib.iptr(ist)))
        return OBCAEdgeResult(out, ist)

    def clearance(self, states, prob) -> np.ndarray:
        """n x 2 (plain, tight) clearances of the state pairs `states` (n x 2 x 5), one launch of
        k_plan_clearance on the call's own buffers; prob: one value or one per pair."""
        from . import _lib
        states = np.ascontiguousarray(states, np.float64)
        n = states.shape[0] if states.ndim == 3 else 0
        assert states.shape == (n, 2, NX), states.shape
        prob = np.ascontiguousarray(np.broadcast_to(np.asarray(prob, np.int32), (n,)))
        out = np.zeros((n, 2))
        self._check(self._lib.piadmm_obca_clearance(self._h, n, _lib.dptr(states), _lib.iptr(prob), _lib.dptr(out)))
        return out

    def dual_pi(self, w, zb, lamb, status, gains, S, D):
        """One launch of k_plan_dual_pi on the call's own buffers (piadmm_obca_dual_pi): w, zb, lamb,
        S, D n x 2 x 7 x 9, status n x 7, gains one row or n rows of DUAL_PAR.  Returns
        (lamb_out, S', D', dres n x 7); the arguments stay as they are."""
        from . import _lib
        w = np.ascontiguousarray(w, np.float64)
        n = w.shape[0] if w.ndim == 4 else 0
        shp = (n, 2, NT, 9)
        zb, lamb = np.ascontiguousarray(zb, np.float64), np.ascontiguousarray(lamb, np.float64)
        S, D = np.array(S, np.float64, order="C"), np.array(D, np.float64, order="C")
        assert w.shape == zb.shape == lamb.shape == S.shape == D.shape == shp, (w.shape, zb.shape, S.shape)
        status = np.ascontiguousarray(status, np.int32)
        assert status.shape == (n, NT), status.shape
        gains = np.ascontiguousarray(np.atleast_2d(np.asarray(gains, np.float64)))
        assert gains.ndim == 2 and gains.shape[1] == DUAL_PAR, gains.shape
        lamb_out, dres = np.zeros(shp), np.zeros((n, NT))
        self._check(self._lib.piadmm_obca_dual_pi(self._h, n, _lib.dptr(w), _lib.dptr(zb), _lib.dptr(lamb),
                                                  _lib.iptr(status), _lib.dptr(gains), gains.shape[0], _lib.dptr(S),
                                                  _lib.dptr(D), _lib.dptr(lamb_out), _lib.dptr(dres)))
        return lamb_out, S, D, dres

    def order(self, lst, work) -> np.ndarray:
        """One launch of k_plan_order on the call's own buffers (piadmm_obca_order): the m distinct
        scenarios of `lst` sorted by `work` (n x 2), as `plan_order` states it."""
        from . import _lib
        lst = np.ascontiguousarray(lst, np.int32).reshape(-1)
        work = np.ascontiguousarray(work, np.int32)
        assert work.ndim == 2 and work.shape[1] == 2, work.shape
        out = np.zeros(len(lst), np.int32)
        self._check(self._lib.piadmm_obca_order(self._h, _lib.iptr(lst), len(lst), _lib.iptr(work), work.shape[0],
                                                _lib.iptr(out)))
        return out

    def clock_tick(self, clock, ran, ref):
        """One launch each of k_plan_clock and k_plan_compact on the call's own buffers
        (piadmm_obca_clock_tick): clock n x 3, ran n, ref 2 x n_ref x 5 or n x 2 x n_ref x 5.
        Returns (clock_out, window n x 2 x 8 x 5, the alive scenarios ascending), as `clock_tick` /
        `clock_window` state them."""
        from . import _lib
        clock = np.ascontiguousarray(clock, np.int32)
        n = clock.shape[0]
        assert clock.shape == (n, 3), clock.shape
        ran = np.ascontiguousarray(ran, np.int32)
        ref = np.ascontiguousarray(ref, np.float64)
        assert ran.shape == (n,) and ref.shape[-3] == 2 and ref.shape[-1] == NX, (ran.shape, ref.shape)
        rows = ref.shape[0] if ref.ndim == 4 else 1
        out, win = np.zeros((n, 3), np.int32), np.zeros((n, 2, N_HORZ, NX))
        lst, count = np.zeros(n, np.int32), np.zeros(1, np.int32)
        self._check(self._lib.piadmm_obca_clock_tick(self._h, n, _lib.iptr(clock), _lib.iptr(ran), _lib.dptr(ref), rows,
                                                     ref.shape[-2], _lib.iptr(out), _lib.dptr(win), _lib.iptr(lst),
                                                     _lib.iptr(count)))
        assert 0 <= count[0] <= n and not lst[count[0]:].any()
        return out, win, lst[:count[0]].copy()

    def propagate(self, states, ctrl, par, w=None) -> np.ndarray:
        """One launch of k_plan_propagate on the call's own buffers (piadmm_obca_propagate): the
        states n x 2 x 5 the vehicles reach from `states` under the held controls ctrl (n x 2 x 2:
        a, omega), the plant rows par (one for all, or n) and the disturbance w (n x 2 x 5 or None),
        as `propagate` states it."""
        from . import _lib
        states = np.ascontiguousarray(states, np.float64)
        n = states.shape[0] if states.ndim == 3 else 0
        ctrl = np.ascontiguousarray(ctrl, np.float64)
        assert states.shape == (n, 2, NX) and ctrl.shape == (n, 2, NU), (states.shape, ctrl.shape)
        par = np.ascontiguousarray(np.broadcast_to(np.asarray(par, np.float64).reshape(-1, FEEDBACK_PAR),
                                                   (n, FEEDBACK_PAR)))
        if w is not None:
            w = np.ascontiguousarray(w, np.float64)
            assert w.shape == states.shape, w.shape
        out = np.zeros((n, 2, NX))
        self._check(self._lib.piadmm_obca_propagate(self._h, n, _lib.dptr(states), _lib.dptr(ctrl), _lib.dptr(par),
                                                    _lib.dptr(w), _lib.dptr(out)))
        return out

    def noise_tape(self, n, cap, par, streams=None, seed=0, k0=0, raw=False):
        """k_plan_noise on the call's own buffers (piadmm_obca_noise_tape): the disturbance rows
        n x cap x 2 x 5 of the streams `streams` (None: 0 .. n-1) at step indices k0 .. k0 + cap - 1
        under the noise rows par (one for all, or n), as `noise_tape` states them; with raw=True
        also the generator's words, n x cap x 2 x 3 x 4 uint32 (`noise_raw`).  The library checks
        the arguments."""
        from . import _lib
        n, cap = int(n), int(cap)
        par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, NOISE_PAR))
        if streams is not None:
            streams = np.ascontiguousarray(streams, np.int64).reshape(-1)
            assert streams.shape == (n,), streams.shape
        tape = np.zeros((max(n, 0), max(cap, 0), 2, NX))
        words = np.zeros((max(n, 0), max(cap, 0), 2, 3, 4), np.uint32) if raw else None
        self._check(self._lib.piadmm_obca_noise_tape(
            self._h, n, cap, _lib.dptr(par), par.shape[0],
            None if streams is None else streams.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            ctypes.c_uint64(int(seed)), int(k0), _lib.dptr(tape),
            None if words is None else words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return (tape, words) if raw else tape

    def delay_tau(self, n, cap, par, streams=None, seed=0, k0=0, tape=None, raw=False):
        """k_plan_delay on the call's own buffers (piadmm_obca_delay_tau): the latencies n x cap x 2
        of the streams `streams` (None: 0 .. n-1) at step indices k0 .. k0 + cap - 1 under the delay
        rows par (one for all, or n) and the recorded latencies tape (n x cap x 2 or None), as
        `delay_tau` states them; with raw=True also the call's words, n x cap x 2 x 4 uint32
        (`noise_raw` with calls=(3,)).  The library checks the arguments."""
        from . import _lib
        n, cap = int(n), int(cap)
        par = np.ascontiguousarray(np.asarray(par, np.float64).reshape(-1, DELAY_PAR))
        if streams is not None:
            streams = np.ascontiguousarray(streams, np.int64).reshape(-1)
            assert streams.shape == (n,), streams.shape
        if tape is not None:
            tape = np.ascontiguousarray(tape, np.float64)
            assert tape.shape == (n, cap, 2), tape.shape
        tau = np.zeros((max(n, 0), max(cap, 0), 2))
        words = np.zeros((max(n, 0), max(cap, 0), 2, 4), np.uint32) if raw else None
        self._check(self._lib.piadmm_obca_delay_tau(
            self._h, n, cap, _lib.dptr(par), par.shape[0],
            None if streams is None else streams.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            ctypes.c_uint64(int(seed)), int(k0), _lib.dptr(tape), _lib.dptr(tau),
            None if words is None else words.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))))
        return (tau, words) if raw else tau

    def delay_exchange(self, X, prob, tau):
        """The stale message alone, one launch of k_delay_exchange on the call's own buffers
        (piadmm_obca_delay_exchange): X n x 2 x 8 x 5 the local solves' states, prob one value or one
        per scenario, tau n x 2 latencies in [0, DT].  Returns (local_x n x 2 x 7 x 5, A n x 2 x 7 x
        4 x 2, b n x 2 x 7 x 4): `stale_states` and `halfspaces` of it."""
        from . import _lib
        X = np.ascontiguousarray(X, np.float64)
        n = X.shape[0] if X.ndim == 4 else 0
        tau = np.ascontiguousarray(tau, np.float64)
        assert X.shape == (n, 2, N_HORZ, NX) and tau.shape == (n, 2), (X.shape, tau.shape)
        prob = np.ascontiguousarray(np.broadcast_to(np.asarray(prob, np.int32), (n,)))
        lx, A, b = np.zeros((n, 2, NT, NX)), np.zeros((n, 2, NT, 4, 2)), np.zeros((n, 2, NT, 4))
        self._check(self._lib.piadmm_obca_delay_exchange(self._h, n, _lib.dptr(X), _lib.iptr(prob), _lib.dptr(tau),
                                                         _lib.dptr(lx), _lib.dptr(A), _lib.dptr(b)))
        return lx, A, b

    def fleet_stats(self, clear, summary, iters=None, mask=None, edges=(0.0,), worst=1) -> "OBCAFleetStats":
        """The fleet statistics of the caller's arrays (piadmm_obca_fleet_stats: k_stats_fleet,
        k_stats_rows and k_stats_worst on the call's own buffers), as `fleet_stats_host` states them:
        clear (R + 1) x n x 2, summary n x 4, iters R x n and mask R x n x 2 (None for R = 0)."""
        from . import _lib
        clear, summary = np.ascontiguousarray(clear, np.float64), np.ascontiguousarray(summary, np.float64)
        R, n = clear.shape[0] - 1, clear.shape[1]
        assert clear.shape == (R + 1, n, 2) and summary.shape == (n, 4), (clear.shape, summary.shape)
        iters = None if iters is None else np.ascontiguousarray(iters, np.int32)
        mask = None if mask is None else np.ascontiguousarray(mask, np.int32)
        assert iters is None or iters.shape == (R, n), iters.shape
        assert mask is None or mask.shape == (R, n, 2), mask.shape

        def call(*a):
            return self._lib.piadmm_obca_fleet_stats(self._h, R, n, _lib.dptr(clear), _lib.dptr(summary),
                                                     _lib.iptr(iters) if R else None, _lib.iptr(mask) if R else None, *a)
        rc, out = _stats_call(call, n, R, edges, worst)
        self._check(rc)
        return out

    def time_edge(self, recs: np.ndarray, repeats: int) -> float:
        """ms per edge launch over `repeats` launches of `recs` (HIP events)."""
        from . import _lib
        recs = np.ascontiguousarray(recs, np.float64)
        ms = ctypes.c_float()
        self._check(self._lib.piadmm_obca_edge_time(self._h, _lib.dptr(recs), recs.shape[0], int(repeats),
                                                    ctypes.byref(ms)))
        return ms.value

    def upload(self, recs: np.ndarray):
        from . import _lib
        recs = np.ascontiguousarray(recs, np.float64)
        self._check(self._lib.piadmm_obca_upload(self._h, _lib.dptr(recs), recs.shape[0]))

    def run_async(self, repeats: int = 1):
        self._check(self._lib.piadmm_obca_run(self._h, int(repeats)))

    def time(self, repeats: int) -> float:
        """ms per launch over `repeats` launches on the resident batch (HIP events)."""
        ms = ctypes.c_float()
        self._check(self._lib.piadmm_obca_time(self._h, int(repeats), ctypes.byref(ms)))
        return ms.value

    def download(self, n: int) -> OBCAResult:
        from . import _lib
        out = np.zeros((n, OUT))
        ist = np.zeros((n, 3), np.int32)
        self._check(self._lib.piadmm_obca_download(self._h, _lib.dptr(out), _lib.iptr(ist), n))
        return OBCAResult(out, ist)


# ---------------------------------------------------------------------------------------------
# The consensus loop (decentralized_overtaking_ADMM.py:31-102) for many scenarios at once
# ---------------------------------------------------------------------------------------------
# a parameter row of piadmm_obca_fleet_begin (include/piadmm.h), by constructor argument
FLEET_ROW = ("rho", "min_dis", "conv_thres", "max_x", "max_y", "r", "q", "x_bound", "mu_max", "g_max",
             "max_admm_iter", "max_iter", "round_decimals", "start")
_FLEET_INTS = ("max_admm_iter", "max_iter", "round_decimals", "start")
FLEET_PAR = 16                        # doubles per row (PIADMM_OBCA_FLEET_PAR); the rest is zero


def _per_scenario(pl, n, **params):
    """For each parameter: pl.<name>_s, its value per scenario, from a scalar or a length-n
    sequence (an integer one stays float where a value is not integral, so that the library sees
    it and refuses it).  True when any was a sequence."""
    any_seq = False
    for name, val in params.items():
        arr = np.asarray(val, np.float64)
        if arr.ndim:
            any_seq = True
            assert arr.shape == (n,), (name, arr.shape, n)
        arr = np.broadcast_to(arr, (n,)).copy()
        if name in _FLEET_INTS and np.all(np.isfinite(arr)) and np.all(arr == np.floor(arr)):
            arr = arr.astype(np.int64)
        setattr(pl, name + "_s", arr)
    return any_seq


def _scenario_refs(pl, specs, ref_traj):
    """pl.specs, pl.ref_traj (the shared reference, None when each scenario has its own),
    pl.ref_traj_s (n x 2 x n_ref x 5, a broadcast view of a shared one) and pl.n_ref; returns
    (the references to upload, whether they are per scenario).  ref_traj: 2 x n_ref x 5 for all,
    or n x 2 x n_ref x 5; without it the references of `specs`."""
    n = pl.n
    pl.specs = None if specs is None else [_spec(sp) for sp in specs]
    assert pl.specs is None or len(pl.specs) == n
    if ref_traj is None and pl.specs is not None:
        ref = np.stack([np.stack(ref_traj_gen(sp)) for sp in pl.specs]) if n else np.zeros((0, 2, 51, NX))
        pl.ref_traj = None
    else:
        pl.ref_traj = ref_traj_gen() if ref_traj is None else ref_traj
        ref = np.stack([np.asarray(r_, np.float64) for r_ in pl.ref_traj])
        if ref.ndim == 4:
            pl.ref_traj = None
    ref = np.ascontiguousarray(ref, np.float64)
    each = ref.ndim == 4
    assert ref.shape[-3] == 2 and ref.shape[-1] == NX and (not each or ref.shape[0] == n), ref.shape
    pl.n_ref = ref.shape[-2]
    pl.ref_traj_s = ref if each else np.broadcast_to(ref, (n,) + ref.shape)
    return ref, each


def _spec_of(pl, s):
    return None if pl.specs is None else pl.specs[s]


class OBCARunRecord:
    """state_record / iter_num_record / lambda_record as in the script (:18-20, :100-103), one
    entry per MPC step, stacked over scenarios; status_record keeps, per ADMM iterate, the
    scenarios submitted and every local / edge status (nothing is silent)."""

    def __init__(self):
        self.state_record = []
        self.iter_num_record = []
        self.lambda_record = []
        self.status_record = []


class OBCAPlanner:
    """The OBCA-ADMM overtaking planner on the GPU.  Per ADMM iterate, in the script's order: one
    local launch over all still-active scenarios x 2 vehicles (:49-63), bar_state_update (:66),
    check_converge (:67), one edge launch with the fused lambda_update (:71-79), the residuals
    (:82-85); a scenario stops at both residuals <= the thresholds or i_iter > max_admm_iter (:86)
    and is not resubmitted.  Then the horizon shift -- of the PREVIOUS iterate's bar_state, as :87
    is written -- and init_state = X[1] (:99).

    prob, primal_thres, dual_thres: one value or one per scenario.  update_lamb_ij: 0 leaves lamb_ij untouched (the
    commented-out :220), 1 takes each vehicle's local Lambda.  on_stage(name, inputs, outputs) sees
    every stage: "local", "exchange", "converge", "edge", "residual", "shift".

    Every parameter of FLEET_ROW is one value or one per scenario (`rho_s`, `min_dis_s`, ... keep
    the value of each scenario; the scalar attributes keep a scalar argument and are None for a
    sequence).  specs: one OvertakeSpec per scenario, giving its reference, init_state and seeded
    state; ref_traj: one reference (2 x n_ref x 5) or one per scenario (`ref_traj_s`).

    dual: None keeps lambda_update; dict(kP=, kI=, windup_sat=, d_gain=, windup=), each one value or
    one per scenario, replaces it by the PI anti-windup law (`lambda_update_pi`), the integrator
    shifted with the state (`shift_dual`).  OBCADevicePlanner takes the same argument.

    clock: None keeps the one step of all scenarios; n x 2 rows (c0, len), or True for everyone at
    t_step0 over the whole reference, gives every scenario its own step (`clock`, n x 3: c, len,
    alive, ticked by `clock_tick`): it is seeded at c0, reads its reference at c, and once
    c + 8 > len it is retired -- skipped by every later step, its state frozen, its stop iterate 0.

    feedback: None closes a step with init_state = X[1]; dict(par=, tape=) closes it through the
    plant instead (`propagate`): init_state = propagate(the closing step's init_state, the first
    control of the stopping local solution, par, tape[s][k]) with k the steps since the attachment.
    par: one plant row or n (`feedback_row`; None: the nominal plant), tape: n x cap x 2 x 5
    disturbance rows or None.  `measure` overwrites init_state with states measured outside.
    OBCADevicePlanner takes the same argument.  Not together with clock.

    noise: None, or dict(par=, streams=, seed=, k0=) on top of feedback: the disturbance of scenario
    s at the step k since the feedback's attachment is tape[s][k] (if any) plus the row
    `noise_tape` draws for stream streams[s] at step index k0 + k -- a pure function of (seed,
    stream, step index), so no tape is kept.  `set_noise` / `clear_noise` attach and detach it; a
    new `set_feedback` and `clear_feedback` drop it.  OBCADevicePlanner takes the same argument and
    draws the same disturbances (k_plan_noise).

    delay: None, or dict(par=, streams=, seed=, k0=, tape=): communication delay in the exchange.
    Vehicle v of scenario s sends, at every iterate of the step k since the attachment, the
    halfspaces and local_x of `stale_states(X, tau)` in place of its local states, with tau =
    `delay_tau`'s latency of stream streams[s] at step index k0 + k (tape n x cap x 2: recorded
    latencies added in front); what it keeps for itself (controls, X, init_state) is unchanged.
    `set_delay` / `clear_delay` attach and detach it; independent of feedback and noise, not together
    with clock.  OBCADevicePlanner takes the same argument (piadmm_obca_delay_plan)."""

    def __init__(self, batch, n_scenarios, prob=1, t_step0=0, rho=1.0, min_dis=0.1, max_admm_iter=50,
                 primal_thres=0.01, dual_thres=0.01, round_decimals=4, start=1, update_lamb_ij=0, max_iter=60,
                 conv_thres=0.1, on_stage=None, max_x=150.0, max_y=20.0, r=1e4, q=1e5, x_bound=1000.0,
                 mu_max=100000.0, g_max=1000.0, ref_traj=None, specs=None, dual=None, clock=None, feedback=None,
                 noise=None, delay=None):
        self.batch = batch
        self.n = int(n_scenarios)
        self.prob = [int(prob)] * self.n if np.isscalar(prob) else [int(p) for p in prob]
        assert len(self.prob) == self.n
        self.t_step = int(t_step0)
        self.rho = float(rho) if np.ndim(rho) == 0 else None
        self.min_dis = float(min_dis) if np.ndim(min_dis) == 0 else None
        self.max_admm_iter = int(max_admm_iter) if np.ndim(max_admm_iter) == 0 else None
        self.primal_thres = np.broadcast_to(np.asarray(primal_thres, np.float64), (self.n,)).copy()
        self.dual_thres = np.broadcast_to(np.asarray(dual_thres, np.float64), (self.n,)).copy()
        self.conv_thres = conv_thres if np.ndim(conv_thres) == 0 else None
        self.round_decimals, self.start, self.max_iter = (v if np.ndim(v) == 0 else None
                                                          for v in (round_decimals, start, max_iter))
        self.update_lamb_ij = update_lamb_ij
        _per_scenario(self, self.n, rho=rho, min_dis=min_dis, conv_thres=conv_thres, max_x=max_x, max_y=max_y, r=r,
                      q=q, x_bound=x_bound, mu_max=mu_max, g_max=g_max, max_admm_iter=max_admm_iter,
                      max_iter=max_iter, round_decimals=round_decimals, start=start)
        self.on_stage = on_stage or (lambda name, inputs, outputs: None)
        _scenario_refs(self, specs, ref_traj)
        self.clock = None
        if clock is not None:
            rows = clock_rows(self.n, clock, self.t_step, self.n_ref)
            assert (rows[:, 0] >= 0).all() and (rows[:, 1] <= self.n_ref).all() \
                and (rows[:, 0] + N_HORZ <= rows[:, 1]).all(), rows
            self.clock = np.concatenate((rows, np.ones((self.n, 1), np.int32)), axis=1)
        t0 = [self.t_step] * self.n if self.clock is None else [int(c) for c in self.clock[:, 0]]
        self.bar_prev = [seeded_bar_state(t0[s], p, spec=_spec_of(self, s)) for s, p in enumerate(self.prob)]
        self.init_state = [np.stack([executed_path(v, t0[s] * DT, _spec_of(self, s)) for v in (0, 1)])
                           for s in range(self.n)]
        self.lamb_last = [np.zeros((2, NT, 9)) for _ in range(self.n)]
        # the PI anti-windup dual law (dual=dict(kP=, kI=, windup_sat=, d_gain=, windup=), each one
        # value or one per scenario): S = lamb_bar, D = 0, as piadmm_obca_dual_plan attaches it
        self.dual_par = None if dual is None else dual_rows(self.n, dual)
        if dual is not None:
            self.dual_S = [b["lamb_bar"].copy() for b in self.bar_prev]
            self.dual_D = [np.zeros((2, NT, 9)) for _ in range(self.n)]
        self.feedback = None
        self.noise = None
        if feedback is not None:
            self.set_feedback(**feedback)
        if noise is not None:
            self.set_noise(**noise)
        self.delay = None
        if delay is not None:
            self.set_delay(**delay)
        self.record = OBCARunRecord()
        self.record.state_record.append(np.stack(self.init_state))

    def set_delay(self, par=None, streams=None, seed=0, k0=0, tape=None):
        """Attach the communication delay (see the class): from the next step on the exchange is
        stale.  The step count starts again."""
        from . import _lib
        delay = delay_args(self.n, par, streams, seed, k0, tape)
        if self.clock is not None:
            err = _lib.PiadmmError("obca_delay_plan: a clock is attached (obca_clock_plan: the delay counts the "
                                   "plan's steps, not per-scenario clocks)")
            err.code = _lib.E_STATE
            raise err
        self.delay = delay
        self._delay_steps = 0

    def clear_delay(self):
        self.delay = None

    def delay_tau(self):
        """The open step's latencies, n x 2 (the DELAY_TAU item of OBCADevicePlanner.get)."""
        assert self.delay is not None, "no delay attached"
        par, streams, seed, k0, tape = self.delay
        k = self._delay_steps
        assert tape is None or k < tape.shape[1], "latency tape exhausted"
        assert k0 + k < NOISE_K_MAX, "delay step index exhausted"
        return delay_tau(self.n, 1, par, streams, seed, k0 + k, None if tape is None else tape[:, k:k + 1])[:, 0]

    def set_feedback(self, par=None, tape=None):
        """Attach the plant (see the class): from the next step on a step closes through `propagate`.
        The step count starts again, so an attached noise is dropped."""
        assert self.clock is None, "feedback and clock do not go together"
        self.feedback = feedback_args(self.n, dict(par=par, tape=tape))
        self._feedback_steps = 0
        self.noise = None

    def clear_feedback(self):
        self.feedback = None
        self.noise = None

    def set_noise(self, par=None, streams=None, seed=0, k0=0):
        """Attach the noise (see the class; feedback must be attached, as piadmm_obca_noise_plan
        refuses without it)."""
        from . import _lib
        noise = noise_args(self.n, par, streams, seed, k0)
        if self.feedback is None:
            err = _lib.PiadmmError("obca_noise_plan: no feedback attached (obca_feedback_plan: the noise enters "
                                   "through the plant step)")
            err.code = _lib.E_STATE
            raise err
        self.noise = noise

    def clear_noise(self):
        self.noise = None

    def feedback_steps(self):
        """The steps closed since the attachment."""
        assert self.feedback is not None, "no feedback attached"
        return self._feedback_steps

    def measure(self, slots, states):
        """init_state of the scenarios `slots` = the measured `states` (m x 2 x 5); nothing else changes."""
        states = np.asarray(states, np.float64)
        assert states.shape == (len(slots), 2, NX) and np.isfinite(states).all(), states.shape
        self.init_state = list(self.init_state)
        for k, s in enumerate(slots):
            self.init_state[int(s)] = states[k].copy()

    @staticmethod
    def _copy(bar):
        return {k: v.copy() for k, v in bar.items()}

    def step(self):
        """One MPC step of every scenario."""
        n = self.n
        if self.feedback is not None and self.feedback[1] is not None:
            assert self._feedback_steps < self.feedback[1].shape[1], "disturbance tape exhausted"
        if self.clock is None:
            assert self.t_step + N_HORZ <= self.n_ref, "reference exhausted"
            ran = list(range(n))
            t_of = [self.t_step] * n
        else:
            # every scenario at its own step; the retired ones are skipped
            ran = [s for s in range(n) if self.clock[s, 2]]
            assert ran, "no scenario alive"
            t_of = [int(c) for c in self.clock[:, 0]]
        tau = None if self.delay is None else self.delay_tau()
        bar = [self._copy(b) for b in self.bar_prev]
        bar_prev = [self._copy(b) for b in self.bar_prev]
        x0_step = [np.array(x, np.float64) for x in self.init_state]
        ctrl_prev = [np.zeros((2, NT * NU)) for _ in range(n)]
        X = [None] * n
        U0 = [None] * n
        iters = np.zeros(n, int)
        shift_in = [None] * n
        active = list(ran)
        i_iter = 0
        while active:
            i_iter += 1
            # ---- vehicle side: one launch, scenarios x vehicles ----
            recs = np.ascontiguousarray(np.stack([
                local_record(bar[s], v, t_of[s], self.init_state[s][v], self.ref_traj_s[s], rho=self.rho_s[s],
                             min_dis=self.min_dis_s[s], prob=self.prob[s], max_x=self.max_x_s[s],
                             max_y=self.max_y_s[s], r=self.r_s[s], q=self.q_s[s], max_iter=self.max_iter_s[s])
                for s in active for v in (0, 1)]))
            res = self.batch.solve(recs)
            self.on_stage("local", dict(recs=recs, scenarios=list(active), i_iter=i_iter, t_step=self.t_step),
                          dict(result=res))
            fullx = [[res.bar_fullx(2 * k + v) for v in (0, 1)] for k in range(len(active))]
            ctrl = [np.stack([np.append(res.U[2 * k + v][:, 0], res.U[2 * k + v][:, 1]) for v in (0, 1)])
                    for k in range(len(active))]
            for k, s in enumerate(active):
                X[s] = [res.X[2 * k].copy(), res.X[2 * k + 1].copy()]
                U0[s] = np.stack([res.U[2 * k + v][0] for v in (0, 1)])
            # ---- information exchange ----
            before = [bar[s] for s in active]
            for k, s in enumerate(active):
                if tau is None:
                    bar[s] = bar_state_update(bar[s], fullx[k], prob=self.prob[s])
                else:
                    bar[s] = bar_state_update(bar[s], fullx[k], prob=self.prob[s], tau=tau[s],
                                              fullX=[res.X[2 * k + v] for v in (0, 1)])
                if self.update_lamb_ij:
                    bar[s]["lamb_ij"] = np.stack([fullx[k][v][:, 5:] for v in (0, 1)])
            self.on_stage("exchange", dict(bar=before, fullx=fullx, scenarios=list(active)),
                          dict(bar=[self._copy(bar[s]) for s in active]))
            conv = [check_converge(bar[s], self.conv_thres_s[s], self.min_dis_s[s]) for s in active]
            self.on_stage("converge", dict(bar=[self._copy(bar[s]) for s in active]), dict(if_converge=conv))
            # ---- RSU side: one launch, the dual update fused ----
            erecs = np.ascontiguousarray(np.stack([
                edge_record(bar[s], rho=self.rho_s[s], min_dis=self.min_dis_s[s], prob=self.prob[s],
                            max_iter=self.max_iter_s[s], round_decimals=self.round_decimals_s[s],
                            start=self.start_s[s], x_bound=self.x_bound_s[s], mu_max=self.mu_max_s[s],
                            g_max=self.g_max_s[s]) for s in active]))
            eres = self.batch.solve_edge(erecs)
            self.on_stage("edge", dict(recs=erecs, scenarios=list(active)), dict(result=eres))
            lamb_prev = [bar[s]["lamb_bar"].copy() for s in active]
            if self.dual_par is None:
                for k, s in enumerate(active):
                    bar[s]["Z_bar"] = eres.Z_bar[k].copy()
                    bar[s]["lamb_bar"] = eres.lamb_bar[k].copy()
            else:
                # the law instead of the fused update: the integrator before this iterate is the
                # one the previous iterate's bar_state corresponds to (B16)
                dual_before = {s: (self.dual_S[s], self.dual_D[s]) for s in active}
                dres_pi = np.zeros((len(active), NT))
                for k, s in enumerate(active):
                    bar[s]["Z_bar"] = eres.Z_bar[k].copy()
                    wrote = [int(c) in EDGE_WRITES_ITERATE for c in eres.status[k]]
                    bar[s], self.dual_S[s], self.dual_D[s], dres_pi[k] = lambda_update_pi(
                        bar[s], self.dual_S[s], self.dual_D[s], self.dual_par[s % len(self.dual_par)], wrote)
            self.record.status_record.append(dict(t_step=self.t_step, i_iter=i_iter, scenarios=list(active),
                                                  local_status=res.status.copy(), edge_status=eres.status.copy(),
                                                  if_converge=conv))
            # ---- residuals (:82-86) ----
            primal = np.array([np.abs(ctrl[k] - ctrl_prev[s]).sum() for k, s in enumerate(active)])
            if self.dual_par is None:
                dual = eres.dual_residual()
            else:
                dual = np.zeros(len(active))
                for t in range(NT):
                    dual = dual + dres_pi[:, t]
            stop = ((primal <= self.primal_thres[active]) & (dual <= self.dual_thres[active])) \
                | (i_iter > self.max_admm_iter_s[active])
            self.on_stage("residual",
                          dict(ctrl=ctrl, ctrl_prev=[ctrl_prev[s] for s in active],
                               lamb_bar=[bar[s]["lamb_bar"] for s in active], lamb_bar_prev=lamb_prev, i_iter=i_iter,
                               scenarios=list(active)),
                          dict(primal=primal, dual=dual, stop=stop))
            nxt = []
            for k, s in enumerate(active):
                if stop[k]:
                    iters[s] = i_iter
                    shift_in[s] = bar_prev[s]           # :87: the previous iterate's bar_state (B16)
                    if self.dual_par is not None:
                        self.dual_S[s], self.dual_D[s] = dual_before[s]
                else:
                    bar_prev[s] = self._copy(bar[s])
                    ctrl_prev[s] = ctrl[k]
                    nxt.append(s)
            active = nxt
        # ---- next time step (:87, :99-103): of the scenarios this step ran ----
        self.bar_prev, self.init_state = list(self.bar_prev), list(self.init_state)
        for s in ran:
            self.bar_prev[s] = iterate_next_state(shift_in[s])
            if self.dual_par is not None:
                self.dual_S[s], self.dual_D[s] = shift_dual(self.dual_S[s], self.dual_D[s])
            self.init_state[s] = np.stack([X[s][0][1], X[s][1][1]])
            self.lamb_last[s] = bar[s]["lamb_bar"]
        if self.feedback is not None:
            # the vehicle instead of the prediction: from the closing step's init_state under the
            # stopping solution's first control (every scenario ran: no clock with feedback)
            par, tape = self.feedback
            w = None if tape is None else tape[:, self._feedback_steps]
            if self.noise is not None:
                # the step's row of every stream, the tape's row in front
                zpar, streams, seed, k0 = self.noise
                wn = noise_tape(n, 1, zpar, streams, seed, k0 + self._feedback_steps)[:, 0]
                w = wn if w is None else w + wn
            nxt = propagate(np.stack(x0_step), np.stack(U0), par, w)
            self.init_state = [nxt[s] for s in range(n)]
            self._feedback_steps += 1
        if self.delay is not None:
            self._delay_steps += 1
        self.on_stage("shift", dict(bar_prev=shift_in, X=X, iters=iters.copy()), dict(bar_next=self.bar_prev, init_state=self.init_state))
        self.record.state_record.append(np.stack(self.init_state))
        self.record.iter_num_record.append(iters)
        self.record.lambda_record.append(np.stack(self.lamb_last))
        if self.clock is not None:
            self.clock = clock_tick(self.clock, self.clock[:, 2])
        self.t_step += 1

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            if self.clock is not None and not self.clock[:, 2].any():
                break
            self.step()
        return self.record


# ---------------------------------------------------------------------------------------------
# The same loop, device-resident (csrc/piadmm_obca_plan.hip behind piadmm_obca_plan_*)
# ---------------------------------------------------------------------------------------------
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


# ---------------------------------------------------------------------------------------------
# Fleet risk statistics and the worst-case gather of a run record (piadmm_obca_fleet_stats,
# piadmm_obca_stats_trace, piadmm_obca_gather_trace; include/piadmm.h), in NumPy
# ---------------------------------------------------------------------------------------------
STATS_EDGES = 64                      # PIADMM_OBCA_STATS_EDGES: the most edges
STATS_WORST = 64                      # PIADMM_OBCA_STATS_WORST: the most worst scenarios
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
    from . import _lib
    edges = np.ascontiguousarray(np.asarray(edges, np.float64).reshape(-1))
    B, K = len(edges), int(K)
    st = _lib.ObcaStatsC()
    hist = np.zeros((2, B + 1), np.int64)
    row_min, row_arg = np.zeros((R + 1, 2)), np.zeros((R + 1, 2), np.int32)
    row_below, worst = np.zeros((R + 1, 2, B), np.int32), np.zeros(max(K, 0), np.int32)
    # the library refuses what is out of range; the arrays only have to exist
    rc = call(_lib.dptr(edges) if B else None, B, K, ctypes.byref(st),
              hist.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)), _lib.dptr(row_min), _lib.iptr(row_arg),
              _lib.iptr(row_below) if B else None, _lib.iptr(worst) if K > 0 else None)
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


# ---------------------------------------------------------------------------------------------
# The tenant record of piadmm_obca_tenant_export / _import (include/piadmm.h), in NumPy
# ---------------------------------------------------------------------------------------------
TENANT_MAGIC = 0x314E5454
TENANT_ABI = 7
TENANT_HEADER = 64                    # bytes: sixteen int32
TENANT_INTS = 12                      # int32 words behind the fp64 section of a record
TENANT_F64 = 1474                     # fp64 words of a record, + 10 n_ref, + TENANT_F64_LAW with a law
TENANT_F64_LAW = 512
# the int32 section: name -> (first word, words)
TENANT_INT_FIELDS = {"ITERS": (0, 1), "STOP": (1, 1), "CONVERGE": (2, 1), "PROB": (3, 1), "STATUS_MASK": (4, 2),
                     "WORK": (6, 2), "CLOCK": (8, 3)}
_TENANT_SHAPES = {"STATE": (PLAN_STATE,), "STATE_PREV": (PLAN_STATE,), "CTRL": (2, NT * NU), "CTRL_PREV": (2, NT * NU),
                  "X": (2, N_HORZ, NX), "LAMBDA": (2, NT, 9), "PRIMAL": (), "DUAL": (), "PRIMAL_THRES": (),
                  "DUAL_THRES": (), "PAR": (FLEET_PAR,), "WINDOW": (2, N_HORZ, NX), "DUAL_S": (2, NT, 9),
                  "DUAL_D": (2, NT, 9), "DUAL_S_PREV": (2, NT, 9), "DUAL_D_PREV": (2, NT, 9), "DUAL_PAR": (DUAL_PAR,),
                  "ITERS": (), "STOP": (), "CONVERGE": (), "PROB": (), "STATUS_MASK": (2,), "WORK": (2,), "CLOCK": (3,)}


def tenant_layout(n_ref, law=False):
    """The layout of one tenant record: dict(f64={name: (first fp64 word, words)}, F=the fp64 words,
    ints=TENANT_INT_FIELDS, record_bytes=8 F + 48), as the table of include/piadmm.h has it."""
    fields = [("STATE", PLAN_STATE), ("STATE_PREV", PLAN_STATE), ("CTRL", 28), ("CTRL_PREV", 28), ("X", 80),
              ("LAMBDA", 126), ("PRIMAL", 1), ("DUAL", 1), ("PRIMAL_THRES", 1), ("DUAL_THRES", 1), ("PAR", FLEET_PAR),
              ("REF", 10 * int(n_ref)), ("WINDOW", 80)]
    if law:
        fields += [("DUAL_S", 126), ("DUAL_D", 126), ("DUAL_S_PREV", 126), ("DUAL_D_PREV", 126), ("DUAL_PAR", DUAL_PAR)]
    f64, o = {}, 0
    for name, words in fields:
        f64[name] = (o, words)
        o += words
    assert o == TENANT_F64 + 10 * int(n_ref) + (TENANT_F64_LAW if law else 0)
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


def tenant_pack(items, slots, n_ref, update_lamb_ij=0, t_step=0):
    """The blob piadmm_obca_tenant_export writes for the scenarios `slots`, from the plan's
    piadmm_obca_plan_get items (name -> array over all n scenarios): STATE, STATE_PREV, CTRL,
    CTRL_PREV, X, LAMBDA, PRIMAL, DUAL, PRIMAL_THRES, DUAL_THRES, PAR, REF, ITERS, STOP, CONVERGE, PROB,
    STATUS_MASK; with a law DUAL_S, DUAL_D, DUAL_S_PREV, DUAL_D_PREV and DUAL_PAR; with the order WORK;
    with a clock CLOCK and WINDOW.  PAR, REF and DUAL_PAR of one row are shared: the row goes into
    every record.  Without CLOCK the record's clock is (t_step, n_ref, 1) and its window the 8
    reference rows at t_step (zeros past the end).  Returns a uint8 array."""
    slots = [int(s) for s in np.asarray(slots).reshape(-1)]
    m, n_ref = len(slots), int(n_ref)
    law, order, clocked = "DUAL_S" in items, "WORK" in items, "CLOCK" in items
    lay = tenant_layout(n_ref, law)
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
    body = np.concatenate((f64.view(np.uint8).reshape(m, -1), ints.view(np.uint8).reshape(m, -1)), axis=1)
    return np.concatenate((hdr.view(np.uint8), body.reshape(-1)))


def tenant_unpack(blob):
    """The tenants of a blob: dict(m, n_ref, update_lamb_ij, law, order, and per field of the record an
    array over the m tenants -- copies).  ValueError for what piadmm_obca_tenant_import refuses of the
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
    if m < 1 or n_ref < N_HORZ or ulij not in (0, 1) or law not in (0, 1) or order not in (0, 1) or hdr[11:].any():
        raise ValueError("tenant blob: bad header (counts or flags)")
    lay = tenant_layout(n_ref, bool(law))
    if (F, n_int, rec_bytes, hdr_bytes) != (lay["F"], TENANT_INTS, lay["record_bytes"], TENANT_HEADER):
        raise ValueError("tenant blob: bad header (section sizes)")
    if raw.size != TENANT_HEADER + m * rec_bytes:
        raise ValueError(f"tenant blob: {raw.size} bytes, not the {TENANT_HEADER + m * rec_bytes} of its header (truncated?)")
    body = raw[TENANT_HEADER:].reshape(m, rec_bytes)
    f64 = np.ascontiguousarray(body[:, :8 * F]).view(np.float64).reshape(m, F)
    ints = np.ascontiguousarray(body[:, 8 * F:]).view(np.int32).reshape(m, TENANT_INTS)
    out = dict(m=m, n_ref=n_ref, update_lamb_ij=ulij, law=bool(law), order=bool(order))
    for name, (o, words) in lay["f64"].items():
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
        if why is not None:
            raise ValueError(f"tenant blob: row {k}: {why}")
    return out


class OBCADevicePlanner:
    """`OBCAPlanner` with the loop on the device: the planner state stays resident on the batch's
    handle and one ADMM iterate is a fixed chain of launches (csrc/piadmm_obca_plan.hip); the host
    reads back the number of scenarios still active.  Same constructor arguments, same seeding
    (`seeded_bar_state`, `executed_path`) and the same OBCARunRecord fields as OBCAPlanner.

    Without on_stage a step is one `piadmm_obca_plan_step`; status_record then keeps one entry per
    MPC step: the iterate each scenario stopped at and, per scenario, the OR of (1 << status) over
    its local and its edge solves (nothing is silent).  With on_stage the step goes iterate by
    iterate, the callback sees the six stages of OBCAPlanner built from `get`, and status_record
    keeps one entry per iterate as OBCAPlanner's does.

    The planner takes the batch's device buffers over (include/piadmm.h): `batch.upload` / `solve`
    / `solve_edge` on the same batch end the plan.

    With `specs`, a reference per scenario (ref_traj n x 2 x n_ref x 5) or a sequence for any
    parameter of FLEET_ROW the plan is a fleet (`self.fleet`): it is opened by
    piadmm_obca_fleet_begin with one reference and one parameter row (`par`) per scenario.
    Otherwise it is opened by piadmm_obca_plan_begin, as ever.

    With order=True every active list is kept longest first by the work of each scenario's last
    solves (piadmm_obca_order_plan; `work_init` n x 2 seeds the record, `work()` reads it): the
    per-scenario results are the same bit for bit, ACTIVE and the LOCAL_ / EDGE_ items follow the
    list's order.

    With clock= every scenario has its own MPC step and reference length (piadmm_obca_clock_plan):
    clock is n x 2 rows (c0, len), or True for everyone at t_step0 over the whole reference.
    Scenario s is seeded at its own c0 and reads its reference at its own step; once c + 8 > len it
    is retired and frozen while the others go on.  `clock()` reads the record, `admit` puts new
    tenants into slots, `run` / `run_traced` stop when nothing is alive.  t_step counts the plan's
    steps.

    Running tenants move as records (piadmm_obca_tenant_export / _import): `export_tenants` of any
    plan, `import_tenants` into a clocked fleet plan, `compact()` for a new planner with the alive
    tenants only, `save` / `load` for a checkpoint of the whole plan; a moved tenant continues bit
    for bit.

    With feedback=dict(par=, tape=) a step closes through a plant instead of with init_state = X[1]
    (piadmm_obca_feedback_plan, `propagate`): par one plant row or n (`feedback_row`; None: the
    nominal plant), tape n x cap x 2 x 5 disturbance rows or None.  `set_feedback` / `clear_feedback`
    attach and detach it at a step boundary, `feedback_steps()` counts the steps closed since,
    `measure(slots, states)` writes states measured outside over init_state
    (piadmm_obca_feedback_measure; any plan, no trace).  `run_traced` works with it unchanged: the
    trace's states and clearances are those of the states the vehicles reached.  Not together with
    clock or the tenant calls.

    With noise=dict(par=, streams=, seed=, k0=) on top of feedback the disturbance is drawn on the
    device (piadmm_obca_noise_plan, k_plan_noise; `noise_tape` is the statement): scenario s at the
    step k since the feedback's attachment gets the row of stream streams[s] (None: s) at step index
    k0 + k, added behind the tape's row if there is a tape.  `set_noise` / `clear_noise` attach and
    detach it; `set_feedback` and `clear_feedback` drop it.  A scenario is re-run alone from (seed,
    its stream id, k0): a plan of the worst few with streams = their ids draws what they drew.

    With delay=dict(par=, streams=, seed=, k0=, tape=) the exchange is stale (piadmm_obca_delay_plan,
    k_plan_delay and k_plan_exchange_stale; `delay_tau` and `stale_states` are the statements): every
    vehicle sends the halfspaces of its plan interpolated back by its latency of the open step,
    `get("DELAY_TAU")`.  `set_delay` / `clear_delay` attach and detach it at a step boundary;
    independent of feedback and noise, not together with clock or the tenant calls."""

    def __init__(self, batch, n_scenarios, prob=1, t_step0=0, rho=1.0, min_dis=0.1, max_admm_iter=50,
                 primal_thres=0.01, dual_thres=0.01, round_decimals=4, start=1, update_lamb_ij=0, max_iter=60,
                 conv_thres=0.1, on_stage=None, max_x=150.0, max_y=20.0, r=1e4, q=1e5, x_bound=1000.0,
                 mu_max=100000.0, g_max=1000.0, ref_traj=None, state=None, specs=None, dual=None, order=False,
                 work_init=None, clock=None, feedback=None, noise=None, delay=None):
        from . import _lib
        self.batch = batch
        self._lib = batch._lib
        self.n = int(n_scenarios)
        self.prob = [int(prob)] * self.n if np.isscalar(prob) else [int(p) for p in prob]
        assert len(self.prob) == self.n
        self.t_step = int(t_step0)
        self.rho = float(rho) if np.ndim(rho) == 0 else None
        self.min_dis = float(min_dis) if np.ndim(min_dis) == 0 else None
        self.max_admm_iter = int(max_admm_iter) if np.ndim(max_admm_iter) == 0 else None
        self.primal_thres = np.broadcast_to(np.asarray(primal_thres, np.float64), (self.n,)).copy()
        self.dual_thres = np.broadcast_to(np.asarray(dual_thres, np.float64), (self.n,)).copy()
        self.conv_thres = conv_thres if np.ndim(conv_thres) == 0 else None
        self.round_decimals, self.start, self.max_iter = (v if np.ndim(v) == 0 else None
                                                          for v in (round_decimals, start, max_iter))
        self.update_lamb_ij = update_lamb_ij
        any_seq = _per_scenario(self, self.n, rho=rho, min_dis=min_dis, conv_thres=conv_thres, max_x=max_x,
                                max_y=max_y, r=r, q=q, x_bound=x_bound, mu_max=mu_max, g_max=g_max,
                                max_admm_iter=max_admm_iter, max_iter=max_iter, round_decimals=round_decimals,
                                start=start)
        self.on_stage = on_stage
        ref, ref_each = _scenario_refs(self, specs, ref_traj)
        self.fleet = bool(any_seq or ref_each or self.specs is not None)
        # every scenario is seeded at the step it starts at: its own c0 with a clock
        rows = None if clock is None else clock_rows(self.n, clock, self.t_step, self.n_ref)
        t0 = [self.t_step] * self.n if rows is None else [int(c) for c in rows[:, 0]]
        self.init_state = [np.stack([executed_path(v, t0[s] * DT, _spec_of(self, s)) for v in (0, 1)])
                           for s in range(self.n)]
        if state is None:
            seeds = {}
            for s, p in enumerate(self.prob):
                key = (p, _spec_of(self, s), t0[s])
                if key not in seeds:
                    seeds[key] = pack_state(seeded_bar_state(t0[s], p, spec=key[1]), self.init_state[s])
            state = (np.stack([seeds[(p, _spec_of(self, s), t0[s])] for s, p in enumerate(self.prob)]) if self.n
                     else np.zeros((0, PLAN_STATE)))
        state = np.ascontiguousarray(state, np.float64)
        assert state.shape == (self.n, PLAN_STATE)
        prob_a = np.ascontiguousarray(self.prob if self.n else [0], np.int32)
        if not self.fleet:
            self.par = None
            self.cfg = _lib.ObcaPlanCfgC(
                n_scenarios=self.n, t_step0=self.t_step, max_admm_iter=self.max_admm_iter,
                round_decimals=int(round_decimals), start=int(start), update_lamb_ij=int(update_lamb_ij),
                max_sqp_iter=int(max_iter), n_ref=self.n_ref, rho=self.rho, min_dis=self.min_dis,
                conv_thres=float(conv_thres), max_x=max_x, max_y=max_y, r=r, q=q, x_bound=x_bound, mu_max=mu_max,
                g_max=g_max)
            self._check(self._lib.piadmm_obca_plan_begin(batch._h, ctypes.byref(self.cfg), _lib.iptr(prob_a),
                                                         _lib.dptr(self.primal_thres), _lib.dptr(self.dual_thres),
                                                         _lib.dptr(ref), _lib.dptr(state)))
        else:
            # cfg carries what stays shared; the rows carry the rest
            self.par = np.zeros((self.n, FLEET_PAR))
            for j, name in enumerate(FLEET_ROW):
                self.par[:, j] = getattr(self, name + "_s")
            if not ref_each:
                ref = np.ascontiguousarray(self.ref_traj_s)
            self.cfg = _lib.ObcaPlanCfgC(n_scenarios=self.n, t_step0=self.t_step, update_lamb_ij=int(update_lamb_ij),
                                         n_ref=self.n_ref)
            self._check(self._lib.piadmm_obca_fleet_begin(batch._h, ctypes.byref(self.cfg), _lib.iptr(prob_a),
                                                          _lib.dptr(self.primal_thres), _lib.dptr(self.dual_thres),
                                                          _lib.dptr(ref), _lib.dptr(self.par), _lib.dptr(state)))
        self.dual_par = None
        self._feedback = None
        self._noise = None
        self._delay = None
        if dual is not None:
            self.set_dual(**dual)
        self.order = False
        if order:
            self.set_order(work_init)
        else:
            assert work_init is None, "work_init seeds the order's record: pass order=True"
        self._clock = None
        if clock is not None:
            self.set_clock(None if clock is True else rows)
        if feedback is not None:
            self.set_feedback(**feedback)
        if noise is not None:
            self.set_noise(**noise)
        if delay is not None:
            self.set_delay(**delay)
        self.record = OBCARunRecord()
        self.record.state_record.append(np.stack(self.init_state))

    def set_delay(self, par=None, streams=None, seed=0, k0=0, tape=None):
        """Attach the communication delay (piadmm_obca_delay_plan; a step boundary only, no clock):
        par one delay row or n rows (`delay_row`; None: the default row), streams n stream ids (None:
        0 .. n-1), seed a uint64, k0 the step index of the open step, tape n x cap x 2 recorded
        latencies or None.  A second call replaces the first.  The library checks the arguments."""
        from . import _lib
        rows = np.ascontiguousarray(np.asarray(delay_row() if par is None else par, np.float64).reshape(-1, DELAY_PAR))
        if streams is not None:
            streams = np.ascontiguousarray(streams, np.int64).reshape(-1)
            assert streams.shape == (self.n,), streams.shape
        if tape is not None:
            tape = np.ascontiguousarray(tape, np.float64)
            assert tape.ndim == 3 and tape.shape[0] == self.n and tape.shape[2] == 2, tape.shape
        self._check(self._lib.piadmm_obca_delay_plan(
            self.batch._h, 1, _lib.dptr(rows), rows.shape[0],
            None if streams is None else streams.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            ctypes.c_uint64(int(seed)), int(k0), _lib.dptr(tape), 0 if tape is None else tape.shape[1]))
        self._delay = (rows, streams, int(seed), int(k0), tape)

    def clear_delay(self):
        """Detach the delay (a step boundary only): the exchange is the plain one again."""
        self._check(self._lib.piadmm_obca_delay_plan(self.batch._h, 0, None, 0, None, 0, 0, None, 0))
        self._delay = None

    def set_feedback(self, par=None, tape=None):
        """Attach the plant (piadmm_obca_feedback_plan; a step boundary only, no clock): par one plant
        row or n rows (None: the nominal plant), tape n x cap x 2 x 5 disturbance rows or None.  A
        second call replaces the first and starts its tape again; an attached noise is dropped."""
        from . import _lib
        rows, tape = feedback_args(self.n, dict(par=par, tape=tape))
        self._check(self._lib.piadmm_obca_feedback_plan(self.batch._h, 1, None if par is None else _lib.dptr(rows),
                                                        rows.shape[0], _lib.dptr(tape),
                                                        0 if tape is None else tape.shape[1]))
        self._feedback = (rows, tape)
        self._noise = None

    def clear_feedback(self):
        """Detach the plant (a step boundary only): a step closes with init_state = X[1] again.  An
        attached noise goes with it."""
        self._check(self._lib.piadmm_obca_feedback_plan(self.batch._h, 0, None, 0, None, 0))
        self._feedback = None
        self._noise = None

    def set_noise(self, par=None, streams=None, seed=0, k0=0):
        """Attach the device-side noise (piadmm_obca_noise_plan; a step boundary only, feedback
        attached): par one noise row or n rows (`noise_row`; None: the zero row), streams n stream ids
        (None: 0 .. n-1), seed a uint64, k0 the step index of the feedback's step 0.  A second call
        replaces the first.  The library checks the arguments."""
        from . import _lib
        rows = np.ascontiguousarray(np.asarray(noise_row() if par is None else par, np.float64).reshape(-1, NOISE_PAR))
        if streams is not None:
            streams = np.ascontiguousarray(streams, np.int64).reshape(-1)
            assert streams.shape == (self.n,), streams.shape
        self._check(self._lib.piadmm_obca_noise_plan(
            self.batch._h, 1, _lib.dptr(rows), rows.shape[0],
            None if streams is None else streams.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            ctypes.c_uint64(int(seed)), int(k0)))
        self._noise = (rows, streams, int(seed), int(k0))

    def clear_noise(self):
        """Detach the noise (a step boundary only): the tape alone, or nothing, disturbs the plant."""
        self._check(self._lib.piadmm_obca_noise_plan(self.batch._h, 0, None, 0, None, 0, 0))
        self._noise = None

    def feedback_steps(self):
        """The steps closed since the attachment (PLAN_GET FEEDBACK_STEPS)."""
        return int(self.get("FEEDBACK_STEPS")[0])

    def measure(self, slots, states):
        """init_state of both state copies of the scenarios `slots` (ascending, distinct) = the
        measured `states` (m x 2 x 5), one scatter launch (piadmm_obca_feedback_measure; a step
        boundary, no trace); nothing else changes."""
        from . import _lib
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        states = np.ascontiguousarray(states, np.float64)
        assert states.shape == (len(slots), 2, NX), states.shape
        self._check(self._lib.piadmm_obca_feedback_measure(self.batch._h, len(slots), _lib.iptr(slots),
                                                           _lib.dptr(states)))
        self.init_state = list(self.init_state)
        for k, s in enumerate(slots):
            self.init_state[int(s)] = states[k].copy()

    def set_clock(self, clock_init=None):
        """Attach the per-scenario clocks (piadmm_obca_clock_plan; a step boundary only): clock_init
        n x 2 rows (c0, len), or None for everyone at the plan's step over the whole reference."""
        from . import _lib
        t_plan = int(self.get("T_STEP")[0])
        rows = clock_rows(self.n, True if clock_init is None else clock_init, t_plan, self.n_ref)
        self._check(self._lib.piadmm_obca_clock_plan(self.batch._h, 1, None if clock_init is None else _lib.iptr(rows)))
        self._clock = np.concatenate((rows, np.ones((self.n, 1), np.int32)), axis=1)

    def clear_clock(self):
        """Detach the clocks (a step boundary only; every scenario alive, on one step, over the whole
        reference): the plan is plain again at that step."""
        self._check(self._lib.piadmm_obca_clock_plan(self.batch._h, 0, None))
        if self._clock is not None:
            self.t_step = int(self._clock[0, 0])
        self._clock = None

    def clock(self):
        """The record (c, len, alive) per scenario, n x 3 (PLAN_GET CLOCK)."""
        return self.get("CLOCK")

    def alive(self):
        """The scenarios the next step runs: every one without a clock, else the alive ones."""
        return np.ones(self.n, bool) if self._clock is None else self._clock[:, 2].astype(bool)

    def admit(self, slots, clock, state=None, ref=None, par=None, prob=None, primal_thres=None, dual_thres=None,
              specs=None):
        """New tenants into `slots` of the clocked plan (piadmm_obca_clock_admit; a step boundary, no
        trace): clock m x 2 rows (c0, len); state m x 556, ref m x 2 x n_ref x 5, par m x FLEET_PAR,
        prob, primal_thres, dual_thres m each -- None keeps what the slot has.  With specs= (one
        OvertakeSpec per tenant) a missing ref is the spec's reference and a missing state the
        state seeded at the tenant's c0, as the constructor seeds it."""
        from . import _lib
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        m = len(slots)
        clock = np.ascontiguousarray(clock, np.int32)
        assert clock.shape == (m, 2), clock.shape
        if prob is not None:
            prob = np.ascontiguousarray(np.broadcast_to(np.asarray(prob, np.int32), (m,)))
        if specs is not None:
            specs = [_spec(sp) for sp in specs]
            assert len(specs) == m
            if ref is None:
                ref = np.stack([np.stack(ref_traj_gen(sp)) for sp in specs])
            if state is None:
                pr = [self.prob[s] for s in slots] if prob is None else prob
                state = np.stack([pack_state(seeded_bar_state(int(c), int(p_), spec=sp),
                                             np.stack([executed_path(v, int(c) * DT, sp) for v in (0, 1)]))
                                  for sp, c, p_ in zip(specs, clock[:, 0], pr)])

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float64)
            assert a.shape == shape, (a.shape, shape)
            return a
        state, ref = arr(state, (m, PLAN_STATE)), arr(ref, (m, 2, self.n_ref, NX))
        par = arr(par, (m, FLEET_PAR))
        primal_thres, dual_thres = arr(primal_thres, (m,)), arr(dual_thres, (m,))
        self._check(self._lib.piadmm_obca_clock_admit(self.batch._h, m, _lib.iptr(slots), _lib.iptr(clock),
                                                      _lib.dptr(state), _lib.dptr(ref), _lib.dptr(par), _lib.iptr(prob),
                                                      _lib.dptr(primal_thres), _lib.dptr(dual_thres)))
        # the host's copies of what the slots now hold
        self._clock[slots, :2] = clock
        self._clock[slots, 2] = 1
        if ref is not None:
            self.ref_traj_s = np.array(self.ref_traj_s)
            self.ref_traj_s[slots] = ref
            self.ref_traj = None
        for k, s in enumerate(slots):
            if state is not None:
                self.init_state[s] = unpack_state(state[k])[1]
            if prob is not None:
                self.prob[s] = int(prob[k])
            if primal_thres is not None:
                self.primal_thres[s] = primal_thres[k]
            if dual_thres is not None:
                self.dual_thres[s] = dual_thres[k]
            if par is not None:
                self.par[s] = par[k]
                for j, name in enumerate(FLEET_ROW):
                    col = getattr(self, name + "_s").astype(np.float64)
                    col[s] = par[k, j]
                    setattr(self, name + "_s", col)
            if specs is not None and self.specs is not None:
                self.specs[s] = specs[k]

    # -- running tenants: export, import, compaction, checkpoints (piadmm_obca_tenant_export / _import) --
    TENANT_ITEMS = ("STATE", "STATE_PREV", "CTRL", "CTRL_PREV", "X", "LAMBDA", "PRIMAL", "DUAL", "PRIMAL_THRES",
                    "DUAL_THRES", "PAR", "REF", "ITERS", "STOP", "CONVERGE", "PROB", "STATUS_MASK")

    def tenant_items(self):
        """Every piadmm_obca_plan_get item a tenant record holds, by name: what `tenant_pack` takes."""
        names = self.TENANT_ITEMS
        if self.dual_par is not None:
            names += ("DUAL_S", "DUAL_D", "DUAL_S_PREV", "DUAL_D_PREV", "DUAL_PAR")
        if self.order:
            names += ("WORK",)
        if self._clock is not None:
            names += ("CLOCK", "WINDOW")
        return {k: self.get(k) for k in names}

    def export_tenants(self, slots) -> bytes:
        """The running tenants in `slots` as one blob (piadmm_obca_tenant_export; a step boundary only):
        `tenant_unpack` reads it, `import_tenants` of any clocked fleet plan with the same n_ref,
        update_lamb_ij, law and order continues them bit for bit.  The plan is not changed."""
        from . import _lib
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        size = ctypes.c_int64()
        self._check(self._lib.piadmm_obca_tenant_export_bytes(self.batch._h, len(slots), ctypes.byref(size)))
        blob = np.zeros(size.value, np.uint8)
        self._check(self._lib.piadmm_obca_tenant_export(self.batch._h, len(slots), _lib.iptr(slots), blob.ctypes.data,
                                                      blob.nbytes))
        return blob.tobytes()

    def import_tenants(self, slots, tenants):
        """The tenants of a blob of `export_tenants` into `slots` (piadmm_obca_tenant_import; a clocked
        fleet plan at a step boundary, without a trace).  Nothing is zeroed: a slot holds what the
        tenant had, a retired tenant stays retired."""
        from . import _lib
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        blob = np.frombuffer(tenants, np.uint8) if isinstance(tenants, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(tenants, np.uint8)
        self._check(self._lib.piadmm_obca_tenant_import(self.batch._h, len(slots), _lib.iptr(slots), blob.ctypes.data,
                                                      blob.nbytes))
        # the host's copies of what the slots now hold
        t = tenant_unpack(blob)
        self._clock[slots, :2] = t["CLOCK"][:, :2]
        self._clock[slots, 2] = t["CLOCK"][:, 0] + N_HORZ <= t["CLOCK"][:, 1]
        self.ref_traj_s = np.array(self.ref_traj_s)
        self.ref_traj_s[slots] = t["REF"]
        self.ref_traj = None
        self.par[slots] = t["PAR"]
        for j, name in enumerate(FLEET_ROW):
            col = getattr(self, name + "_s").astype(np.float64)
            col[slots] = t["PAR"][:, j]
            setattr(self, name + "_s", col)
        self.primal_thres[slots] = t["PRIMAL_THRES"]
        self.dual_thres[slots] = t["DUAL_THRES"]
        if self.dual_par is not None and len(self.dual_par) == self.n:
            self.dual_par[slots] = t["DUAL_PAR"]
        for k, s in enumerate(slots):
            self.prob[s] = int(t["PROB"][k])
            self.init_state[s] = unpack_state(t["STATE"][k])[1]
            if self.specs is not None:
                self.specs[s] = None              # the tenant's reference is its own, not a spec's

    @classmethod
    def from_tenants(cls, batch, tenants, t_step=0, dual_par=None, on_stage=None):
        """A new clocked fleet plan on `batch` that holds exactly the tenants of a blob, in its order:
        opened through piadmm_obca_fleet_begin on the tenants' own rows and references, the clock
        attached, then the law and the order when the blob carries them, then the import.  dual_par:
        the one gains row the plan shares (None: a row per tenant, the blob's).  The plan counts its
        steps from t_step; the library opens it at min(t_step, n_ref - 8), which a clocked plan
        only shows in T_STEP."""
        t = tenant_unpack(tenants)
        m, par = t["m"], t["PAR"]
        kw = {name: par[:, j] for j, name in enumerate(FLEET_ROW)}
        pl = cls(batch, m, prob=[int(p) for p in t["PROB"]], t_step0=min(int(t_step), t["n_ref"] - N_HORZ),
                 primal_thres=t["PRIMAL_THRES"], dual_thres=t["DUAL_THRES"], update_lamb_ij=t["update_lamb_ij"],
                 ref_traj=t["REF"], state=t["STATE"], clock=True, on_stage=on_stage, **kw)
        if t["law"]:
            pl._set_dual_rows(t["DUAL_PAR"] if dual_par is None else np.asarray(dual_par, np.float64).reshape(1, DUAL_PAR))
        if t["order"]:
            pl.set_order()
        pl.import_tenants(np.arange(m), tenants)
        pl.t_step = int(t_step)
        pl.record.state_record[0] = np.stack(pl.init_state)
        return pl

    def _shared_gains(self):
        """The one gains row a plan of more than one scenario shares, else None."""
        shared = self.dual_par is not None and len(self.dual_par) == 1 and self.n > 1
        return self.dual_par[0].copy() if shared else None

    def compact(self):
        """A new planner on the same batch that holds only the alive tenants, in ascending order of
        their slots (`compact_slots` on the result: where each was).  The batch holds one plan, so
        this planner ends as the new one opens; the tenants continue bit for bit."""
        alive = np.flatnonzero(self.alive())
        if not len(alive):
            raise ValueError("compact: no tenant alive")
        blob = self.export_tenants(alive)
        pl = type(self).from_tenants(self.batch, blob, t_step=int(self.get("T_STEP")[0]), dual_par=self._shared_gains(),
                                     on_stage=self.on_stage)
        pl.compact_slots = alive
        return pl

    def _trace_attached(self):
        try:
            self.trace_rows()
            return True
        except Exception:
            return False

    def save(self, path):
        """Checkpoint of the whole plan at a step boundary (piadmm.io.save_plan_checkpoint, one
        .npz): the blob of all n tenants, the plan cfg, T_STEP, which attachments were on and the
        shared gains row if any.  A trace is not saved (the file says one was attached; it stays
        readable here)."""
        from . import io
        cfg = {f: getattr(self.cfg, f) for f, _ in self.cfg._fields_}
        return io.save_plan_checkpoint(path, self.export_tenants(np.arange(self.n)), int(self.get("T_STEP")[0]), cfg,
                                       dict(fleet=self.fleet, clock=self._clock is not None,
                                            law=self.dual_par is not None, order=bool(self.order),
                                            trace=self._trace_attached()), self._shared_gains())

    @classmethod
    def load(cls, batch, path, on_stage=None):
        """The plan `save` wrote, reopened on `batch` (`from_tenants` at the saved T_STEP) so that its
        next steps are the uninterrupted run's, bit for bit.  It is a fleet plan whatever the saved
        one was; a plan saved without a clock gets its clock detached again."""
        from . import io
        ck = io.load_plan_checkpoint(path)
        pl = cls.from_tenants(batch, ck["tenants"], t_step=ck["t_step"], dual_par=ck["dual_par"], on_stage=on_stage)
        if not ck["attached"]["clock"] and pl.alive().all():
            pl.clear_clock()
        return pl

    def _set_dual_rows(self, rows):
        from . import _lib
        rows = np.ascontiguousarray(rows, np.float64).reshape(-1, DUAL_PAR)
        self._check(self._lib.piadmm_obca_dual_plan(self.batch._h, _lib.dptr(rows), rows.shape[0]))
        self.dual_par = rows

    def set_order(self, work_init=None):
        """Attach the longest-first order (piadmm_obca_order_plan; a step boundary only), its record
        zero or seeded with work_init (n x 2: Q, I per scenario)."""
        from . import _lib
        if work_init is not None:
            work_init = np.ascontiguousarray(work_init, np.int32)
            assert work_init.shape == (self.n, 2), work_init.shape
        self._check(self._lib.piadmm_obca_order_plan(self.batch._h, 1, _lib.iptr(work_init)))
        self.order = True

    def clear_order(self):
        """Detach the order: every list is ascending again (a step boundary only)."""
        self._check(self._lib.piadmm_obca_order_plan(self.batch._h, 0, None))
        self.order = False

    def work(self):
        """The order's record (Q, I) per scenario, n x 2 (PLAN_GET WORK)."""
        return self.get("WORK")

    def _check(self, rc):
        from . import _lib
        if rc != 0:
            msg = self._lib.piadmm_obca_last_error(self.batch._h)
            err = _lib.PiadmmError(f"libpiadmm error {rc}: {msg.decode() if msg else ''}")
            err.code = rc
            raise err

    def set_dual(self, **dual):
        """Attach the PI anti-windup dual law (piadmm_obca_dual_plan; a step boundary only): kP, kI,
        windup_sat, d_gain, windup, each one value or one per scenario.  `dual_par` keeps the rows."""
        from . import _lib
        rows = dual_rows(self.n, dual)
        self._check(self._lib.piadmm_obca_dual_plan(self.batch._h, _lib.dptr(rows), rows.shape[0]))
        self.dual_par = rows

    def clear_dual(self):
        """Detach the law: the plan runs the plain lambda_update again (a step boundary only)."""
        self._check(self._lib.piadmm_obca_dual_plan(self.batch._h, None, 0))
        self.dual_par = None

    def counts(self):
        """(scenarios submitted to the last iterate, scenarios still active, iterates run in the open step)."""
        c = np.zeros(3, np.int32)
        self._check(self._lib.piadmm_obca_plan_get(self.batch._h, PLAN_GET["COUNTS"][0], c.ctypes.data, c.nbytes))
        return int(c[0]), int(c[1]), int(c[2])

    def get(self, what):
        """One item of the resident plan (include/piadmm.h, piadmm_obca_plan_get), shaped: a name of
        PLAN_GET, of NOISE_GET or of DELAY_GET."""
        if what in DELAY_GET:
            code, dt = DELAY_GET[what]
            shape = {"DELAY_PAR": (1 if self._delay is None else len(self._delay[0]), DELAY_PAR),
                     "DELAY_TAU": (self.n, 2), "DELAY_STREAMS": (self.n,), "DELAY_SEED": (3,)}[what]
            out = np.zeros(shape, dt)
            self._check(self._lib.piadmm_obca_plan_get(self.batch._h, code, out.ctypes.data, out.nbytes))
            return out
        if what in NOISE_GET:
            code, dt = NOISE_GET[what]
            shape = {"NOISE_PAR": (1 if self._noise is None else len(self._noise[0]), NOISE_PAR),
                     "NOISE_STREAMS": (self.n,), "NOISE_SEED": (2,)}[what]
            out = np.zeros(shape, dt)
            self._check(self._lib.piadmm_obca_plan_get(self.batch._h, code, out.ctypes.data, out.nbytes))
            return out
        code, dt = PLAN_GET[what]
        n, m = self.n, (self.counts()[0] if what != "COUNTS" else 0)
        rows = n if self.fleet else 1
        shape = {"STATE": (n, PLAN_STATE), "STATE_PREV": (n, PLAN_STATE), "CTRL": (n, 2, NT * NU),
                 "CTRL_PREV": (n, 2, NT * NU), "X": (n, 2, N_HORZ, NX), "ITERS": (n,), "ACTIVE": (m,),
                 "PRIMAL": (n,), "DUAL": (n,), "STOP": (n,), "CONVERGE": (n,), "LOCAL_REC": (2 * m, REC),
                 "LOCAL_OUT": (2 * m, OUT), "LOCAL_IST": (2 * m, 3), "EDGE_REC": (m, EDGE_REC),
                 "EDGE_OUT": (m, EDGE_OUT), "EDGE_IST": (m, NT, 3), "T_STEP": (1,), "LAMBDA": (n, 2, NT, 9),
                 "COUNTS": (3,), "STATUS_MASK": (n, 2), "REF": (rows, 2, self.n_ref, NX),
                 "PAR": (rows, FLEET_PAR), "DUAL_S": (n, 2, NT, 9), "DUAL_D": (n, 2, NT, 9),
                 "DUAL_PAR": (1 if self.dual_par is None else len(self.dual_par), DUAL_PAR), "WORK": (n, 2),
                 "CLOCK": (n, 3), "WINDOW": (n, 2, N_HORZ, NX), "PRIMAL_THRES": (n,), "DUAL_THRES": (n,),
                 "PROB": (n,), "DUAL_S_PREV": (n, 2, NT, 9), "DUAL_D_PREV": (n, 2, NT, 9),
                 "FEEDBACK_PAR": (1 if self._feedback is None else len(self._feedback[0]), FEEDBACK_PAR),
                 "FEEDBACK_STEPS": (1,)}[what]
        out = np.zeros(shape, dt)
        self._check(self._lib.piadmm_obca_plan_get(self.batch._h, code, out.ctypes.data, out.nbytes))
        return out

    def iterate(self):
        """One ADMM iterate of the open MPC step; the number of scenarios still active."""
        left = ctypes.c_int32()
        self._check(self._lib.piadmm_obca_plan_iterate(self.batch._h, ctypes.byref(left)))
        return left.value

    def _tick(self, steps=1):
        """The host's copy of the clocks after `steps` closed steps (the record is deterministic)."""
        for _ in range(steps if self._clock is not None else 0):
            self._clock = clock_tick(self._clock, self._clock[:, 2])

    def shift(self):
        self._check(self._lib.piadmm_obca_plan_shift(self.batch._h))
        self._tick()

    def close(self):
        """End the plan (the batch stays usable after its next upload)."""
        if self.batch._h:
            self._lib.piadmm_obca_plan_end(self.batch._h)

    def _close_step(self, iters, status):
        if self._clock is None and self._feedback is None:
            X = self.get("X")
            self.init_state = [X[s, :, 1].copy() for s in range(self.n)]
        else:
            # a retired scenario's init_state is frozen, an admitted one's X is zero until it runs;
            # with feedback init_state is the state the vehicle reached, not X[1]
            st = self.get("STATE")
            self.init_state = [unpack_state(st[s])[1] for s in range(self.n)]
        self.record.state_record.append(np.stack(self.init_state))
        self.record.iter_num_record.append(np.asarray(iters, int))
        self.record.lambda_record.append(self.get("LAMBDA"))
        self.record.status_record.extend(status)
        self.t_step += 1

    def step(self):
        """One MPC step of every scenario."""
        from . import _lib
        if self.on_stage is not None:
            return self._step_staged()
        iters = np.zeros(self.n, np.int32)
        self._check(self._lib.piadmm_obca_plan_step(self.batch._h, _lib.iptr(iters)))
        self._tick()
        mask = self.get("STATUS_MASK")
        self._close_step(iters, [dict(t_step=self.t_step, iters=iters.copy(), local_status_mask=mask[:, 0].copy(),
                                      edge_status_mask=mask[:, 1].copy())])

    def _step_staged(self):
        n = self.n
        status = []
        left, i_iter = int(self.alive().sum()), 0
        while left:
            i_iter += 1
            before = self.get("STATE")
            ctrl_prev = self.get("CTRL_PREV")
            left = self.iterate()
            active = [int(s) for s in self.get("ACTIVE")]
            after = self.get("STATE")
            recs = self.get("LOCAL_REC")
            res = OBCAResult(self.get("LOCAL_OUT"), self.get("LOCAL_IST"))
            self.on_stage("local", dict(recs=recs, scenarios=list(active), i_iter=i_iter, t_step=self.t_step),
                          dict(result=res))
            fullx = [[res.bar_fullx(2 * k + v) for v in (0, 1)] for k in range(len(active))]
            bar_in = [unpack_state(before[s])[0] for s in active]
            # the exchange leaves Z_bar and lamb_bar as they were; the edge answer replaces them later
            bar_ex = []
            for k, s in enumerate(active):
                b = unpack_state(after[s])[0]
                b["Z_bar"], b["lamb_bar"] = bar_in[k]["Z_bar"].copy(), bar_in[k]["lamb_bar"].copy()
                bar_ex.append(b)
            self.on_stage("exchange", dict(bar=bar_in, fullx=fullx, scenarios=list(active)), dict(bar=bar_ex))
            conv = [bool(c) for c in self.get("CONVERGE")[active]]
            self.on_stage("converge", dict(bar=bar_ex), dict(if_converge=conv))
            erecs = self.get("EDGE_REC")
            eres = OBCAEdgeResult(self.get("EDGE_OUT"), self.get("EDGE_IST"))
            self.on_stage("edge", dict(recs=erecs, scenarios=list(active)), dict(result=eres))
            status.append(dict(t_step=self.t_step, i_iter=i_iter, scenarios=list(active), local_status=res.status.copy(),
                               edge_status=eres.status.copy(), if_converge=conv))
            ctrl = self.get("CTRL")
            self.on_stage("residual",
                          dict(ctrl=[ctrl[s] for s in active], ctrl_prev=[ctrl_prev[s] for s in active],
                               lamb_bar=[unpack_state(after[s])[0]["lamb_bar"] for s in active],
                               lamb_bar_prev=[b["lamb_bar"] for b in bar_in], i_iter=i_iter, scenarios=list(active)),
                          dict(primal=self.get("PRIMAL")[active], dual=self.get("DUAL")[active],
                               stop=self.get("STOP")[active].astype(bool)))
        iters = self.get("ITERS")
        frozen = self.get("STATE_PREV")
        X = self.get("X")
        self.shift()
        nxt = self.get("STATE")
        self.on_stage("shift", dict(bar_prev=[unpack_state(frozen[s])[0] for s in range(n)],
                                    X=[[X[s, 0], X[s, 1]] for s in range(n)], iters=iters.astype(int)),
                      dict(bar_next=[unpack_state(nxt[s])[0] for s in range(n)],
                           init_state=[unpack_state(nxt[s])[1] for s in range(n)]))
        self._close_step(iters, status)

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            if not self.alive().any():
                break
            self.step()
        return self.record

    def steps_left(self):
        """The steps the longest-lived scenario has left (None without a clock: the plan's reference
        decides)."""
        if self._clock is None:
            return None
        c = self._clock[self._clock[:, 2] != 0]
        return int((c[:, 1] - N_HORZ - c[:, 0] + 1).max()) if len(c) else 0

    def trace_begin(self, cap_steps, keep_lambda=True):
        """Attach a device-side run record of capacity cap_steps to the plan (a step boundary only)."""
        self._check(self._lib.piadmm_obca_trace_begin(self.batch._h, int(cap_steps),
                                                      TRACE_LAMBDA if keep_lambda else 0))
        self._trace_lambda = bool(keep_lambda)

    def trace_run(self, n_steps):
        """n_steps MPC steps on the device, recorded; the number completed."""
        done = ctypes.c_int32()
        rc = self._lib.piadmm_obca_trace_run(self.batch._h, int(n_steps), ctypes.byref(done))
        self._tick(done.value)
        self._check(rc)
        return done.value

    def trace_rows(self):
        r = np.zeros(1, np.int32)
        self._check(self._lib.piadmm_obca_trace_get(self.batch._h, TRACE_GET["ROWS"][0], r.ctypes.data, r.nbytes))
        return int(r[0])

    def trace_get(self, what):
        """One item of the attached trace (include/piadmm.h, piadmm_obca_trace_get), shaped."""
        code, dt = TRACE_GET[what]
        n, R = self.n, (self.trace_rows() if what not in ("ROWS", "SUMMARY") else 0)
        shape = {"STATES": (R + 1, n, 2, NX), "CLEARANCE": (R + 1, n, 2), "ITERS": (R, n), "STATUS_MASK": (R, n, 2),
                 "PRIMAL": (R, n), "DUAL": (R, n), "LAMBDA": (R, n, 2, NT, 9), "SUMMARY": (n, 4), "ROWS": (1,)}[what]
        out = np.zeros(shape, dt)
        self._check(self._lib.piadmm_obca_trace_get(self.batch._h, code, out.ctypes.data, out.nbytes))
        return out

    def trace_end(self):
        self._check(self._lib.piadmm_obca_trace_end(self.batch._h))

    def trace_stats(self, edges, worst=1) -> OBCAFleetStats:
        """The fleet statistics of the attached trace, reduced on the device in place
        (piadmm_obca_stats_trace): only the results come back.  `fleet_stats_host` on the arrays
        `trace_get` returns is the same statement."""
        def call(*a):
            return self._lib.piadmm_obca_stats_trace(self.batch._h, *a)
        # without a trace the call itself says so: R only sizes the result arrays
        r = np.zeros(1, np.int32)
        got = self._lib.piadmm_obca_trace_get(self.batch._h, TRACE_GET["ROWS"][0], r.ctypes.data, r.nbytes)
        rc, out = _stats_call(call, self.n, int(r[0]) if got == 0 else 0, edges, worst)
        self._check(rc)
        return out

    def trace_gather_bytes(self, m):
        size = ctypes.c_int64()
        self._check(self._lib.piadmm_obca_gather_trace_bytes(self.batch._h, int(m), ctypes.byref(size)))
        return int(size.value)

    def trace_gather(self, slots, nbytes=None):
        """Every row of the scenarios `slots` (distinct, any order) of the attached trace, gathered on
        the device (piadmm_obca_gather_trace): name -> array with column k = scenario slots[k], as
        `trace_gather_unpack` shapes them.  nbytes: the blob's size, when the caller knows better."""
        from . import _lib
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        m = len(slots)
        size = self.trace_gather_bytes(m) if nbytes is None else int(nbytes)
        blob = np.zeros(max(size, 1), np.uint8)
        self._check(self._lib.piadmm_obca_gather_trace(self.batch._h, m, _lib.iptr(slots), blob.ctypes.data, size))
        return trace_gather_unpack(blob[:size], self.trace_rows(), m, getattr(self, "_trace_lambda", None))

    def trace_worst(self, edges, K):
        """(statistics, the gathered record of the K worst scenarios by plain minimum clearance)."""
        st = self.trace_stats(edges, worst=K)
        return st, self.trace_gather(st.worst)

    def trace(self, keep_lambda=True):
        """The attached trace as an OBCATrace."""
        summary = self.trace_get("SUMMARY")
        return OBCATrace(states=self.trace_get("STATES"), clearance=self.trace_get("CLEARANCE"),
                         iters=self.trace_get("ITERS"), status_mask=self.trace_get("STATUS_MASK"),
                         primal=self.trace_get("PRIMAL"), dual=self.trace_get("DUAL"),
                         min_clearance=summary[:, 0].copy(), min_row=summary[:, 1].astype(np.int64),
                         min_clearance_tight=summary[:, 2].copy(), iters_sum=summary[:, 3].astype(np.int64),
                         lamb=self.trace_get("LAMBDA") if keep_lambda else None)

    def run_traced(self, n_steps, keep_lambda=True):
        """`run` with the record kept on the device: one piadmm_obca_trace_begin, one
        piadmm_obca_trace_run of n_steps MPC steps and the downloads at the end, instead of the
        per-step downloads of `step`.  Fills `record` as `run` does (status_record with the per-step
        entry of the un-staged `step`; lambda_record only with keep_lambda), advances t_step and
        init_state, and returns the OBCATrace with the clearances.  Staged stepping stays on `run`."""
        if self.on_stage is not None:
            raise ValueError("run_traced does not stage: use run() with on_stage")
        n_steps = int(n_steps)
        if self._clock is not None:
            n_steps = min(n_steps, self.steps_left())      # with nothing alive: an empty trace
        self.trace_begin(max(n_steps, 1), keep_lambda)
        if n_steps:
            self.trace_run(n_steps)
        tr = self.trace(keep_lambda)
        self.trace_end()
        for k in range(tr.iters.shape[0]):
            iters = tr.iters[k].copy()
            self.init_state = [tr.states[k + 1, s].copy() for s in range(self.n)]
            self.record.state_record.append(np.stack(self.init_state))
            self.record.iter_num_record.append(np.asarray(iters, int))
            if keep_lambda:
                self.record.lambda_record.append(tr.lamb[k].copy())
            self.record.status_record.append(dict(t_step=self.t_step, iters=iters.copy(),
                                                  local_status_mask=tr.status_mask[k, :, 0].copy(),
                                                  edge_status_mask=tr.status_mask[k, :, 1].copy()))
            self.t_step += 1
        return tr
