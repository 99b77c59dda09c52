"""The overtaking scenario of the OBCA planner: constants, references, vehicle geometry, the bar state,
the per-scenario parameters, and the local (vehicle) and edge (RSU) records."""
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
    entries, theta linearly, no wrap.  The statements of stale_state (csrc/piadmm_obca_plan_draw.h) in
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


def local_z(bar):
    """w = [local_x, lamb_ij] (num_veh x 7 x 9), the local side of the consensus (optimizer.py:303-304, :333)."""
    return np.concatenate([bar["local_x"], bar["lamb_ij"]], axis=2)


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


# a parameter row of piadmm_obca_fleet_begin (include/piadmm.h), by constructor argument; the rest is zero
FLEET_ROW = ("rho", "min_dis", "conv_thres", "max_x", "max_y", "r", "q", "x_bound", "mu_max", "g_max",
             "max_admm_iter", "max_iter", "round_decimals", "start")
_FLEET_INTS = ("max_admm_iter", "max_iter", "round_decimals", "start")


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


def lambda_update(bar, rho):
    """`lambda_update` (optimizer.py:330-335): lamb_bar += rho (w - Z_bar).  Host form of the
    update the edge kernel fuses behind its solve."""
    out = {k: v.copy() for k, v in bar.items()}
    out["lamb_bar"] = bar["lamb_bar"] + rho * (local_z(bar) - bar["Z_bar"])
    return out
