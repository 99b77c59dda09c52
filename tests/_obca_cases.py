"""Case sets of the OBCA local subproblem shared by tests/test_obca_cases.py (CPU: the NumPy oracle
against the C++ port, and the coverage each set must have) and tests/test_gpu_obca.py (GPU: the
kernel against the oracle on the same sets).  A plain module: nothing here runs on import but
the 72 `overtaking_problem` records of BASE; oracle answers are computed on demand and cached.
"""
import functools

import numpy as np

from oracle import obca_oracle as O
from piadmm import obca

T_STEPS = (2, 8, 14, 20, 29, 35)
VARIANTS = ("initial", "consensus", "perturbed")

# (prob, t_step, vehicle, variant) of BASE[k]
KEYS = [(prob, ts, veh, var) for prob in (1, 0) for ts in T_STEPS for veh in (0, 1) for var in VARIANTS]
BASE = [obca.overtaking_problem(ts, veh, var, prob=prob) for prob, ts, veh, var in KEYS]


def modify(rec, **kw):
    """`rec` with the fields `kw` (names of obca.unpack) overridden."""
    d = obca.unpack(rec)
    unknown = set(kw) - set(d)
    assert not unknown, unknown
    d.update(kw)
    return obca.pack(d.pop("init"), d.pop("ref"), d.pop("A_o"), d.pop("b_o"), d.pop("lamb_ij_o"),
                     d.pop("lamb_bar"), d.pop("Z_bar"), **d)


def _all(**kw):
    return np.ascontiguousarray(np.stack([modify(rec, **kw) for rec in BASE]))


def base():
    return np.ascontiguousarray(np.stack(BASE))


def truncated(k):
    """BASE stopped after k SQP iterations: the iterate and the multipliers after k steps (line
    search, merit parameter, multiplier blend), not the fixed point."""
    assert 1 <= k <= 4
    return _all(max_iter=k)


def off_default():
    """name -> records: BASE at parameters no preset uses.

    rho_small / rho_large   the consensus weight, two decades either side of 1
    min_dis_0.5             a wider (5a) margin, still feasible everywhere
    r_q_1                   r = q = 1: the tracking weights no longer dwarf the consensus terms, the
                            controls leave zero and the control-bound rows (y_u) become active
                            (21 problems).  With max_iter = 12: 54 problems converge within it and
                            18 are compared at their 12th iterate; at the scenario's 60, 8 problems
                            run all 60 iterations and the set costs the oracle 10 s instead of 4
    state_box               max_x = the record's last reference x - 0.05 m: the upper x row of the
                            state box binds at the end of the horizon (y_x[:, 0] < 0) on 34 of 72
                            problems, all converged.  One max_x for all of BASE binds on six
                            problems only (83.0: vehicle 0 at t_step 35), and no max_y binds on a
                            converged problem without leaving 30 others infeasible: vehicle 0's y
                            falls from its executed 4.0 towards the reference's 0 along the whole
                            horizon, so its largest y is X_1's, which the bicycle cannot move.
    infeasible              min_dis = 1.0, max_y = 3.0, max_x = 60: 39 problems qp_infeasible at the
                            first QP, 33 converged
    """
    box = np.stack([modify(rec, max_x=float(obca.unpack(rec)["ref"][7, 0] - 0.05)) for rec in BASE])
    return {
        "rho_small": _all(rho=0.01),
        "rho_large": _all(rho=100.0),
        "min_dis_0.5": _all(min_dis=0.5),
        "r_q_1": _all(r=1.0, q=1.0, max_iter=12),
        "state_box": np.ascontiguousarray(box),
        "infeasible": _all(min_dis=1.0, max_y=3.0, max_x=60.0),
    }


OFF_DEFAULT_NAMES = ("rho_small", "rho_large", "min_dis_0.5", "r_q_1", "state_box", "infeasible")
EXCHANGED_T = (8, 14, 20)


@functools.lru_cache(maxsize=None)
def _solve(raw):
    p, opt = O.from_record(np.frombuffer(raw, np.float64))
    return p, O.solve_local(p, opt)


def oracle(recs):
    """[(LocalProblem, Result)] of oracle/obca_oracle.py for each record; each distinct record is
    solved once per process."""
    return [_solve(np.ascontiguousarray(rec, np.float64).tobytes()) for rec in recs]


PRIMAL = ("X", "U", "Lam")
MULTIPLIERS = ("y_a", "y_b", "y_n", "y_x", "pi", "y_u", "y_l")
WRITES_ITERATE = (O.CONVERGED, O.MAX_ITER, O.LINESEARCH_FAIL)
ATOL, RTOL = 1e-7, 1e-9        # X, U, Lambda (the bars of tests/test_gpu_obca.py); the cost: RTOL
MULT_TOL = 1e-7                # a multiplier block, relative to max(1, max |reference block|)


def compare(res, orc, exempt=()):
    """An OBCAResult against the oracle's answers `orc` (from `oracle`): status and SQP iteration
    count equal exactly (problems listed in `exempt` may differ in both and are then not compared
    further); for every status that writes an iterate, X, U, Lambda within ATOL + RTOL |ref|, the
    cost within RTOL max(1, |ref|) and each multiplier block within MULT_TOL max(1, max |ref|).
    Returns the worst deviation per block relative to max(1, max |reference block|)."""
    worst = dict.fromkeys(PRIMAL + ("cost",) + MULTIPLIERS, 0.0)
    for k, (_, r) in enumerate(orc):
        same = res.status[k] == r.status and int(res.iters[k]) == r.iters
        if not same and k in exempt:
            continue
        assert same, (k, int(res.status[k]), r.status, int(res.iters[k]), r.iters)
        if r.status not in WRITES_ITERATE:
            continue
        for name in PRIMAL:
            got, ref = getattr(res, name)[k], getattr(r, name)
            worst[name] = max(worst[name], float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max())))
            np.testing.assert_allclose(got, ref, rtol=RTOL, atol=ATOL, err_msg=f"{name} {k}")
        dev = abs(res.cost[k] - r.cost) / max(1.0, abs(r.cost))
        worst["cost"] = max(worst["cost"], float(dev))
        assert dev <= RTOL, (k, res.cost[k], r.cost)
        for name in MULTIPLIERS:
            got, ref = np.asarray(getattr(res, name)[k]), np.asarray(getattr(r, name))
            dev = float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))
            worst[name] = max(worst[name], dev)
            assert dev <= MULT_TOL, (name, k, dev)
    return worst


def report(title, worst):
    print(f"{title}: worst deviation rel. max(1, max|ref|): "
          + "  ".join(f"{name} {dev:.1e}" for name, dev in worst.items()))


@functools.lru_cache(maxsize=None)
def _exchanged():
    recs = []
    for prob in (1, 0):
        for ts in EXCHANGED_T:
            for var in VARIANTS:
                idx = [KEYS.index((prob, ts, veh, var)) for veh in (0, 1)]
                sol = [r for _, r in oracle([BASE[i] for i in idx])]
                if any(r.status != O.CONVERGED for r in sol):
                    continue
                fullx = [np.concatenate([r.X[1:], r.Lam], axis=1) for r in sol]
                bar = obca.bar_state_update(obca.create_bar_state(), fullx, prob=prob)
                for veh in (0, 1):
                    o = 1 - veh
                    lij = np.zeros((obca.NT, 4))
                    for t in range(obca.NT):
                        dvec = fullx[veh][t, :2] - fullx[o][t, :2]
                        lij[t] = obca.separating_duals(bar["A"][o, t], dvec / np.linalg.norm(dvec), 0.9)
                    recs.append(modify(BASE[idx[veh]], A_o=bar["A"][o], b_o=bar["b"][o], lamb_ij_o=lij))
    return np.ascontiguousarray(np.stack(recs))


def exchanged():
    """What the planner's second ADMM iterate sees: the records of BASE at t_step 8, 14, 20 (both
    vehicles, variants and halfspace models: 36 records) with the other vehicle's A_o, b_o the
    halfspaces of its SOLVED plan (obca.bar_state_update on the oracle's converged bar_fullx of
    both vehicles) in place of those of `executed_path`, and lamb_ij_o from
    obca.separating_duals along the solved centre-to-centre direction."""
    return _exchanged().copy()
