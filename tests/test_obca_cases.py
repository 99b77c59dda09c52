"""The OBCA case sets of tests/_obca_cases.py are sound before a GPU sees them: the two independent
CPU implementations of the batched SQP (oracle/obca_oracle.py in NumPy, oracle/obca_cpu.cpp in
C++) agree on every set -- status and SQP iteration count exactly, X / U / Lambda / cost and all
seven multiplier blocks within the bars of tests/test_gpu_obca.py -- and the oracle's answers
have the coverage the GPU tests rely on (truncated runs that stop mid-way, active control-bound
and state-box rows, infeasible QPs next to converged ones, every multiplier block nonzero).

The norm row y_n ((L0-L2)^2 + (L1-L3)^2 <= 1, optimizer.py:126-129) has no set: no input of this
scenario family makes it bind.  (5b) is an equality, A(X_t)' Lambda_t = -w_t with w_t = A_o'
lamb_ij_o data of the record, and A(theta) has orthonormal rows e, n, so the row's value is
|w_t|^2 at every feasible point whatever X and Lambda are: the row is implied when |w_t| <= 1
and infeasible otherwise.  In the condensed QP, where (5b) is eliminated, its gradient is zero
up to rounding (2 m' M dLam = -2 m' gb_v since m . dm/dtheta = 0), so it is never added to the
active set.  Tried on BASE with the C++ port, y_n stayed identically zero on all 72 problems for:
Z_bar's Lambda targets 5 and 50 (all four, and the first only), the same with rho = 100;
rho = 0.01 and 1e-4; lamb_ij_o scaled so that |w_t| = 0.945, 0.99, 0.999999 and 1.0 (all
converged, y_n = 0); |w_t| = 1.000001 and 1.08 end qp_infeasible at the first QP on all 72.
"""
import numpy as np
import pytest

import _obca_cases as C
from oracle import obca_cpu
from oracle import obca_oracle as O
from piadmm import obca

SETS = ("base",) + tuple(f"truncated_{k}" for k in (1, 2, 3, 4)) + C.OFF_DEFAULT_NAMES + ("exchanged",)


def _records(name):
    if name == "base":
        return C.base()
    if name.startswith("truncated_"):
        return C.truncated(int(name[-1]))
    if name == "exchanged":
        return C.exchanged()
    return C.off_default()[name]


def _answers(name):
    return [r for _, r in C.oracle(_records(name))]


def _count(name, status):
    return sum(r.status == status for r in _answers(name))


@pytest.mark.parametrize("name", SETS)
def test_cpu_port_equals_the_oracle(name):
    recs = _records(name)
    out, ist, _ = obca_cpu.solve(recs, threads=4)
    worst = C.compare(obca.OBCAResult(out, ist), C.oracle(recs))
    C.report(f"obca_cpu vs oracle, {name} ({len(recs)} problems)", worst)


def test_truncated_runs_stop_inside_the_sqp():
    one = _answers("truncated_1")
    assert all(r.status == O.MAX_ITER and r.iters == 1 for r in one)
    for k in (2, 3):
        assert _count(f"truncated_{k}", O.CONVERGED) >= 5 and _count(f"truncated_{k}", O.MAX_ITER) >= 5
    # a truncated run ends where the full run stood after k iterations: never later than it
    for k in (1, 2, 3, 4):
        for full, cut in zip(_answers("base"), _answers(f"truncated_{k}")):
            assert cut.iters == min(full.iters, k)
            assert cut.status == (O.CONVERGED if full.iters <= k else O.MAX_ITER)


def test_control_bound_rows_are_active_at_r_q_1():
    assert sum(np.abs(r.y_u).max() > 1e-6 for r in _answers("r_q_1")) >= 5
    # and nowhere at the defaults: the set is what covers these rows
    assert all(np.abs(r.y_u).max() == 0.0 for r in _answers("base"))


def test_state_box_binds_on_converged_problems():
    recs = _records("state_box")
    n = 0
    for rec, r in zip(recs, _answers("state_box")):
        if r.status != O.CONVERGED:
            continue
        d = obca.unpack(rec)
        n += bool(np.any(np.abs(r.X[1:, 0] - d["max_x"]) <= 1e-9) or np.any(np.abs(np.abs(r.X[1:, 1]) - d["max_y"]) <= 1e-9))
    assert n >= 5, n


def test_infeasible_set_has_both_outcomes():
    assert _count("infeasible", O.QP_INFEASIBLE) >= 5 and _count("infeasible", O.CONVERGED) >= 5


def test_exchanged_set_converges():
    """`exchanged` is kept only while the oracle converges on at least 90 % of it."""
    recs = _records("exchanged")
    assert len(recs) == 36
    assert _count("exchanged", O.CONVERGED) >= 0.9 * len(recs)
    # the halfspaces differ from those of the executed path the records started from
    keys = [(prob, ts, veh, var) for prob in (1, 0) for ts in C.EXCHANGED_T for var in C.VARIANTS for veh in (0, 1)]
    moved = sum(not np.array_equal(obca.unpack(rec)["b_o"], obca.unpack(C.BASE[C.KEYS.index(k)])["b_o"])
                for rec, k in zip(recs, keys))
    assert moved >= 30, moved


def test_every_multiplier_block_but_the_norm_row_is_exercised():
    nonzero = dict.fromkeys(C.MULTIPLIERS, 0)
    for name in SETS:
        for r in _answers(name):
            if r.status in C.WRITES_ITERATE:
                for blk in C.MULTIPLIERS:
                    nonzero[blk] += bool(np.any(np.asarray(getattr(r, blk)) != 0.0))
    print("problems with a nonzero block:", nonzero)
    for blk in ("y_a", "y_b", "y_x", "pi", "y_l", "y_u"):
        assert nonzero[blk] >= 10, nonzero
    assert nonzero["y_n"] == 0     # see the module docstring: the row cannot bind
