"""GPU parity off the presets: the cases of tests/_offpreset_cases.py (proved sound on the CPU by
tests/test_offpreset_cases.py) on the fused kernel (csrc/piadmm_device.hip) and on the graph kernel
(csrc/piadmm_graph.hip; PIADMM_GRAPH=1 sends a job of disjoint pairs there), against the oracle:

(a) host-stepped (piadmm_outer_iter / piadmm_get_state / piadmm_step_finish): pos_old, hat, lam, S
    and D after every outer iteration at 1e-8 (D scaled by max(1, |S|)), the stop flag at the same
    iteration, xt and u after the propagation, and the pair penalties rho_pi of the global PI law;
(b) piadmm_mpc_step on a fresh handle (one launch: the speculative and compact loops, which host
    stepping does not take): every QP status 0, equal iteration counts, u and xt at 1e-8, the
    residual histories at 1e-7, no inexact QP.

The cases set dt, L, beta, Pnorm, Pcost, rho, u_max, du_max, dis_thres, round_decimals 2 / 6,
eps_pri / eps_dual, kI, theta1, theta2, windup_sat, windup, tight_p, avg_delay, var_delay and the
global PI law's rho_num, rho_min, rho_max, d_gain, dual_init, ki_adapt, pi_trad off their presets'
values; the saturating cases run the back-calculation D = lam_sat - lam_raw on both kernels."""
import numpy as np
import pytest

import _offpreset_cases as C

pytestmark = pytest.mark.gpu

WORST = {}      # (group, path) -> (worst deviation, its tolerance)


@pytest.fixture(scope="module")
def Solver():
    from piadmm.solver import PI_ADMM_MI355X, device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    return PI_ADMM_MI355X


@pytest.fixture(scope="module", autouse=True)
def report():
    """The figures DESIGN.md section 3 quotes: the worst deviation of each group on each path,
    printed once the module's tests have run (every single comparison is asserted in its test)."""
    yield
    for (group, path), (w, tol) in sorted(WORST.items()):
        print(f"off-preset group {group}, {path}: worst deviation {w * tol:.2e} (bar {tol:g})")


def on_kernel(case, kernel, monkeypatch):
    assert kernel in case.kernels
    if kernel == "graph":
        monkeypatch.setenv("PIADMM_GRAPH", "1")
    else:
        monkeypatch.delenv("PIADMM_GRAPH", raising=False)


def note(case, path, worst, tol=C.TOL):
    """``worst`` in units of ``tol`` (C.excess)."""
    key = (case.group, path)
    WORST[key] = max(WORST.get(key, (0.0, tol)), (worst, tol))
    print(f"{case.name} [{path}]: worst deviation {worst * tol:.2e} (bar {tol:g})")


@pytest.mark.parametrize("case,kernel", C.GPU_PARAMS, ids=C.GPU_IDS)
def test_host_stepped_iterations_match_oracle(Solver, case, kernel, monkeypatch):
    on_kernel(case, kernel, monkeypatch)
    cfg, run = case.cfg, C.oracle_run(case.name)
    worst = 0.0
    with Solver(cfg, case.scenario()) as s:
        for t in range(case.steps):
            worst = max(worst, C.check_iterations(s, t, run.states[t], run.recs[t]))
        if case.group == "G":
            rho = s.step_state()["rho_pi"]
            np.testing.assert_allclose(rho, run.rho_pi[-1], rtol=C.TOL, atol=C.TOL)
            worst = max(worst, C.excess(rho, run.rho_pi[-1]))
        assert s.counters()["inexact"] == 0
    note(case, "host-stepped", worst)


@pytest.mark.parametrize("case,kernel", C.GPU_PARAMS, ids=C.GPU_IDS)
def test_one_launch_step_matches_oracle(Solver, case, kernel, monkeypatch):
    on_kernel(case, kernel, monkeypatch)
    cfg, run = case.cfg, C.oracle_run(case.name)
    worst = worst_r = 0.0
    with Solver(cfg, case.scenario()) as s:
        assert s.C == len(run.recs[0].iters)
        for t, ro in enumerate(run.recs):
            rg = s.mpc_step()
            np.testing.assert_array_equal(rg.status, 0, err_msg=f"step {t}")
            np.testing.assert_array_equal(rg.iters, ro.iters, err_msg=f"step {t}")
            np.testing.assert_allclose(rg.xt, ro.xt, rtol=C.TOL, atol=C.TOL, err_msg=f"xt, step {t}")
            np.testing.assert_allclose(rg.u, ro.u, rtol=C.TOL, atol=C.TOL, err_msg=f"u, step {t}")
            worst = max(worst, C.excess(rg.xt, ro.xt), C.excess(rg.u, ro.u))
            for c, hist in enumerate(ro.resid):
                n = len(hist)
                if n:
                    res = np.array(hist, np.float64)
                    np.testing.assert_allclose(rg.resid[c, :n], res, rtol=1e-7, atol=1e-7, err_msg=f"resid, step {t}")
                    worst_r = max(worst_r, C.excess(rg.resid[c, :n], res, rtol=1e-7, atol=1e-7))
                assert np.all(np.isnan(rg.resid[c, n:]))
        assert s.counters()["inexact"] == 0
    note(case, "one launch", worst)
    note(case, "one launch, residuals", worst_r, 1e-7)
