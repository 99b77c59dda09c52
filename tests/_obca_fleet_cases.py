"""The four base cases of the per-scenario OBCA planner, shared by the CPU test
(tests/test_obca_fleet_host.py) and the GPU test (tests/test_gpu_obca_fleet.py): one row per
scenario of every argument that can differ between the scenarios of a fleet.

Row 0 is the default manoeuvre on default parameters, row 3 the default manoeuvre on other
parameters, rows 1 and 2 other manoeuvres.  r, q, max_x and x_bound are off their defaults on one
row each; round_decimals differs on the row that stops at its first iterate.  With the residual
thresholds below, rows 0 and 1 stop at iterate 3 and row 2 at iterate 2, each by its own
max_admm_iter, and row 3 at iterate 1 by its thresholds."""
import numpy as np

from piadmm import obca

SPECS = [obca.OvertakeSpec(20, 10, 20, 4.0), obca.OvertakeSpec(18, 12, 15, 3.5), obca.OvertakeSpec(16, 11, 12, 3.0),
         obca.OvertakeSpec(20, 10, 20, 4.0)]
ROWS = dict(
    prob=[1, 0, 1, 0],
    rho=[1.0, 0.5, 2.0, 1.5],
    min_dis=[0.1, 0.05, 0.3, 0.2],
    max_admm_iter=[2, 2, 1, 2],
    primal_thres=[0.01, 0.01, 0.01, np.inf],
    dual_thres=[0.01, 0.01, 0.01, np.inf],
    r=[1e4, 2e4, 1e4, 1e4],
    q=[1e5, 1e5, 5e4, 1e5],
    max_x=[150.0, 150.0, 150.0, 200.0],
    x_bound=[1000.0, 500.0, 1000.0, 1000.0],
    round_decimals=[-1, -1, -1, 4],
)
STOP_ITERS = [3, 3, 2, 1]
T_STEPS = (5, 12)


def fleet_kwargs(cases, t_step0):
    """Planner arguments of the fleet whose scenario k is case cases[k]."""
    kw = {name: [vals[c] for c in cases] for name, vals in ROWS.items()}
    return dict(kw, n_scenarios=len(cases), specs=[SPECS[c] for c in cases], t_step0=t_step0)


def single_kwargs(case, t_step0):
    """Planner arguments of case `case` alone, every parameter a scalar."""
    kw = {name: vals[case] for name, vals in ROWS.items()}
    kw.update(prob=[kw["prob"]], primal_thres=[kw["primal_thres"]], dual_thres=[kw["dual_thres"]])
    return dict(kw, n_scenarios=1, specs=[SPECS[case]], t_step0=t_step0)
