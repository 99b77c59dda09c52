"""The gains of the PI anti-windup dual law that the CPU test (tests/test_obca_dual_pi_host.py)
chooses with the host planner and the GPU test (tests/test_gpu_obca_dual_pi.py) runs on the device,
and the coverage counts both assert.

GAINS is for the 3-scenario SETUP plan of tests/test_gpu_obca_plan.py, FLEET_GAINS one row per case
of tests/_obca_fleet_cases.py (kI = the row's rho).  With them, at every iterate of MPC step 12
some entries of the written slots are clipped at windup_sat and some are not, and from the second
iterate on a non-zero back-calculation term D enters the integrator (d_gain != 0)."""
import numpy as np

from piadmm import obca

GAINS = dict(kP=0.5, kI=1.0, windup_sat=0.05, d_gain=0.5, windup=1)
FLEET_GAINS = dict(kP=[0.5, 0.25, 1.0, 0.0], kI=[1.0, 0.5, 2.0, 1.5], windup_sat=[0.05, 0.1, 0.05, 0.2],
                   d_gain=[0.5, 1.0, 0.25, 0.5], windup=[1, 1, 1, 0])


def fleet_gains(cases):
    """FLEET_GAINS of the fleet whose scenario k is case cases[k]."""
    return {name: [vals[c] for c in cases] for name, vals in FLEET_GAINS.items()}


def wrote_of(status):
    """The 7 `wrote` flags of one scenario's edge statuses."""
    return [int(c) in obca.EDGE_WRITES_ITERATE for c in status]


def coverage(lamb_new, D_in, wrote, row):
    """(clipped, unclipped, fed back) over the entries of the written slots of one scenario's
    iterate: |lam'| at windup_sat, |lam'| below it, and a non-zero D entering S (d_gain != 0).
    Without windup nothing counts as clipped."""
    m = np.broadcast_to(np.asarray(wrote, bool)[None, :, None], (2, obca.NT, 9))
    sat, d_gain, windup = row[2], row[3], row[4] != 0.0
    a = np.abs(np.asarray(lamb_new))
    clipped = int((m & (a == sat)).sum()) if windup else 0
    fed = int((m & (np.asarray(D_in) != 0.0)).sum()) if d_gain != 0.0 else 0
    return clipped, int(m.sum()) - clipped, fed


def bar_of_edge(erec, z_bar):
    """The bar_state `lambda_update_pi` reads, from one edge record and the edge output's Z_bar."""
    u = obca.edge_unpack(erec)
    return dict(local_x=u["local_x"], lamb_ij=u["lamb_ij"], lamb_bar=u["lamb_bar"], Z_bar=np.asarray(z_bar))
