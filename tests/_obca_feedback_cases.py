"""Cases of the closed-loop feedback tests (tests/test_obca_feedback_host.py,
tests/test_gpu_obca_feedback.py): the vehicle model written out from optimizer.py:75-77, the
boundary states of the plant step, and the one tolerance of the GPU tests."""
import numpy as np

from piadmm import obca

# k_plan_propagate against obca.propagate: device libm is not NumPy's.  The largest absolute deviation
# measured on an MI355X over `kernel_cases` at every size of KERNEL_SIZES, with and without w, is
# 2.220446e-16 (one ulp of a y of 1.44 m after 64 RK4 substeps); the bound is 8 times it, the margin
# for libm differences between ROCm releases.  Every other GPU assertion is bit equality.
PROPAGATE_MEASURED = 2.220446e-16
PROPAGATE_TOL = 8 * PROPAGATE_MEASURED

PW = 4                                  # waves per workgroup of the plan's kernels (csrc/piadmm_obca_plan.hip)
# scenarios: 2n lanes at the wave boundary (31, 32, 33) and at the workgroup boundary (32 PW +- 1)
KERNEL_SIZES = (1, 31, 32, 33, 32 * PW - 1, 32 * PW + 1)


def f(st, con, lr=1.0, lf=1.5):
    """The reference's right-hand side (decentralized/optimizer.py:75-77) for states (..., 5) and
    controls (..., 2): beta = atan(lr tan(delta) / (lr + lf)),
    rhs = (v cos(theta + beta), v sin(theta + beta), a, v / lr sin(beta), steering_rate)."""
    v, theta, delta = st[..., 2], st[..., 3], st[..., 4]
    beta = np.arctan(lr * np.tan(delta) / (lr + lf))
    return np.stack((v * np.cos(theta + beta), v * np.sin(theta + beta), con[..., 0], v / lr * np.sin(beta),
                     con[..., 1]), axis=-1)


# (state, control) pairs at the edges of the model: v = 0, delta = 0, delta = +-0.6, theta near +-pi,
# a and omega beyond the actuator limits of the nominal row (5, 20)
BOUNDARY = (
    ((3.0, 1.0, 0.0, 0.3, 0.2), (1.0, 0.5)),                 # v = 0
    ((10.0, -2.0, 15.0, 0.1, 0.0), (0.5, 0.0)),              # delta = 0
    ((50.0, 4.0, 20.0, 0.05, 0.6), (-1.0, -0.4)),            # delta = +0.6, steering back
    ((50.0, 4.0, 20.0, -0.05, -0.6), (-1.0, 0.4)),           # delta = -0.6, steering back
    ((120.0, 0.5, 12.0, np.pi - 1e-9, 0.1), (0.2, 0.1)),     # theta near +pi
    ((120.0, 0.5, 12.0, -np.pi + 1e-9, -0.1), (0.2, -0.1)),  # theta near -pi
    ((20.0, 0.0, 18.0, 0.0, 0.05), (9.0, 0.3)),              # a saturated
    ((20.0, 0.0, 18.0, 0.0, 0.05), (-9.0, 0.3)),
    ((20.0, 0.0, 18.0, 0.0, 0.05), (0.5, 30.0)),             # omega saturated: delta reaches 0.6 mid-step
    ((20.0, 0.0, 18.0, 0.0, -0.05), (0.5, -30.0)),
)
# the boundary pairs whose nominal step stays inside every limit: there the plant is st + DT f(st, con)
BOUNDARY_INSIDE = BOUNDARY[:6]

# plant rows of the kernel cases: both methods, n_sub 1 and 64, axle distances, gains and limits off nominal
ROWS = (
    dict(),
    dict(method=1),
    dict(n_sub=64),
    dict(method=1, n_sub=64),
    dict(method=(0, 1), n_sub=(64, 3), lr=(1.2, 0.9), lf=(1.4, 1.7), gain_a=(0.8, 1.1), gain_w=(0.0, 1.3),
         a_max=(2.0, 5.0), w_max=(0.5, 20.0)),
)


def path_states(n):
    """n state pairs of the default manoeuvre's executed path, spread over its 5 s."""
    return np.stack([np.stack([obca.executed_path(v, 4.2 * k / max(n - 1, 1)) for v in (0, 1)]) for k in range(n)])


def kernel_cases(n, seed=0):
    """(states n x 2 x 5, ctrl n x 2 x 2, par n x 16, w n x 2 x 5) for n scenarios: vehicle v of
    scenario k is boundary pair (2 k + v) % len(BOUNDARY), every third scenario a state of the
    executed path under a random admissible control instead; scenario k runs plant row k % len(ROWS)."""
    rng = np.random.default_rng(seed)
    states, ctrl = np.zeros((n, 2, 5)), np.zeros((n, 2, 2))
    path = path_states(n)
    for k in range(n):
        for v in (0, 1):
            if k % 3 == 2:
                states[k, v], ctrl[k, v] = path[k, v], rng.uniform((-3.0, -0.5), (3.0, 0.5))
            else:
                st, con = BOUNDARY[(2 * k + v) % len(BOUNDARY)]
                states[k, v], ctrl[k, v] = st, con
    par = np.stack([obca.feedback_row(**ROWS[k % len(ROWS)]) for k in range(n)])
    w = rng.normal(0.0, (0.3, 0.3, 0.1, 0.01, 0.005), (n, 2, 5))
    return states, ctrl, par, w


def bad_rows():
    """(field, value, a word of the refusal) for every way a plant row can be wrong."""
    return (("method", 2, "method"), ("method", 0.5, "method"), ("n_sub", 0, "n_sub"), ("n_sub", 65, "n_sub"),
            ("n_sub", 1.5, "n_sub"), ("lr", 0.0, "lr"), ("lr", -1.0, "lr"), ("lf", 0.0, "lf"), ("a_max", 0.0, "a_max"),
            ("w_max", -2.0, "w_max"), ("gain_a", np.inf, "finite"), ("gain_w", np.nan, "finite"),
            ("lr", np.nan, "finite"))
