"""State pairs for the clearance kernel, shared by the CPU test (tests/test_obca_clearance_host.py)
and the GPU test (tests/test_gpu_obca_clearance.py): crafted geometry with its closed-form plain
clearance, and 70 seeded random pairs (about half of them overlapping).  Coordinates stay inside
the planner's box (|x| <= 150, |y| <= 20).  The seed is one at which no pair, crafted or random,
stands within MARGIN of the zero / non-zero decision in either box set; the CPU test asserts it."""
import math

import numpy as np

from piadmm import obca

MARGIN = 1e-9
SEED = 11
L, W = obca.LENGTH, obca.WIDTH


def _pair(x0, y0, th0, x1, y1, th1, v0=15.0, v1=10.0):
    return np.array([[x0, y0, v0, th0, 0.0], [x1, y1, v1, th1, 0.0]])


def crafted():
    """[(name, state pair 2 x 5, prob, the plain clearance in closed form)]."""
    reach = math.hypot(L, W) / 2 * math.cos(math.atan2(W, L) - math.pi / 4)
    return [
        ("side by side", _pair(50.0, 4.0, 0.0, 51.0, 0.0, 0.0), 1, 4.0 - W),
        ("side by side, close", _pair(120.0, -2.5, 0.0, 118.0, 0.0, 0.0), 0, 2.5 - W),
        ("nose to tail", _pair(10.0, 0.0, 0.0, 15.0, 0.5, 0.0), 1, 5.0 - L),
        ("tail to nose", _pair(40.0, 1.0, math.pi, 33.0, 1.0, math.pi), 0, 7.0 - L),
        ("corner to corner", _pair(0.0, 0.0, 0.0, L + 1.5, W + 0.7, 0.0), 1, math.hypot(1.5, 0.7)),
        ("corner to corner, far", _pair(149.0, -19.0, 0.0, 149.0 - L - 30.0, -19.0 + W + 5.0, 0.0), 0,
         math.hypot(30.0, 5.0)),
        ("45 degrees facing an edge", _pair(0.0, 0.0, 0.0, 6.0, 0.0, math.pi / 4), 1, 6.0 - L / 2 - reach),
        ("overlapping", _pair(0.0, 0.0, 0.0, 2.0, 0.5, 0.4), 1, 0.0),
        ("overlapping, crossed", _pair(80.0, 3.0, 0.0, 80.5, 3.0, math.pi / 2), 0, 0.0),
        ("coincident", _pair(3.0, 1.0, 0.2, 3.0, 1.0, 0.2), 1, 0.0),
    ]


def random_pairs(n=70, seed=SEED):
    """(states n x 2 x 5, prob n): vehicle 1 within 7 m x 5 m of vehicle 0, any headings, speeds up to 20."""
    rng = np.random.default_rng(seed)
    states = np.zeros((n, 2, 5))
    for k in range(n):
        x0, y0 = rng.uniform(10.0, 140.0), rng.uniform(-14.0, 14.0)
        states[k] = _pair(x0, y0, rng.uniform(-math.pi, math.pi), x0 + rng.uniform(-7.0, 7.0),
                          y0 + rng.uniform(-5.0, 5.0), rng.uniform(-math.pi, math.pi), v0=rng.uniform(0.0, 20.0),
                          v1=rng.uniform(0.0, 20.0))
    return states, rng.integers(0, 2, n).astype(np.int32)


def all_cases():
    """The crafted pairs, then the random ones: (states, prob)."""
    cr = crafted()
    rs, rp = random_pairs()
    return (np.ascontiguousarray(np.concatenate([np.stack([c[1] for c in cr]), rs])),
            np.concatenate([np.array([c[2] for c in cr], np.int32), rp]))
