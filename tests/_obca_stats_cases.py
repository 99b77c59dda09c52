"""Cases of the fleet statistics tests (tests/test_obca_stats_host.py, tests/test_gpu_obca_stats.py):
the inputs of the kernels alone and the field-by-field bit comparison of two results.

Every comparison in these tests is bit equality against obca.fleet_stats_host or against slices of
trace_get: there is no tolerance anywhere."""
import dataclasses

import numpy as np

from piadmm import obca

ST = 128                                # scenarios per workgroup of the statistics kernels (csrc/piadmm_obca_plan_trace.hip)
# one lane, a wave boundary on either side, more than one workgroup of partials, an odd tail
SIZES = (1, 2, 63, 64, 65, 130, 1000)
ROWS = (0, 1, 3)
# B = 1, 5, 64: every edge is a value the inputs take (VALUES), so values sit on edges
EDGES = {1: np.array([0.5]), 5: np.array([0.0, 0.25, 0.5, 1.0, 2.0]), 64: np.arange(64) * 0.125}
# a small set: many exact ties across wave and workgroup boundaries; -0.0 ties with 0.0 and keeps its sign
VALUES = np.array([0.0, -0.0, 0.125, 0.25, 0.5, 1.0, 2.0, 4.0, 7.875, 8.5, -1.0])
NOT_FINITE = np.array([np.nan, np.inf, -np.inf])
MASKS = np.array([1, 1, 1, 0, 3, 2, 5, 9], np.int32)    # mostly converged alone; some with another bit, some empty


def same(got, want, msg=""):
    """Every field of two OBCAFleetStats bit for bit: dtype, shape and bytes."""
    for f in dataclasses.fields(obca.OBCAFleetStats):
        a, b = getattr(got, f.name), getattr(want, f.name)
        if isinstance(b, np.ndarray):
            assert isinstance(a, np.ndarray) and a.dtype == b.dtype and a.shape == b.shape, (msg, f.name, a, b)
            assert a.tobytes() == b.tobytes(), (msg, f.name, a, b)
        else:
            assert type(a) is int and a == b, (msg, f.name, a, b)


def kernel_case(n, R, variant="ties", seed=0):
    """(clear (R + 1) x n x 2, summary n x 4, iters R x n, mask R x n x 2) for the kernels alone.

    ties       values drawn from VALUES with one value in eight not finite
    tail       as ties, but -2.0, below everything else, sits in the last scenario alone (the last lane
               of the last workgroup) of both minima and of every row
    nonfinite  every clearance and every minimum is NaN, +inf or -inf
    The iterate sums are near 2^31 per scenario, so their sum passes 2^32 from n = 3 on."""
    rng = np.random.default_rng(1000 * n + 10 * R + seed)

    def draw(shape):
        x = rng.choice(VALUES, shape)
        bad = rng.random(shape) < (1.0 if variant == "nonfinite" else 0.125)
        return np.where(bad, rng.choice(NOT_FINITE, shape), x)
    clear = draw((R + 1, n, 2))
    summary = np.zeros((n, 4))
    summary[:, 0], summary[:, 2] = draw(n), draw(n)
    summary[:, 1] = rng.integers(0, R + 1, n)
    summary[:, 3] = 2.0 ** 31 - 1 - (np.arange(n) % 7)
    if variant == "tail":
        clear[:, n - 1, :] = -2.0
        summary[n - 1, 0] = summary[n - 1, 2] = -2.0
    iters = rng.integers(0, 51, (R, n)).astype(np.int32)
    mask = rng.choice(MASKS, (R, n, 2)).astype(np.int32)
    return clear, summary, iters, mask
