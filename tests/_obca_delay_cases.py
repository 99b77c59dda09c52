"""Cases of the communication-delay tests (tests/test_obca_delay_host.py, tests/test_gpu_obca_delay.py):
the kernel's shapes, streams and seeds, the delay rows, the states of the stale message and the one
tolerance of the GPU tests."""
import numpy as np

from piadmm import obca

# k_plan_delay against obca.delay_tau: the words and the uniforms are exact, the device's log, sqrt
# and cos are not NumPy's.  DELAY_MEASURED is the largest absolute deviation of the device's latency
# from the NumPy statement measured on an MI355X over every case of `kernel_cases` under UNIT_ROW
# (tau = clip(0.05 + 0.025 z) inside [0, 0.1]: one ulp of a tau between 1/16 and 1/8); the bound is
# 8 times it, the margin for libm differences between ROCm releases.  Every other GPU assertion on
# tau is bit equality.
DELAY_MEASURED = 1.387779e-17
DELAY_TOL = 8 * DELAY_MEASURED

PW = 4                                  # waves per workgroup of the plan's kernels (csrc/piadmm_obca_plan.h)
# scenarios: 2n lanes at the wave boundary (31, 32, 33) and at the workgroup boundary (32 PW -+ 1)
KERNEL_SIZES = (1, 31, 32, 33, 32 * PW - 1, 32 * PW + 1)
CAPS = (1, 3)
STREAM_EDGES = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1)
SEEDS = (0, 2 ** 32, 2 ** 64 - 1)
K0S = (0, 2 ** 31 - 4)
# scenarios of the stale message alone: one wave each, so PW is the workgroup boundary
EXCHANGE_SIZES = (1, PW - 1, PW, PW + 1, 129)

# the latency the tightening was designed for, per vehicle a little apart
UNIT_ROW = obca.delay_row(avg=(obca.AVG_DELAY, 0.04), std=(obca.VAR_DELAY, 0.03))
ZERO_ROW = obca.delay_row()             # avg = std = 0, tau_max = DT: tau = 0, or the tape alone


def streams_for(n):
    """n stream ids: the four edges first (as many as fit), then ids spread over [0, 2^63)."""
    rest = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(1)).astype(np.int64)
    out = rest.copy()
    k = min(n, len(STREAM_EDGES))
    out[:k] = np.array(STREAM_EDGES[:k], np.int64)
    return out


def kernel_cases():
    """(n, cap, streams, seed, k0) of every kernel case: every size at every cap, the seeds and step
    offsets going round so that each appears with each cap."""
    out, i = [], 0
    for n in KERNEL_SIZES:
        for cap in CAPS:
            out.append((n, cap, streams_for(n), SEEDS[i % len(SEEDS)], K0S[(i // len(SEEDS)) % len(K0S)]))
            i += 1
    return out


def bad_rows():
    """(row, a word of the refusal) for every way a delay row can be wrong."""
    def row(at, value):
        r = obca.delay_row(avg=0.05, std=0.025, tau_max=0.09, trunc=3.0)
        r[at] = value
        return r
    above = np.nextafter(obca.DT, 1.0)
    return ((row(0, -1e-300), "avg"), (row(1, -1.0), "avg"), (row(2, -1e-300), "std"), (row(3, -2.0), "std"),
            (row(4, -1e-300), "tau_max"), (row(5, above), "tau_max"), (row(4, 1.0), "tau_max"),
            (row(6, -1.0), "trunc"), (row(7, 1.0), "reserved"), (row(7, -1e-300), "reserved"),
            (row(0, np.nan), "finite"), (row(1, np.inf), "finite"), (row(2, np.nan), "finite"),
            (row(3, np.inf), "finite"), (row(4, np.nan), "finite"), (row(5, -np.inf), "finite"),
            (row(6, np.inf), "finite"), (row(6, np.nan), "finite"), (row(7, np.nan), "finite"))


def exchange_states(n, seed=0):
    """n x 2 x 8 x 5 local states for the stale message alone: constant-acceleration paths with the
    heading turning, and in the first scenarios (as many as fit) the hard entries: theta next to
    +pi and -pi, v = 0 throughout, a -0.0 in every column, a path that does not move at all."""
    rng = np.random.default_rng(seed)
    X = np.zeros((n, 2, 8, 5))
    t = np.arange(8) * obca.DT
    for s in range(n):
        for v in (0, 1):
            x0, y0 = rng.uniform(-100.0, 100.0), rng.uniform(-10.0, 10.0)
            vel, acc = rng.uniform(0.0, 20.0), rng.uniform(-3.0, 3.0)
            th0, om = rng.uniform(-np.pi, np.pi), rng.uniform(-0.5, 0.5)
            X[s, v, :, 2] = vel + acc * t
            X[s, v, :, 3] = th0 + om * t
            X[s, v, :, 0] = x0 + np.cumsum(X[s, v, :, 2] * np.cos(X[s, v, :, 3])) * obca.DT
            X[s, v, :, 1] = y0 + np.cumsum(X[s, v, :, 2] * np.sin(X[s, v, :, 3])) * obca.DT
            X[s, v, :, 4] = rng.uniform(-0.6, 0.6, 8)
    X[0, 0, :, 3] = np.pi - 1e-9 * np.arange(8)             # next to +pi
    X[0, 1, :, 3] = -np.pi + 1e-9 * np.arange(8)            # next to -pi
    if n > 1:
        X[1, 0, :, 2] = 0.0                                 # v = 0
        X[1, 1, 3] = -0.0                                   # a -0.0 in every column of one slot
        X[1, 1, 4] = np.array([0.0, -0.0, 0.0, -0.0, 0.0])
    if n > 2:
        X[2, 0] = X[2, 0, 0]                                # the same state at every slot
        X[2, 1, :, 3] = np.array([np.pi, -np.pi, np.pi, np.pi, -np.pi, -np.pi, np.pi, -np.pi])   # across the cut
    return X


def exchange_taus(n, seed=0):
    """n x 2 latencies in [0, DT]: 0, DT, one ulp above 0, one ulp below DT and values inside,
    going round over the vehicles so that every scenario size sees the edge values."""
    rng = np.random.default_rng(seed + 1)
    edge = np.array([0.0, obca.DT, 5e-324, np.nextafter(obca.DT, 0.0), obca.AVG_DELAY, 0.5 * obca.DT, 1e-9])
    tau = rng.uniform(0.0, obca.DT, (n, 2))
    k = np.arange(2 * n)
    flat = tau.reshape(-1)
    use = k % 3 != 2                                        # two of three entries from the edge values
    flat[use] = edge[(k[use] // 3 * 2 + k[use] % 3) % len(edge)]
    return tau
