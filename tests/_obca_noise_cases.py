"""Cases of the device-side noise tests (tests/test_obca_noise_host.py, tests/test_gpu_obca_noise.py):
the generator's known answers, the kernel's shapes, streams and seeds, and the one tolerance of the
GPU tests."""
import numpy as np

from piadmm import obca

# k_plan_noise against obca.noise_tape: the words and the uniforms are exact, the device's log, sqrt,
# cos and sin are not NumPy's.  NOISE_MEASURED is the largest absolute deviation of the device's
# standard normals (sigma 1, bias 0, no truncation) from the NumPy statement measured on an MI355X
# over every case of `kernel_cases` (2 ulp of a z between 1 and 2, 1 ulp of one between 2 and 4;
# the largest |z| of the cases is 4.04); the bound is 8 times it, the margin for libm differences
# between ROCm releases.  Every other GPU assertion is bit equality.
NOISE_MEASURED = 4.440892e-16
NOISE_TOL = 8 * NOISE_MEASURED

# Philox4x32-10 known answers: (counter, key, result)
KNOWN = (
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
)

PW = 4                                  # waves per workgroup of the plan's kernels (csrc/piadmm_obca_plan.hip)
# scenarios: 2n lanes at the wave boundary (31, 32, 33) and at the workgroup boundary (32 PW -+ 1)
KERNEL_SIZES = (1, 31, 32, 33, 32 * PW - 1, 32 * PW + 1)
CAPS = (1, 3)
# stream ids at the edges of both counter words, seeds at the edges of both key words, step indices
# at both ends of their range (k0 + cap <= 2^31 for every cap of CAPS)
STREAM_EDGES = (0, 2 ** 32 - 1, 2 ** 32, 2 ** 63 - 1)
SEEDS = (0, 2 ** 32, 2 ** 64 - 1)
K0S = (0, 2 ** 31 - 4)

SIGMA = (0.05, 0.05, 0.02, 0.002, 0.001)     # a plausible disturbance of (x, y, v, theta, delta)


def streams_for(n):
    """n stream ids: the four edges first (as many as fit), then ids spread over [0, 2^63)."""
    rest = (np.arange(n, dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) >> np.uint64(1)).astype(np.int64)
    out = rest.copy()
    k = min(n, len(STREAM_EDGES))
    out[:k] = np.array(STREAM_EDGES[:k], np.int64)
    return out


def kernel_cases():
    """(n, cap, streams, seed, k0) of every kernel case: every size at every cap, the seeds and step
    offsets going round so that each appears with each cap; n = 1 at stream 0, seed 0, k0 0 first."""
    out, i = [], 0
    for n in KERNEL_SIZES:
        for cap in CAPS:
            out.append((n, cap, streams_for(n), SEEDS[i % len(SEEDS)], K0S[(i // len(SEEDS)) % len(K0S)]))
            i += 1
    return out


def all_clipped_streams(seed, k0, cap, want, trunc):
    """`want` stream ids, ascending from 0, all of whose standard normals at step indices k0 ..
    k0 + cap - 1 are beyond +-trunc in the NumPy statement by a factor of two: the clipped rows are
    then +-trunc exactly on the device as well."""
    ids = np.arange(64 * want, dtype=np.int64)
    z = np.stack([obca.noise_normal(seed, ids, k0 + i) for i in range(cap)], axis=1)
    good = ids[(np.abs(z) > 2.0 * trunc).all(axis=(1, 2, 3))]
    assert len(good) >= want, len(good)
    return good[:want]


def bad_rows():
    """(row, a word of the refusal) for every way a noise row can be wrong."""
    def row(at, value):
        r = obca.noise_row(sigma=SIGMA, bias=0.01, trunc=3.0)
        r[at] = value
        return r
    return ((row(0, -1e-300), "sigma"), (row(9, -1.0), "sigma"), (row(3, np.nan), "finite"), (row(7, np.inf), "finite"),
            (row(12, np.inf), "finite"), (row(19, np.nan), "finite"), (row(20, -1.0), "trunc"),
            (row(20, np.nan), "finite"), (row(20, np.inf), "finite"), (row(21, 1.0), "reserved"))
