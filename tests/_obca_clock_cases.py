"""Cases of the per-scenario clocks of the OBCA plan (piadmm_obca_clock_plan), shared by the CPU
test (tests/test_obca_clock_host.py) and the GPU test (tests/test_gpu_obca_clock.py), and the hand
loops both compare piadmm.obca.clock_tick / clock_window against."""
import numpy as np

N_REF = 51
# the wave (1), workgroup (4 waves) and 256-entry compaction-tile boundaries of the two kernels
SIZES = (1, 4, 5, 64, 65, 256, 257)
C0 = (5, 8, 12)                      # the phases a mixed fleet cycles over: behind, closing, alongside


def alone_case(n, seed=0):
    """(clock n x 3, ran n, ref n x 2 x N_REF x 5) of one kernel-alone case: scenarios that tick
    and stay alive, that tick and retire exactly (c + 1 + 8 = len + 1), that stand exactly at the
    edge (c + 8 = len) without ticking, that are retired already, in a seeded mix."""
    rng = np.random.default_rng(100 * seed + n)
    length = rng.integers(8, N_REF + 1, n)
    kind = rng.integers(0, 4, n)
    c = np.where(kind == 0, rng.integers(0, N_REF, n) % np.maximum(length - 8, 1),     # well inside
                 np.where(kind == 3, length - 8 + rng.integers(1, 4, n), length - 8))  # past the edge / on it
    ran = np.where(kind == 2, 0, rng.integers(0, 2, n))
    ran[kind == 1] = 1                                                                 # on the edge and ticking: retires
    clock = np.stack((c, length, np.zeros(n, int)), axis=1)
    ref = rng.standard_normal((n, 2, N_REF, 5))
    return np.ascontiguousarray(clock, np.int32), np.ascontiguousarray(ran, np.int32), ref


def tick_by_hand(clock, ran):
    out = []
    for (c, length, _), r in zip(np.asarray(clock).tolist(), np.asarray(ran).tolist()):
        c = c + 1 if r else c
        out.append([c, length, 1 if c + 8 <= length else 0])
    return np.array(out, np.int32).reshape(-1, 3)


def window_by_hand(ref, clock):
    clock = np.asarray(clock)
    n = len(clock)
    out = np.zeros((n, 2, 8, 5))
    for s in range(n):
        c, _, alive = (int(x) for x in clock[s])
        if not alive:
            continue
        r = ref if np.ndim(ref) == 3 else ref[s]
        for v in range(2):
            for t in range(8):
                for j in range(5):
                    out[s, v, t, j] = r[v][c + t][j]
    return out
