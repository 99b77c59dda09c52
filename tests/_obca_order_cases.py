"""Inputs of the longest-first order tests (tests/test_gpu_obca_order.py): the lists and work
records the kernel-alone test sorts, and the seeds of the ordered plans."""
import numpy as np

CLAMP = 2 ** 21 - 1
# the wave and tile boundaries of a 64-lane stride and a 256-thread workgroup, and a long list
SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
KINDS = ("equal", "distinct", "ties", "subset", "clamp")
SUBSET_N = 4096


def alone_case(kind, m, seed=0):
    """(list of m distinct scenarios, work n x 2) of one kernel-alone case."""
    rng = np.random.default_rng(1000 * seed + m)
    n = SUBSET_N if kind == "subset" else m
    if kind == "equal":
        work = np.full((n, 2), 3)
        lst = rng.permutation(n)
    elif kind == "distinct":
        work = np.stack((rng.permutation(n), rng.integers(0, 60, n)), axis=1)
        lst = np.arange(n)
    elif kind == "ties":
        work = np.stack((rng.integers(0, 3, n), rng.integers(0, 2, n)), axis=1)
        lst = np.arange(n)
    elif kind == "subset":
        work = np.stack((rng.integers(0, 40, n), rng.integers(0, 8, n)), axis=1)
        lst = rng.choice(n, size=m, replace=False)
        if m > 1 and np.all(np.diff(lst) > 0):
            lst = lst[::-1]
    elif kind == "clamp":
        vals = np.array([CLAMP - 1, CLAMP, CLAMP + 1, 2 ** 31 - 1])
        work = np.stack((vals[rng.integers(0, 4, n)], vals[rng.integers(0, 4, n)]), axis=1)
        lst = rng.permutation(n)
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(lst, np.int32), np.ascontiguousarray(work, np.int32)


def reversing_work(n):
    """work_init under which the first list is the exact reverse of the identity: Q = s."""
    return np.ascontiguousarray(np.stack((np.arange(n), np.zeros(n, int)), axis=1), np.int32)


def random_work(n, seed):
    rng = np.random.default_rng(seed)
    return np.ascontiguousarray(np.stack((rng.integers(0, 5, n), rng.integers(0, 3, n)), axis=1), np.int32)
