"""Host side of the longest-first order of the device-resident OBCA-ADMM plan
(piadmm_obca_order_plan / piadmm_obca_order, include/piadmm.h): piadmm.obca.plan_order against a
hand-written insertion sort of the stated relation (Q descending, then I descending, then scenario
ascending, Q and I clamped to 2^21 - 1), piadmm.obca.plan_work on crafted status triples, and the
header's declarations.  No kernel runs here."""
import os
import re

import numpy as np
from conftest import ROOT

from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
CLAMP = 2 ** 21 - 1
ORDER_SYMBOLS = ("piadmm_obca_order_plan", "piadmm_obca_order")


def _before(a, b, work):
    """Scenario a sorts strictly before scenario b."""
    qa, ia = (min(int(v), CLAMP) for v in work[a])
    qb, ib = (min(int(v), CLAMP) for v in work[b])
    if qa != qb:
        return qa > qb
    if ia != ib:
        return ia > ib
    return a < b


def insertion_sort(lst, work):
    out = []
    for s in (int(v) for v in lst):
        k = len(out)
        while k > 0 and _before(s, out[k - 1], work):
            k -= 1
        out.insert(k, s)
    return out


def test_clamp_is_the_header_s():
    assert obca.ORDER_CLAMP == CLAMP
    assert "2^21 - 1" in open(HEADER).read()


def test_all_keys_equal_gives_ascending_scenarios():
    rng = np.random.default_rng(0)
    for val in (0, 7):
        work = np.full((40, 2), val, np.int32)
        lst = rng.permutation(40)
        assert obca.plan_order(lst, work).tolist() == list(range(40)) == insertion_sort(lst, work)


def test_q_ties_are_broken_by_i_then_by_index():
    work = np.array([[2, 1], [2, 5], [3, 0], [2, 5], [0, 9], [3, 0]], np.int32)
    got = obca.plan_order(np.arange(6), work)
    assert got.dtype == np.int32
    assert got.tolist() == [2, 5, 1, 3, 0, 4] == insertion_sort(range(6), work)


def test_seeded_inputs_and_a_shuffled_list():
    rng = np.random.default_rng(1)
    for n, hi in ((1, 3), (2, 3), (65, 3), (300, 3), (300, 60), (300, 10 ** 6)):
        work = rng.integers(0, hi, size=(n, 2)).astype(np.int32)
        want = insertion_sort(range(n), work)
        assert obca.plan_order(np.arange(n), work).tolist() == want
        for _ in range(3):                          # the order of the list itself does not matter
            assert obca.plan_order(rng.permutation(n), work).tolist() == want
        assert sorted(want) == list(range(n))


def test_sparse_scenarios_of_a_larger_n():
    rng = np.random.default_rng(2)
    n = 4096
    work = rng.integers(0, 4, size=(n, 2)).astype(np.int32)
    lst = rng.choice(n, size=257, replace=False)
    got = obca.plan_order(lst, work).tolist()
    assert got == insertion_sort(lst, work) == insertion_sort(sorted(lst), work)
    assert sorted(got) == sorted(lst.tolist())
    # the work of scenarios outside the list does not matter
    other = work.copy()
    mask = np.ones(n, bool)
    mask[lst] = False
    other[mask] = 99
    assert obca.plan_order(lst, other).tolist() == got


def test_values_above_the_clamp_compare_equal():
    work = np.array([[CLAMP, 0], [CLAMP + 5, 0], [CLAMP - 1, CLAMP + 9], [2 ** 31 - 1, 0], [CLAMP - 1, CLAMP],
                     [CLAMP, 1]], np.int32)
    got = obca.plan_order([5, 4, 3, 2, 1, 0], work).tolist()
    # Q at or above the clamp ties: I decides (scenario 5), then the index; likewise I of 2 and 4
    assert got == [5, 0, 1, 3, 2, 4] == insertion_sort([5, 4, 3, 2, 1, 0], work)


def test_plan_work_on_crafted_triples():
    m = 3
    li = np.zeros((2 * m, 3), np.int32)
    ei = np.zeros((m, obca.NT, 3), np.int32)
    li[:, 0], ei[:, :, 0] = 50, 50                  # the status column is never read
    # scenario 0: the local solves hold both maxima, in different records
    li[0] = (50, 4, 9)
    li[1] = (50, 6, 2)
    ei[0, :, 1:] = 1
    # scenario 1: the edge solves hold both maxima, in different slots
    li[2] = (50, 1, 1)
    li[3] = (50, 2, 2)
    ei[1, 6, 1], ei[1, 0, 2] = 60, 777
    # scenario 2: Q from a local solve, I from the last edge slot
    li[5] = (50, 0, 31)
    ei[2, 6, 1] = 13
    got = obca.plan_work(li, ei)
    assert got.dtype == np.int32 and got.shape == (m, 2)
    assert got.tolist() == [[9, 6], [777, 60], [31, 13]]
    assert obca.plan_work(np.zeros((0, 3), np.int32), np.zeros((0, obca.NT, 3), np.int32)).shape == (0, 2)


def test_the_new_symbols_are_declared_bound_and_outside_the_plan_set():
    src = open(HEADER).read()
    bound = {n for n, _, _ in _lib.SYMBOLS}
    for name in ORDER_SYMBOLS:
        assert re.search(rf"^\s*int32_t\s+{name}\s*\(", src, re.M), name
        assert name in bound, name
        assert not name.startswith("piadmm_obca_plan_"), name
    m = re.search(r"^#define PIADMM_OBCA_PLAN_GET_WORK (\d+)\s*$", src, re.M)
    assert m and int(m.group(1)) == 26 == obca.PLAN_GET["WORK"][0]
    assert obca.PLAN_GET["WORK"][1] is np.int32
