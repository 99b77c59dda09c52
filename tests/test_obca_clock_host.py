"""Host side of the per-scenario clocks of the OBCA plan (piadmm_obca_clock_plan / _clock_admit /
_clock_tick, include/piadmm.h): the pure restatements piadmm.obca.clock_tick / clock_window against
hand-written loops, retirement exactly at c + 8 > len, the header's names and items and the
bindings.  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_clock_cases as K
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
CLOCK_SYMBOLS = {"piadmm_obca_clock_plan": 3, "piadmm_obca_clock_admit": 10, "piadmm_obca_clock_tick": 11}


@pytest.mark.parametrize("n", K.SIZES)
def test_tick_and_window_against_hand_loops(n):
    clock, ran, ref = K.alone_case(n)
    clock_in, ran_in = clock.copy(), ran.copy()
    got = obca.clock_tick(clock, ran)
    assert got.dtype == np.int32 and got.shape == (n, 3)
    assert np.array_equal(clock, clock_in) and np.array_equal(ran, ran_in)      # the arguments stay
    want = K.tick_by_hand(clock, ran)
    assert got.tolist() == want.tolist()
    win = obca.clock_window(ref, got)
    assert win.shape == (n, 2, 8, 5)
    assert win.tobytes() == K.window_by_hand(ref, want).tobytes()
    # one shared reference for all
    assert obca.clock_window(ref[0], got).tobytes() == K.window_by_hand(ref[0], want).tobytes()
    # a retired scenario's window is zero, an alive one's are the reference's own rows
    for s in range(n):
        c, _, alive = got[s]
        assert (win[s] == ref[s, :, c:c + 8]).all() if alive else not win[s].any()


def test_the_kernel_alone_cases_cover_both_sides_of_the_edge():
    clock, ran, _ = K.alone_case(257)
    out = K.tick_by_hand(clock, ran)
    before = clock[:, 0] + 8 <= clock[:, 1]
    assert (before & (out[:, 2] == 0)).any()            # retires in this tick
    assert (before & (out[:, 2] == 1) & (ran == 1)).any() and (before & (ran == 0)).any()
    assert (~before).any()                              # retired before
    assert (out[:, 0] + 8 == out[:, 1]).any()           # stands exactly on the edge, alive


def test_retirement_is_exactly_at_c_plus_8_above_len():
    n_ref = 20
    ref = np.arange(2 * n_ref * 5, dtype=np.float64).reshape(2, n_ref, 5)
    clock = np.array([[0, 10, 1], [0, n_ref, 1]], np.int32)
    alive = []
    for step in range(15):
        alive.append(clock[:, 2].tolist())
        win = obca.clock_window(ref, clock)
        for s in range(2):
            if clock[s, 2]:
                assert clock[s, 0] + 8 <= clock[s, 1]
                assert win[s, 1, 7, 4] == ref[1, clock[s, 0] + 7, 4]            # the last row read is a valid one
        clock = obca.clock_tick(clock, clock[:, 2])
    # len 10: the steps c = 0, 1, 2 run (c + 8 <= 10), the tick to c = 3 retires; len 20: c = 0 .. 12
    assert [a[0] for a in alive] == [1, 1, 1] + [0] * 12
    assert [a[1] for a in alive] == [1] * 13 + [0] * 2
    assert clock.tolist() == [[3, 10, 0], [13, n_ref, 0]]                       # a retired clock stands still
    # a tick of a scenario that did not run changes nothing
    assert obca.clock_tick([[2, 10, 1]], [0]).tolist() == [[2, 10, 1]]
    assert obca.clock_tick([[2, 10, 1]], [1]).tolist() == [[3, 10, 0]]


def test_clock_rows():
    assert obca.clock_rows(3, True, 7, 51).tolist() == [[7, 51]] * 3
    rows = obca.clock_rows(2, [[5, 51], [8, 20]], 7, 51)
    assert rows.dtype == np.int32 and rows.tolist() == [[5, 51], [8, 20]]


def test_the_header_declares_the_names_and_items_and_lib_binds_them():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int32_t\s+(piadmm_obca_clock_\w+)\s*\(", src, re.M))
    assert declared == set(CLOCK_SYMBOLS)
    assert not any(name.startswith("piadmm_obca_plan_") for name in declared)
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in CLOCK_SYMBOLS.items():
        assert name in bound and len(bound[name]) == nargs, name
        assert hasattr(lib, name), name
        decl = re.search(rf"int32_t\s+{name}\s*\(([^;]*)\);", re.sub(r"/\*.*?\*/", "", src, flags=re.S)).group(1)
        assert len(decl.split(",")) == nargs, name
    codes = {name: int(v) for name, v in re.findall(r"^#define PIADMM_OBCA_PLAN_GET_(\w+) (\d+)\s*$", src, re.M)}
    assert codes["CLOCK"] == 27 == obca.PLAN_GET["CLOCK"][0] and obca.PLAN_GET["CLOCK"][1] is np.int32
    assert codes["WINDOW"] == 28 == obca.PLAN_GET["WINDOW"][0] and obca.PLAN_GET["WINDOW"][1] is np.float64
    assert _lib.load().piadmm_abi_version() == 7
    # the sentence that made t_step the plan's alone is gone
    assert "t_step are the plan's" not in re.sub(r"\s*\*\s*", " ", src) and "piadmm_obca_clock_plan, below" in src


def test_the_calls_refuse_bad_arguments_before_any_device_call():
    """The checks that stand before the first device call answer without a GPU: a null handle, and
    on a handle (where one can be made) a bad n, a null pointer, a row out of range."""
    lib = _lib.load()
    assert lib.piadmm_obca_clock_plan(None, 1, None) == _lib.E_ARG
    assert lib.piadmm_obca_clock_admit(None, 1, None, None, None, None, None, None, None, None) == _lib.E_ARG
    assert lib.piadmm_obca_clock_tick(None, 1, None, None, None, 1, 8, None, None, None, None) == _lib.E_ARG
