"""Host side of the closed-loop feedback (piadmm_obca_feedback_*, piadmm_obca_propagate,
include/piadmm.h): the header's constants against the Python ones, the bindings, and the plant step
`obca.propagate` against the vehicle model written out from optimizer.py:75-77.  No kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_feedback_cases as C
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
SYMBOLS = ("piadmm_obca_propagate", "piadmm_obca_feedback_plan", "piadmm_obca_feedback_measure")


def _define(src, name):
    m = re.search(rf"^#define {name} (-?\d+)\s*$", src, re.M)
    assert m, name
    return int(m.group(1))


def test_header_constants_match_python():
    src = open(HEADER).read()
    assert _define(src, "PIADMM_OBCA_FEEDBACK_PAR") == obca.FEEDBACK_PAR == _lib.FEEDBACK_PAR == 16
    assert obca.FEEDBACK_PAR == 2 * len(obca.FEEDBACK_ROW)
    assert _define(src, "PIADMM_OBCA_PLAN_GET_FEEDBACK_PAR") == obca.PLAN_GET["FEEDBACK_PAR"][0] == 34
    assert _define(src, "PIADMM_OBCA_PLAN_GET_FEEDBACK_STEPS") == obca.PLAN_GET["FEEDBACK_STEPS"][0] == 35
    assert obca.PLAN_GET["FEEDBACK_PAR"][1] == np.float64 and obca.PLAN_GET["FEEDBACK_STEPS"][1] == np.int32
    codes = sorted(v[0] for v in obca.PLAN_GET.values())
    assert codes == list(range(len(codes)))


def test_symbols_are_bound_and_exported_and_the_abi_stays():
    bound = {n for n, _, _ in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int32_t\s+(piadmm_obca_(?:feedback_\w+|propagate))\s*\(", src, re.M))
    assert declared == set(SYMBOLS)
    for name in SYMBOLS:
        assert name in bound, name
        assert hasattr(lib, name), name
    assert _lib.load().piadmm_abi_version() == 7 and _define(src, "PIADMM_ABI_VERSION") == 7


def test_feedback_row_layout_and_defaults():
    row = obca.feedback_row()
    assert row.shape == (16,) and row.dtype == np.float64
    assert row.tolist() == [0, 1, 1.0, 1.5, 1, 1, 5, 20] * 2
    row = obca.feedback_row(method=1, n_sub=(4, 8), lr=(1.2, 0.9))
    assert row[:8].tolist() == [1, 4, 1.2, 1.5, 1, 1, 5, 20] and row[8:].tolist() == [1, 8, 0.9, 1.5, 1, 1, 5, 20]
    assert obca.feedback_row_check(row) is None
    with pytest.raises(AssertionError):
        obca.feedback_row(steps=3)


def _inside_states():
    """States of the executed path with admissible controls, and the boundary pairs that stay inside."""
    rng = np.random.default_rng(3)
    st = C.path_states(24)
    con = rng.uniform((-3.0, -0.5), (3.0, 0.5), (24, 2, 2))
    # pairs of boundary cases: vehicle 0 one, vehicle 1 the next
    nb = len(C.BOUNDARY_INSIDE)
    bst = np.array([[C.BOUNDARY_INSIDE[k][0], C.BOUNDARY_INSIDE[(k + 1) % nb][0]] for k in range(nb)])
    bcon = np.array([[C.BOUNDARY_INSIDE[k][1], C.BOUNDARY_INSIDE[(k + 1) % nb][1]] for k in range(nb)])
    return np.concatenate((st, bst)), np.concatenate((con, bcon))


def test_nominal_plant_is_the_nlp_transition_bit_for_bit():
    st, con = _inside_states()
    want = st + obca.DT * C.f(st, con)
    assert np.abs(want[..., 4]).max() <= obca.MAX_STEER          # the cases stay inside the steering limit
    for w in (None, np.zeros_like(st)):
        got = obca.propagate(st, con, obca.feedback_row(), w)
        # x + 0.0 == x but for the sign of a zero: compare values there, bits without w
        assert np.array_equal(got, want)
        if w is None:
            assert got.tobytes() == want.tobytes()
    # one row per scenario is the same statement
    got = obca.propagate(st, con, np.tile(obca.feedback_row(), (len(st), 1)))
    assert got.tobytes() == want.tobytes()
    # the disturbance is added after the step
    w = np.random.default_rng(4).normal(0, 0.1, st.shape)
    assert obca.propagate(st, con, obca.feedback_row(), w).tobytes() == (want + w).tobytes()


def test_nominal_plant_against_the_oracle_transition():
    """oracle/obca_oracle.py states the same transition with beta = atan(KB tan(delta)),
    KB = lr / (lr + lf) rounded once: one rounding apart in beta's argument, so the comparison is at a
    few ulp of the largest state (|x| <= 200: ulp 2.8e-14), not bit for bit."""
    from oracle import obca_oracle as O
    st, con = _inside_states()
    got = obca.propagate(st, con, obca.feedback_row())
    for k in range(len(st)):
        for v in (0, 1):
            want = O.dyn_eval(st[k, v], con[k, v])[0]
            assert np.abs(got[k, v] - want).max() <= 1e-13, (k, v)


def test_rk4_and_euler_agree_to_the_order_of_their_steps():
    """A smooth case (no limit is reached): Euler's error is first order in the substep, RK4's fourth.
    With RK4 at 64 substeps as the truth, halving Euler's substep halves its error (within 10 %), and
    doubling RK4's single substep divides its error by about 16 (at least 10); Euler at 64 substeps is
    then within its own first-order error of RK4 at 64."""
    st = C.path_states(9)
    st[..., 4] = np.linspace(-0.2, 0.2, 18).reshape(9, 2)
    con = np.tile(np.array([[1.5, 0.8], [-2.0, -0.6]]), (9, 1, 1))

    def run(method, n_sub):
        return obca.propagate(st, con, obca.feedback_row(method=method, n_sub=n_sub))
    truth = run(1, 64)
    e16, e32, e64 = (np.abs(run(0, k) - truth).max() for k in (16, 32, 64))
    assert 1.8 <= e16 / e32 <= 2.2 and 1.8 <= e32 / e64 <= 2.2, (e16, e32, e64)
    r1, r2 = (np.abs(run(1, k) - truth).max() for k in (1, 2))
    assert r1 / r2 >= 10.0 and r1 < e64, (r1, r2, e64)
    assert e64 <= 1.1 * e32 / 2


def test_saturation_cases():
    st = np.array([[[20.0, 0.0, 18.0, 0.0, 0.05]] * 2])
    # a beyond a_max: the plant accelerates at a_max
    got = obca.propagate(st, np.array([[[9.0, 0.0], [-9.0, 0.0]]]), obca.feedback_row())
    assert got[0, 0, 2] == 18.0 + obca.DT * 5.0 and got[0, 1, 2] == 18.0 + obca.DT * -5.0
    lim = obca.propagate(st, np.array([[[5.0, 0.0], [-5.0, 0.0]]]), obca.feedback_row())
    assert got.tobytes() == lim.tobytes()
    # delta reaches 0.6 mid-step: it stays there, and the heading turns less than unclipped Euler's would
    row = obca.feedback_row(n_sub=8)
    got = obca.propagate(st, np.array([[[0.0, 20.0], [0.0, -20.0]]]), row)
    assert got[0, 0, 4] == obca.MAX_STEER and got[0, 1, 4] == -obca.MAX_STEER
    free = st + 0.0
    for _ in range(8):
        free = free + (obca.DT / 8) * C.f(free, np.array([[[0.0, 20.0], [0.0, -20.0]]]))
    assert free[0, 0, 4] > 0.6 and 0.0 < got[0, 0, 3] < free[0, 0, 3]
    # gain_w = 0: the steering does not move, whatever omega
    got = obca.propagate(st, np.array([[[0.0, 7.0], [0.0, -7.0]]]), obca.feedback_row(gain_w=0.0))
    assert (got[..., 4] == 0.05).all()
    # omega beyond w_max acts as w_max
    a = obca.propagate(st, np.array([[[0.0, 30.0]] * 2]), obca.feedback_row(w_max=2.0))
    b = obca.propagate(st, np.array([[[0.0, 2.0]] * 2]), obca.feedback_row(w_max=2.0))
    assert a.tobytes() == b.tobytes()


def test_row_validation_refuses_every_bad_field():
    st, con = C.path_states(2), np.zeros((2, 2, 2))
    for field, value, word in C.bad_rows():
        for veh in (0, 1):
            pair = [obca._FEEDBACK_DEFAULT[field]] * 2
            pair[veh] = value
            row = obca.feedback_row(**{field: tuple(pair)})
            why = obca.feedback_row_check(row)
            assert why is not None and word in why, (field, value, why)
            rows = np.stack([obca.feedback_row(), row])
            # refused before anything else: also with states that are not finite
            with pytest.raises(ValueError, match="row 1"):
                obca.propagate(st * np.nan, con, rows)


def test_feedback_args():
    par, tape = obca.feedback_args(3, dict())
    assert par.shape == (1, 16) and tape is None and par[0].tobytes() == obca.feedback_row().tobytes()
    par, tape = obca.feedback_args(3, dict(par=np.tile(obca.feedback_row(method=1), (3, 1)), tape=np.zeros((3, 4, 2, 5))))
    assert par.shape == (3, 16) and tape.shape == (3, 4, 2, 5)
    with pytest.raises(AssertionError):
        obca.feedback_args(3, dict(tape=np.zeros((2, 4, 2, 5))))
