"""k_plan_clearance (csrc/piadmm_obca_plan_trace.hip) behind piadmm_obca_clearance against its host
restatement piadmm.obca.clearance, on the crafted geometry and the 70 seeded random pairs of
tests/_obca_clearance_cases.py, at n = 1 (a lone wave), 5 (a partial second workgroup) and 70.

Bar: 1e-12 absolute, for the reason of the `b` bar of tests/test_gpu_obca_plan.py -- host and
device sin / cos stand within a few ulp of each other and the coordinates are at most
max_x + max_y = 170, so every vertex, and with it every distance, moves by a few 1e-14 at the most.
The zero / non-zero decision is compared where the host's largest SAT gap stands at least 1e-9 from
0; closer cases are counted and the count must be 0 (the cases were chosen so, and the CPU test
asserts it of the host values)."""
import numpy as np
import pytest

import _obca_clearance_cases as C
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

BAR = 1e-12


@pytest.fixture(scope="module")
def batch():
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    b = obca.OBCABatch(0)
    yield b
    b.close()


@pytest.fixture(scope="module")
def host():
    """(states, prob, host clearances n x 2, host SAT gaps n x 2), computed once."""
    states, prob = C.all_cases()
    want = np.array([obca.clearance(sp, p) for sp, p in zip(states, prob)])
    gaps = np.array([[obca.box_clearance(obca.vehicle_box(sp[0], p, t), obca.vehicle_box(sp[1], p, t))[1]
                      for t in (False, True)] for sp, p in zip(states, prob)])
    return states, prob, want, gaps


@pytest.fixture(scope="module")
def alone(batch, host):
    """Every pair run alone (n = 1)."""
    states, prob = host[0], host[1]
    return np.concatenate([batch.clearance(states[k:k + 1], prob[k:k + 1]) for k in range(len(states))])


def _compare(got, want, gaps):
    assert got.shape == want.shape
    near = int((np.abs(gaps) < C.MARGIN).sum())
    assert near == 0, near
    assert np.array_equal(got == 0.0, want == 0.0), np.nonzero((got == 0.0) != (want == 0.0))
    dev = float(np.abs(got - want).max())
    assert dev <= BAR, dev
    return dev


def test_lone_waves(host, alone):
    _, prob, want, gaps = host
    dev = _compare(alone, want, gaps)
    print(f"clearance, every pair alone: max |device - host| {dev:.3e}")
    for k, (name, _, _, closed) in enumerate(C.crafted()):
        # the host stands within 1e-13 of the closed form (tests/test_obca_clearance_host.py)
        assert abs(alone[k, 0] - closed) <= BAR + 1e-13, (name, alone[k, 0], closed)
    assert np.array_equal(alone[prob == 0, 0], alone[prob == 0, 1])       # prob = 0: the plain value twice
    assert np.any(alone[prob == 1, 0] != alone[prob == 1, 1])             # prob = 1: the boxes moved


def test_partial_workgroup(batch, host, alone):
    states, prob, want, gaps = host
    n_cr = len(C.crafted())
    for lo in range(0, n_cr, 5):
        got = batch.clearance(states[lo:lo + 5], prob[lo:lo + 5])
        _compare(got, want[lo:lo + 5], gaps[lo:lo + 5])
        assert got.tobytes() == alone[lo:lo + 5].tobytes()


def test_seventy_pairs_and_position_independence(batch, host, alone):
    states, prob, want, gaps = host
    lo = len(C.crafted())
    got = batch.clearance(states[lo:], prob[lo:])
    assert got.shape == (70, 2)
    dev = _compare(got, want[lo:], gaps[lo:])
    print(f"clearance, 70 pairs: max |device - host| {dev:.3e}, {int((got[:, 0] == 0).sum())} overlapping")
    # every scenario equals its run alone, bit for bit
    assert got.tobytes() == alone[lo:].tobytes()
    # one value for every pair when prob is a scalar
    assert batch.clearance(states[lo:], 0)[:, 1].tobytes() == got[:, 0].tobytes()


def test_bad_arguments_before_any_device_call(batch, host):
    states, prob = host[0][:4].copy(), host[1][:4].copy()
    lib, h = batch._lib, batch._h
    out = np.full((4, 2), -7.0)
    call = lambda n, s, p, o: lib.piadmm_obca_clearance(h, n, _lib.dptr(s), _lib.iptr(p), _lib.dptr(o))  # noqa: E731
    assert call(0, states, prob, out) == _lib.E_ARG
    assert call(-3, states, prob, out) == _lib.E_ARG
    assert call(4, None, prob, out) == _lib.E_ARG
    assert call(4, states, None, out) == _lib.E_ARG
    assert call(4, states, prob, None) == _lib.E_ARG
    bad_p = prob.copy()
    bad_p[2] = 2
    assert call(4, states, bad_p, out) == _lib.E_ARG
    assert b"prob[2]" in lib.piadmm_obca_last_error(h)
    for val in (np.nan, np.inf, -np.inf):
        bad_s = states.copy()
        bad_s[3, 1, 3] = val
        assert call(4, bad_s, prob, out) == _lib.E_ARG
        assert b"pair 3" in lib.piadmm_obca_last_error(h)
    assert np.all(out == -7.0)                       # nothing was written
    assert call(4, states, prob, out) == 0 and np.all(out >= 0.0)
