"""Host side of the clearance record: piadmm.obca.clearance (the host restatement of
k_plan_clearance, csrc/piadmm_obca_plan_trace.hip) against closed forms and against a brute-force
restatement, the tightened boxes against the offset of util.py:83-99 written out, and the header
and bindings of piadmm_obca_clearance / piadmm_obca_trace_*.  No kernel runs here."""
import ctypes
import math
import os
import re

import numpy as np
from conftest import ROOT

import _obca_clearance_cases as C
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
NEW_SYMBOLS = ("piadmm_obca_clearance", "piadmm_obca_trace_begin", "piadmm_obca_trace_run", "piadmm_obca_trace_get",
               "piadmm_obca_trace_end")
L, W = obca.LENGTH, obca.WIDTH


def _pair(x0, y0, th0, x1, y1, th1, v0=15.0, v1=10.0):
    return np.array([[x0, y0, v0, th0, 0.0], [x1, y1, v1, th1, 0.0]])


def test_closed_forms():
    tol = 1e-13
    # side by side, axis-aligned: gap = lane - WIDTH
    for lane in (2.5, 3.0, 4.0):
        assert abs(obca.clearance(_pair(50.0, lane, 0.0, 51.0, 0.0, 0.0), 0)[0] - (lane - W)) <= tol
    # nose to tail: gap = dx - LENGTH
    for dx in (3.6, 5.0, 20.0):
        assert abs(obca.clearance(_pair(10.0, 0.0, 0.0, 10.0 + dx, 0.5, 0.0), 0)[0] - (dx - L)) <= tol
    # corner to corner
    gx, gy = 1.5, 0.7
    got = obca.clearance(_pair(0.0, 0.0, 0.0, L + gx, W + gy, 0.0), 0)[0]
    assert abs(got - math.hypot(gx, gy)) <= tol
    # the same turned as a whole by 0.3 rad about the origin
    c, s = math.cos(0.3), math.sin(0.3)
    got = obca.clearance(_pair(0.0, 0.0, 0.3, c * (L + gx) - s * (W + gy), s * (L + gx) + c * (W + gy), 0.3), 0)[0]
    assert abs(got - math.hypot(gx, gy)) <= tol
    # box 1 rotated 45 degrees, a corner facing box 0's front edge: its corner reaches
    # hypot(L, W) / 2 * cos(atan2(W, L) - pi / 4) towards box 0
    dx = 6.0
    reach = math.hypot(L, W) / 2 * math.cos(math.atan2(W, L) - math.pi / 4)
    got = obca.clearance(_pair(0.0, 0.0, 0.0, dx, 0.0, math.pi / 4), 0)[0]
    assert abs(got - (dx - L / 2 - reach)) <= tol
    # overlapping, and coincident
    assert obca.clearance(_pair(0.0, 0.0, 0.0, 2.0, 0.5, 0.4), 0) == (0.0, 0.0)
    assert obca.clearance(_pair(3.0, 1.0, 0.2, 3.0, 1.0, 0.2), 1) == (0.0, 0.0)
    # the order of the two vehicles does not matter
    sp = _pair(3.0, 1.0, 0.2, 8.0, 2.5, -0.6)
    assert obca.clearance(sp, 0)[0] == obca.clearance(sp[::-1], 0)[0] > 0.0


def test_crafted_cases_carry_their_closed_form():
    for name, sp, prob, want in C.crafted():
        got = obca.clearance(sp, prob)[0]
        assert abs(got - want) <= 1e-13, (name, got, want)


def _boundary(box, m):
    v = np.array([obca._box_vertex(box, i) for i in range(4)])
    t = np.arange(m)[:, None] / m
    return np.concatenate([v[i] + t * (v[(i + 1) % 4] - v[i]) for i in range(4)])


def test_against_brute_force():
    """Both boundaries sampled at 2000 points per edge: the sampled minimum is >= the exact one and
    exceeds it by at most the sample spacing (each closest point has a sample within half of it)."""
    from scipy.spatial import cKDTree
    m = 2000
    spacing = L / m
    rng = np.random.default_rng(20240)
    n_zero = 0
    for k in range(200):
        x0, y0 = rng.uniform(0, 140), rng.uniform(-10, 10)
        sp = _pair(x0, y0, rng.uniform(-math.pi, math.pi), x0 + rng.uniform(-7, 7), y0 + rng.uniform(-5, 5),
                   rng.uniform(-math.pi, math.pi))
        b0, b1 = obca.vehicle_box(sp[0]), obca.vehicle_box(sp[1])
        exact, gap = obca.box_clearance(b0, b1)
        # the minimum over all 8000 x 8000 sample pairs: a pass over every 40th point of one
        # boundary bounds it, which lets the tree discard far points in the pass over all of them
        pts, tree = _boundary(b0, m), cKDTree(_boundary(b1, m))
        bound = float(tree.query(pts[::40])[0].min())
        brute = min(bound, float(tree.query(pts, distance_upper_bound=bound * (1 + 1e-12) + 1e-300)[0].min()))
        assert exact - 1e-12 <= brute <= exact + spacing, (k, exact, brute, gap)
        n_zero += exact == 0.0
    assert 20 <= n_zero <= 180          # both branches of the distance occurred


def test_tightened_boxes_are_the_plain_ones_at_shifted_centres():
    rng = np.random.default_rng(7)
    sig = math.sqrt(obca.DELAY_PROB / (1.0 - obca.DELAY_PROB))
    worst = 0.0
    for k in range(50):
        sp = _pair(rng.uniform(0, 140), rng.uniform(-5, 5), rng.uniform(-0.5, 0.5), rng.uniform(0, 140),
                   rng.uniform(-5, 5), rng.uniform(-0.5, 0.5), v0=rng.uniform(0, 20), v1=rng.uniform(0, 20))
        shifted = sp.copy()
        for v in (0, 1):
            x, y, vel, th = sp[v, :4]
            # util.py:83-99: pos0 + delta_avg + sqrt(prob / (1 - prob)) * delta_var
            delta_avg = np.array([obca.AVG_DELAY * vel * math.cos(th), obca.AVG_DELAY * vel * math.sin(th)])
            delta_var = np.array([(obca.VAR_DELAY * vel * math.cos(th)) * (obca.VAR_DELAY * vel * math.cos(th)),
                                  (obca.VAR_DELAY * vel * math.sin(th)) * (obca.VAR_DELAY * vel * math.sin(th))])
            shifted[v, :2] = np.array([x, y]) + delta_avg + sig * delta_var
        plain, tight = obca.clearance(sp, 1)
        worst = max(worst, abs(tight - obca.clearance(shifted, 0)[0]))
        assert obca.clearance(sp, 0) == (plain, plain)          # prob = 0: the plain value twice
        # and the tightened halfspaces are those of `halfspaces`: b - b0 = A (centre + offset)
        for v in (0, 1):
            A, b = obca.halfspaces(sp[v], 1)
            cx, cy = obca.vehicle_box(sp[v], 1, True)[:2]
            assert np.abs(b - np.array([L / 2, W / 2, L / 2, W / 2]) - A @ np.array([cx, cy])).max() <= 1e-12
    assert worst <= 1e-12, worst


def test_sat_margin_of_the_gpu_cases():
    """The pairs tests/test_gpu_obca_clearance.py feeds the kernel: none stands within 1e-9 of the
    zero / non-zero decision, in either box set (the seeds were chosen so)."""
    states, prob = C.all_cases()
    assert len(states) == len(C.crafted()) + 70
    for sp, p in zip(states, prob):
        for tight in (False, True):
            gap = obca.box_clearance(obca.vehicle_box(sp[0], p, tight), obca.vehicle_box(sp[1], p, tight))[1]
            assert abs(gap) >= C.MARGIN, (sp, p, gap)
    zero = [obca.clearance(sp, p)[0] == 0.0 for sp, p in zip(states, prob)]
    assert 5 <= sum(zero) <= len(zero) - 5


def _define(src, name):
    m = re.search(rf"^#define {name} (-?\d+)\s*$", src, re.M)
    assert m, name
    return int(m.group(1))


def test_header_defines_match_python():
    src = open(HEADER).read()
    assert _define(src, "PIADMM_OBCA_TRACE_LAMBDA") == obca.TRACE_LAMBDA == 1
    codes = {name: int(v) for name, v in re.findall(r"^#define PIADMM_OBCA_TRACE_GET_(\w+) (\d+)\s*$", src, re.M)}
    assert codes == {k: v[0] for k, v in obca.TRACE_GET.items()}
    assert sorted(codes.values()) == list(range(len(codes)))
    assert set(codes) == {"STATES", "CLEARANCE", "ITERS", "STATUS_MASK", "PRIMAL", "DUAL", "LAMBDA", "SUMMARY", "ROWS"}


def test_every_new_symbol_is_declared_bound_and_exported():
    src = open(HEADER).read()
    declared = set(re.findall(r"^\s*int32_t\s+(piadmm_obca_\w+)\s*\(", src, re.M))
    bound = {n for n, _, _ in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW_SYMBOLS:
        assert name in declared and name in bound and hasattr(lib, name), name
        assert not name.startswith("piadmm_obca_plan_"), name
    assert {n for n in declared if n.startswith("piadmm_obca_trace_")} == set(NEW_SYMBOLS[1:])
    assert _lib.load().piadmm_abi_version() == 7
