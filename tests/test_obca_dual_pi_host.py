"""Host side of the PI anti-windup dual law of the OBCA-ADMM plan (piadmm.obca.lambda_update_pi,
shift_dual, OBCAPlanner(dual=...); piadmm_obca_dual_plan / piadmm_obca_dual_pi in include/piadmm.h).
No kernel runs here: the planner runs on the CPU restatement of both solves
(tests/_obca_edge_ref.OracleBatch).

Bars.  Against obca.lambda_update with kP = 0, kI = rho, windup = 0, S = lamb_bar, D = 0:
2^-52 (|rho e| + |lam'|) per entry, the rounding of one product and one sum.  Against
oracle.piadmm_oracle.dual_update (dual_mode 1, theta2 = 0, theta1 = kP, d_gain = 1), the
saturation identities, the unwritten slots and the shift: bit-equal.

The gains the GPU test runs (tests/_obca_dual_cases.py) are chosen here: the coverage counts below
are asserted so the choice cannot rot."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_dual_cases as C
import _obca_edge_ref as E
import _obca_fleet_cases as F
from oracle import piadmm_oracle as O
from piadmm import _lib, config, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
SETUP = dict(prob=[1, 0, 1], t_step0=12, max_admm_iter=2, round_decimals=-1,
             primal_thres=[0.01, 0.01, np.inf], dual_thres=[0.01, 0.01, np.inf])
MARGIN = 1e-9
EPS = 2.0 ** -52


def _bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    assert a.shape == b.shape, (msg, a.shape, b.shape)
    assert a.tobytes() == b.tobytes(), (msg, float(np.nanmax(np.abs(a - b))))


def _bars(t_step, seed):
    """The seeded bar state of MPC step t_step (consensus error 0) and one an iterate would hold:
    Z_bar off the local side, lamb_bar and the integrator random."""
    rng = np.random.default_rng(seed)
    exact = obca.seeded_bar_state(t_step, 1)
    moved = {k: v.copy() for k, v in exact.items()}
    moved["Z_bar"] = moved["Z_bar"] + 0.3 * rng.standard_normal((2, obca.NT, 9))
    moved["lamb_bar"] = 0.1 * rng.standard_normal((2, obca.NT, 9))
    return exact, moved


@pytest.mark.parametrize("t_step", [5, 12])
@pytest.mark.parametrize("rho", [1.0, 0.7, 1.5])
def test_plain_update_recovered(t_step, rho):
    for bar in _bars(t_step, 100 + t_step):
        want = obca.lambda_update(bar, rho)["lamb_bar"]
        got, S, D, dres = obca.lambda_update_pi(bar, bar["lamb_bar"].copy(), np.zeros((2, obca.NT, 9)),
                                                dict(kP=0.0, kI=rho, windup=0), [True] * obca.NT)
        e = obca.local_z(bar) - bar["Z_bar"]
        bound = EPS * (np.abs(rho * e) + np.abs(got["lamb_bar"]))
        assert np.all(np.abs(got["lamb_bar"] - want) <= bound), float(np.abs(got["lamb_bar"] - want).max())
        _bits(S, got["lamb_bar"], "kP = 0: the integrator is the dual")
        assert not D.any()
        # the slot sums: the entries' bars, and one rounding per partial sum of the 18 terms
        want_d = np.abs(want - bar["lamb_bar"]).sum(axis=(0, 2))
        assert np.all(np.abs(dres - want_d) <= bound.sum(axis=(0, 2)) + 18 * EPS * want_d)


@pytest.mark.parametrize("windup", [1, 0])
def test_against_the_oracle_dual_update(windup):
    kP, kI, sat = 0.75, 1.3, 0.2
    cfg = config.matlab_pi(H=8, dual_mode=config.DUAL_PI, theta1=kP, theta2=0.0, kI=kI, windup=windup, windup_sat=sat)
    rng = np.random.default_rng(7)
    _, bar = _bars(12, 7)
    S, D = 0.1 * rng.standard_normal((2, obca.NT, 9)), 0.05 * rng.standard_normal((2, obca.NT, 9))
    w = obca.local_z(bar)
    lam_o, S_o, D_o = bar["lamb_bar"].copy(), S.copy(), D.copy()
    O.dual_update(cfg, w[0], w[1], bar["Z_bar"].copy(), lam_o, S_o, D_o, np.array([1.0]))
    got, S1, D1, _ = obca.lambda_update_pi(bar, S, D, dict(kP=kP, kI=kI, windup_sat=sat, d_gain=1.0, windup=windup),
                                           [True] * obca.NT)
    _bits(got["lamb_bar"], lam_o, "lamb_bar")
    _bits(S1, S_o, "S")
    if windup:
        _bits(D1, D_o, "D")
        assert (np.abs(lam_o) == sat).any() and (np.abs(lam_o) < sat).any()
    else:
        assert not D1.any()          # the oracle leaves D alone without windup; the law zeroes it


def test_saturation_and_back_calculation():
    _, bar = _bars(5, 3)
    rng = np.random.default_rng(3)
    S, D = 0.1 * rng.standard_normal((2, obca.NT, 9)), 0.05 * rng.standard_normal((2, obca.NT, 9))
    g = dict(kP=0.5, kI=1.0, windup_sat=0.15, d_gain=0.5, windup=1)
    got, S1, D1, dres = obca.lambda_update_pi(bar, S, D, g, [True] * obca.NT)
    e = obca.local_z(bar) - bar["Z_bar"]
    raw = (S + g["kI"] * e + g["d_gain"] * D) + g["kP"] * e
    clipped = np.abs(raw) > g["windup_sat"]
    assert clipped.any() and (~clipped).any()
    lam = got["lamb_bar"]
    assert np.all(np.abs(lam[clipped]) == g["windup_sat"])
    _bits(D1, lam - raw, "D' = lam' - raw")
    assert np.all(D1[clipped] != 0.0) and not D1[~clipped].any()
    _bits(lam[~clipped], raw[~clipped], "unclipped entries are raw")
    _bits(S1, S + g["kI"] * e + g["d_gain"] * D, "S'")
    # the residual: each slot's 18 entries in order, vehicle 0's 9 then vehicle 1's 9
    dr = np.abs(lam - bar["lamb_bar"])
    for t in range(obca.NT):
        acc = 0.0
        for v in (0, 1):
            for li in range(9):
                acc = acc + dr[v, t, li]
        assert dres[t] == acc


def test_unwritten_slots_are_kept():
    _, bar = _bars(12, 5)
    rng = np.random.default_rng(5)
    S, D = 0.1 * rng.standard_normal((2, obca.NT, 9)), 0.05 * rng.standard_normal((2, obca.NT, 9))
    wrote = np.array([True, False, True, True, False, False, True])
    got, S1, D1, dres = obca.lambda_update_pi(bar, S, D, C.GAINS, wrote)
    full = obca.lambda_update_pi(bar, S, D, C.GAINS, [True] * obca.NT)
    for t in range(obca.NT):
        if wrote[t]:
            for a, b in zip((got["lamb_bar"], S1, D1), (full[0]["lamb_bar"], full[1], full[2])):
                _bits(a[:, t], b[:, t], f"written slot {t}")
            assert dres[t] == full[3][t] > 0.0
        else:
            _bits(got["lamb_bar"][:, t], bar["lamb_bar"][:, t], f"lamb_bar of slot {t}")
            _bits(S1[:, t], S[:, t], f"S of slot {t}")
            _bits(D1[:, t], D[:, t], f"D of slot {t}")
            assert dres[t] == 0.0
    for k in ("Z_bar", "A", "b", "lamb_ij", "local_x"):
        _bits(got[k], bar[k], k)


def test_shift_dual_is_the_state_shift():
    rng = np.random.default_rng(11)
    S, D = rng.standard_normal((2, obca.NT, 9)), rng.standard_normal((2, obca.NT, 9))
    S1, D1 = obca.shift_dual(S, D)
    for a, a1 in ((S, S1), (D, D1)):
        bar = obca.create_bar_state()
        bar["lamb_bar"] = a
        _bits(a1, obca.iterate_next_state(bar)["lamb_bar"], "shift")
    _bits(S1[:, -1], S[:, -1], "the last slot repeats")


def test_dual_rows():
    one = obca.dual_rows(3, C.GAINS)
    assert one.shape == (1, obca.DUAL_PAR) and one[0].tolist() == [0.5, 1.0, 0.05, 0.5, 1.0, 0.0, 0.0, 0.0]
    each = obca.dual_rows(4, C.FLEET_GAINS)
    assert each.shape == (4, obca.DUAL_PAR) and each[:, 1].tolist() == F.ROWS["rho"] and not each[:, 5:].any()
    mixed = obca.dual_rows(2, dict(kP=[0.1, 0.2], kI=2.0))
    assert mixed[:, 0].tolist() == [0.1, 0.2] and mixed[:, 1].tolist() == [2.0, 2.0] and not mixed[:, 2:].any()
    _bits(obca.dual_row(C.GAINS), one[0])


def _host_run(kw, gains, steps=1):
    """OBCAPlanner on the CPU restatement with the law: per iterate (scenarios, statuses, lamb_bar
    before and after, D before, residuals, stop) from the stages."""
    log, edge = [], {}
    pl = None

    def on_stage(name, inp, outp):
        if name == "edge":
            edge["status"] = outp["result"].status.copy()
            edge["D_in"] = [pl.dual_D[s].copy() for s in inp["scenarios"]]
        if name == "residual":
            log.append(dict(i_iter=inp["i_iter"], scenarios=list(inp["scenarios"]), status=edge["status"],
                            D_in=edge["D_in"], lamb=[a.copy() for a in inp["lamb_bar"]],
                            lamb_prev=[a.copy() for a in inp["lamb_bar_prev"]], primal=outp["primal"].copy(),
                            dual=outp["dual"].copy(), stop=outp["stop"].copy(), t_step=pl.t_step))

    pl = obca.OBCAPlanner(E.OracleBatch(), dual=gains, on_stage=on_stage, **kw)
    pl.run(steps)
    return pl, log


def _check_coverage(pl, log, iterates):
    near = 0
    per_iter = {}
    for it in log:
        for k, s in enumerate(it["scenarios"]):
            row = pl.dual_par[s % len(pl.dual_par)]
            c = C.coverage(it["lamb"][k], it["D_in"][k], C.wrote_of(it["status"][k]), row)
            tot = per_iter.setdefault((it["t_step"], it["i_iter"]), [0, 0, 0])
            for j in range(3):
                tot[j] += c[j]
            forced = it["i_iter"] > pl.max_admm_iter_s[s]
            if not forced and min(abs(it["primal"][k] - pl.primal_thres[s]), abs(it["dual"][k] - pl.dual_thres[s])) < MARGIN:
                near += 1
    print("coverage (clipped, unclipped, D fed back) per (t_step, iterate):", per_iter, "near a threshold:", near)
    t0 = min(t for t, _ in per_iter)
    for i in iterates:
        clipped, unclipped, fed = per_iter[(t0, i)]
        assert clipped > 0 and unclipped > 0, (i, clipped, unclipped)
        assert (fed > 0) == (i > 1), (i, fed)
    assert near == 0
    return per_iter


def test_gains_cover_both_branches_on_the_setup_plan():
    pl, log = _host_run(dict(SETUP, n_scenarios=3), C.GAINS, steps=2)
    assert C.GAINS["d_gain"] != 0.0 and C.GAINS["windup"] == 1
    _check_coverage(pl, log, (1, 2, 3))
    assert np.asarray(pl.record.iter_num_record).tolist()[0] == [3, 3, 1]


def test_gains_cover_both_branches_on_the_fleet():
    cases = [0, 1, 2, 3]
    pl, log = _host_run(F.fleet_kwargs(cases, 12), C.fleet_gains(cases), steps=1)
    _check_coverage(pl, log, (1, 2, 3))


def test_dual_none_is_the_planner_as_it_was():
    a = obca.OBCAPlanner(E.OracleBatch(), n_scenarios=3, **SETUP)
    b = obca.OBCAPlanner(E.OracleBatch(), n_scenarios=3, dual=None, **SETUP)
    ra, rb = a.run(1), b.run(1)
    for k in ("state_record", "iter_num_record", "lambda_record"):
        _bits(np.asarray(getattr(ra, k), np.float64), np.asarray(getattr(rb, k), np.float64), k)
    assert a.dual_par is None
    # and the law with kP = 0, kI = rho is the same iterates to rounding
    c = obca.OBCAPlanner(E.OracleBatch(), n_scenarios=3, dual=dict(kP=0.0, kI=1.0, windup=0), **SETUP)
    rc = c.run(1)
    assert np.asarray(rc.iter_num_record).tolist() == np.asarray(ra.iter_num_record).tolist()
    assert np.abs(np.asarray(rc.lambda_record) - np.asarray(ra.lambda_record)).max() <= 1e-9


def test_host_planner_shifts_the_integrator_before_the_stopping_iterate():
    """B16 for the integrator: what the shift takes is S, D as they stood before each scenario's
    stopping iterate, i.e. after its last continuing one."""
    hist = {}
    pl = None

    def on_stage(name, inp, outp):
        if name == "local":
            for s in inp["scenarios"]:
                hist[s] = (pl.dual_S[s].copy(), pl.dual_D[s].copy())       # before this iterate

    pl = obca.OBCAPlanner(E.OracleBatch(), n_scenarios=3, dual=C.GAINS, on_stage=on_stage, **SETUP)
    pl.step()
    for s in range(3):
        want = obca.shift_dual(*hist[s])
        _bits(pl.dual_S[s], want[0], f"S of scenario {s}")
        _bits(pl.dual_D[s], want[1], f"D of scenario {s}")
    assert hist[0][1].any()                 # a scenario that ran 3 iterates carries a non-zero D


# ---------------------------------------------------------------------------------------------
# the header and the binding
# ---------------------------------------------------------------------------------------------
NEW_SYMBOLS = {"piadmm_obca_dual_plan": 3, "piadmm_obca_dual_pi": 12}


def test_symbols_are_declared_bound_and_exported():
    src = open(HEADER).read()
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, nargs in NEW_SYMBOLS.items():
        assert re.search(rf"^\s*int32_t\s+{name}\s*\(", src, re.M), name
        assert name in bound and len(bound[name]) == nargs, name
        assert hasattr(lib, name), name
    assert _lib.load().piadmm_abi_version() == 7


def test_constants_match_the_header():
    src = open(HEADER).read()
    m = re.search(r"^#define PIADMM_OBCA_DUAL_PAR (\d+)\s*$", src, re.M)
    assert m and int(m.group(1)) == _lib.DUAL_PAR == obca.DUAL_PAR == 8
    codes = {n: int(v) for n, v in re.findall(r"^#define PIADMM_OBCA_PLAN_GET_(\w+) (\d+)\s*$", src, re.M)}
    assert (codes["DUAL_S"], codes["DUAL_D"], codes["DUAL_PAR"]) == (23, 24, 25)
    assert all(codes[k] == obca.PLAN_GET[k][0] for k in ("DUAL_S", "DUAL_D", "DUAL_PAR"))
    assert re.search(r"kP, kI, windup_sat, d_gain, windup \(0 / 1\), 0, 0, 0", src)
    assert obca.DUAL_ROW == ("kP", "kI", "windup_sat", "d_gain", "windup")


def test_entry_points_refuse_without_a_handle():
    lib = _lib.load()
    assert lib.piadmm_obca_dual_plan(None, None, 0) == _lib.E_ARG
    assert lib.piadmm_obca_dual_pi(None, 1, None, None, None, None, None, 1, None, None, None, None) == _lib.E_ARG
