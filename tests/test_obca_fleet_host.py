"""Host side of the per-scenario OBCA planner: `OvertakeSpec` through the scenario helpers, the
piadmm_obca_fleet_begin binding and its constants, and OBCAPlanner's per-scenario arguments on
the CPU (the two launches answered by the restatements, tests/_obca_edge_ref.OracleBatch).  No
kernel runs here."""
import ctypes
import os
import re

import numpy as np
import pytest
from conftest import ROOT

import _obca_edge_ref as E
import _obca_fleet_cases as F
from piadmm import _lib, obca

HEADER = os.path.join(ROOT, "include", "piadmm.h")
GOLDEN = os.path.join(ROOT, "tests", "golden", "ref_obca.npz")


def _bits(a, b, msg=""):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (msg, a.shape, b.shape, a.dtype, b.dtype)
    assert a.tobytes() == b.tobytes(), msg


# ---------------------------------------------------------------------------------------------
# spec=None and OvertakeSpec() are today's helpers: the expressions below are the ones the
# helpers held before they took a spec (20 m/s against 10 m/s, a 20 m gap, a 4 m lane change)
# ---------------------------------------------------------------------------------------------
def _ref_traj_gen_fixed():
    n = int(obca.T_PERIOD / obca.DT) + 1
    out = []
    for v, x0 in ((20.0, 0.0), (10.0, 20.0)):
        x = np.linspace(x0, x0 + v * obca.T_PERIOD, n)
        out.append(np.vstack((x, np.zeros_like(x), v * np.ones_like(x), np.zeros_like(x), np.zeros_like(x))).T)
    return out


def _executed_path_fixed(veh, tau):
    import math
    if veh == 1:
        return np.array([20.0 + 10.0 * tau, 0.0, 10.0, 0.0, 0.0])
    lane = 4.0

    def sstep(u):
        u = min(max(u, 0.0), 1.0)
        return u * u * (3 - 2 * u), 6 * u * (1 - u)

    a, da = sstep((tau - 0.2) / 0.6)
    b, db = sstep((tau - 3.0) / 0.6)
    y = lane * (a - b)
    dy = lane * (da - db) / 0.6
    return np.array([20.0 * tau, y, 20.0, math.atan2(dy, 20.0), 0.0])


@pytest.mark.parametrize("spec", [None, obca.OvertakeSpec(), obca.OvertakeSpec(20, 10, 20, 4)],
                         ids=["none", "default", "ints"])
def test_default_spec_is_todays_scenario_bit_for_bit(spec):
    g = np.load(GOLDEN, allow_pickle=False)
    refs = obca.ref_traj_gen(spec)
    for v in (0, 1):
        np.testing.assert_array_equal(refs[v], g[f"ref{v}"])         # as tests/test_obca_oracle.py compares
        _bits(refs[v], _ref_traj_gen_fixed()[v], "ref_traj_gen")
    for k in range(0, 101):
        for v in (0, 1):
            _bits(obca.executed_path(v, k * 0.05, spec), _executed_path_fixed(v, k * 0.05), f"executed_path {v} {k}")
    for t_step, prob in ((0, 1), (5, 0), (12, 1), (30, 0)):
        a, b = obca.seeded_bar_state(t_step, prob, spec=spec), obca.seeded_bar_state(t_step, prob)
        for key in a:
            _bits(a[key], b[key], key)
        # and the seeded arrays are what executed_path gives
        for t in range(obca.NT):
            for v in (0, 1):
                _bits(a["local_x"][v, t], _executed_path_fixed(v, (t_step + t + 1) * obca.DT), "local_x")


def test_a_spec_moves_the_scenario():
    sp = obca.OvertakeSpec(v0=18, v1=12, gap=15, lane=3.5)
    refs = obca.ref_traj_gen(sp)
    assert refs[0][0].tolist() == [0.0, 0.0, 18.0, 0.0, 0.0] and refs[1][0].tolist() == [15.0, 0.0, 12.0, 0.0, 0.0]
    assert refs[0].shape == (51, 5) and abs(refs[1][-1, 0] - (15.0 + 12.0 * 5.0)) < 1e-12
    assert obca.executed_path(1, 1.0, sp).tolist() == [27.0, 0.0, 12.0, 0.0, 0.0]
    mid = obca.executed_path(0, 2.0, sp)
    assert mid[1] == 3.5 and mid[2] == 18.0 and mid[0] == 36.0
    assert hash(sp) == hash(obca.OvertakeSpec(18.0, 12.0, 15.0, 3.5))


def test_seeded_states_of_every_spec_are_consistent():
    """seeded_bar_state's promise for any spec: A_0' lamb_0 + A_1' lamb_1 = 0 to rounding (the
    equality check_converge evaluates), Z_bar = [local_x, lamb_ij] (g_eq(w) = 0 at the seed)."""
    specs = F.SPECS + obca.overtaking_fleet(6, seed=3)[0]
    for sp in specs:
        for t_step in F.T_STEPS:
            for prob in (0, 1):
                bar = obca.seeded_bar_state(t_step, prob, spec=sp)
                eq = (np.einsum("tij,ti->tj", bar["A"][0], bar["lamb_ij"][0])
                      + np.einsum("tij,ti->tj", bar["A"][1], bar["lamb_ij"][1]))
                assert np.abs(eq).max() <= 1e-15 * 8, (sp, t_step, prob, np.abs(eq).max())
                _bits(bar["Z_bar"], obca.local_z(bar), "Z_bar")
                assert np.all(bar["lamb_ij"] >= 0)
                # the thresholds of check_converge only: the equality part holds at any threshold
                assert obca.check_converge(bar, 1e-14, -np.inf)
                for v in (0, 1):
                    _bits(bar["local_x"][v, 0], obca.executed_path(v, (t_step + 1) * obca.DT, sp), "local_x")


def test_overtaking_fleet_draws_from_the_stated_ranges():
    specs, par = obca.overtaking_fleet(500, seed=1)
    assert len(specs) == 500 and set(par) == {"rho", "min_dis"}
    for name, lo, hi in (("v0", 16, 20), ("v1", 8, 12), ("gap", 12, 20), ("lane", 3, 4)):
        v = np.array([getattr(s, name) for s in specs])
        assert v.min() >= lo and v.max() <= hi and v.max() - v.min() > 0.9 * (hi - lo), name
    assert par["rho"].shape == (500,) and 0.5 <= par["rho"].min() and par["rho"].max() <= 2.0
    assert 0.05 <= par["min_dis"].min() and par["min_dis"].max() <= 0.3
    again = obca.overtaking_fleet(500, seed=1)
    assert again[0] == specs and np.array_equal(again[1]["rho"], par["rho"])
    assert obca.overtaking_fleet(500, seed=2)[0] != specs


# ---------------------------------------------------------------------------------------------
# the binding
# ---------------------------------------------------------------------------------------------
def test_fleet_symbol_is_declared_bound_and_exported():
    name = "piadmm_obca_fleet_begin"
    assert not name.startswith("piadmm_obca_plan_")
    src = open(HEADER).read()
    assert re.search(rf"^\s*int32_t\s+{name}\s*\(", src, re.M)
    bound = {n: a for n, _, a in _lib.SYMBOLS}
    assert name in bound and len(bound[name]) == 8
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name)
    assert _lib.load().piadmm_abi_version() == 7


def test_fleet_constants_match_the_header():
    src = open(HEADER).read()
    m = re.search(r"^#define PIADMM_OBCA_FLEET_PAR (\d+)\s*$", src, re.M)
    assert m and int(m.group(1)) == _lib.FLEET_PAR == obca.FLEET_PAR == 16
    assert len(obca.FLEET_ROW) == 14 <= obca.FLEET_PAR
    codes = {n: int(v) for n, v in re.findall(r"^#define PIADMM_OBCA_PLAN_GET_(\w+) (\d+)\s*$", src, re.M)}
    assert codes["REF"] == obca.PLAN_GET["REF"][0] == 21 and codes["PAR"] == obca.PLAN_GET["PAR"][0] == 22
    # the row order the header states is the order the planner packs
    row = re.search(r"rho, min_dis, conv_thres, max_x, max_y, r, q, x_bound, mu_max, g_max,\s*\*?\s*"
                    r"max_admm_iter, max_sqp_iter, round_decimals, start, 0, 0", src)
    assert row
    assert [n.replace("max_iter", "max_sqp_iter") for n in obca.FLEET_ROW] == \
        ["rho", "min_dis", "conv_thres", "max_x", "max_y", "r", "q", "x_bound", "mu_max", "g_max", "max_admm_iter",
         "max_sqp_iter", "round_decimals", "start"]


def test_fleet_begin_refuses_without_a_handle():
    lib = _lib.load()
    assert lib.piadmm_obca_fleet_begin(None, None, None, None, None, None, None, None) == _lib.E_ARG


# ---------------------------------------------------------------------------------------------
# OBCAPlanner with one row per scenario = the scenarios one by one
# ---------------------------------------------------------------------------------------------
def _run(kw, steps=2):
    stages = []
    pl = obca.OBCAPlanner(E.OracleBatch(), on_stage=lambda name, inp, outp: stages.append((name, inp, outp)), **kw)
    return pl, stages, pl.run(steps)


def _bar_bits(a, b, msg):
    assert set(a) == set(b)
    for key in a:
        _bits(a[key], b[key], f"{msg} {key}")


@pytest.mark.parametrize("t_step0", F.T_STEPS)
def test_a_fleet_equals_its_scenarios_one_by_one(t_step0):
    pl, stages, rec = _run(F.fleet_kwargs(range(4), t_step0))
    # no row is excused: every solve of the run converged
    for st in rec.status_record:
        assert not st["local_status"].any() and not st["edge_status"].any(), st
    # each row stops by its own rule
    assert np.asarray(rec.iter_num_record).tolist() == [F.STOP_ITERS, F.STOP_ITERS]
    assert pl.rho is None and pl.rho_s.tolist() == F.ROWS["rho"] and pl.max_admm_iter_s.tolist() == F.ROWS["max_admm_iter"]
    assert pl.ref_traj is None and pl.ref_traj_s.shape == (4, 2, 51, 5)
    for c in range(4):
        one, ostages, orec = _run(F.single_kwargs(c, t_step0))
        assert one.rho == F.ROWS["rho"][c] and one.rho_s.tolist() == [F.ROWS["rho"][c]]
        _bits(one.ref_traj_s[0], pl.ref_traj_s[c], "reference")
        _bits(np.asarray(orec.state_record)[:, 0], np.asarray(rec.state_record)[:, c], "state_record")
        _bits(np.asarray(orec.iter_num_record)[:, 0], np.asarray(rec.iter_num_record)[:, c], "iter_num_record")
        _bits(np.asarray(orec.lambda_record)[:, 0], np.asarray(rec.lambda_record)[:, c], "lambda_record")
        # every stage the scenario took part in, in order
        mine = []
        for name, inp, outp in stages:
            if name == "shift":
                mine.append((name, None))
            elif name in ("local", "exchange", "edge", "residual"):
                scen = list(inp["scenarios"])
                mine.append((name, scen.index(c) if c in scen else None))
                last = mine[-1][1]
            else:                                                   # "converge" follows its "exchange"
                mine.append((name, last))
        picked = [(name, k, inp, outp) for (name, k), (_, inp, outp) in zip(mine, stages) if name == "shift" or k is not None]
        assert [p[0] for p in picked] == [s[0] for s in ostages]
        for (name, k, inp, outp), (_, oinp, ooutp) in zip(picked, ostages):
            if name == "local":
                _bits(inp["recs"][2 * k:2 * k + 2], oinp["recs"], "local records")
                _bits(outp["result"].raw[2 * k:2 * k + 2], ooutp["result"].raw, "local outputs")
                assert inp["i_iter"] == oinp["i_iter"] and inp["t_step"] == oinp["t_step"]
            elif name == "exchange":
                _bar_bits(outp["bar"][k], ooutp["bar"][0], "exchange")
            elif name == "converge":
                assert outp["if_converge"][k] == ooutp["if_converge"][0]
            elif name == "edge":
                _bits(inp["recs"][k], oinp["recs"][0], "edge record")
                _bits(outp["result"].raw[k], ooutp["result"].raw[0], "edge output")
            elif name == "residual":
                _bits(outp["primal"][k], ooutp["primal"][0], "primal")
                _bits(outp["dual"][k], ooutp["dual"][0], "dual")
                assert bool(outp["stop"][k]) == bool(ooutp["stop"][0])
            else:
                _bar_bits(inp["bar_prev"][c], oinp["bar_prev"][0], "shift in")
                _bar_bits(outp["bar_next"][c], ooutp["bar_next"][0], "shift out")
                _bits(outp["init_state"][c], ooutp["init_state"][0], "init_state")


def test_the_records_carry_the_scenarios_own_row():
    pl, stages, _ = _run(F.fleet_kwargs(range(4), 5), steps=1)
    recs = [s for s in stages if s[0] == "local"][0][1]["recs"]
    erecs = [s for s in stages if s[0] == "edge"][0][1]["recs"]
    for c in range(4):
        ref = np.stack(obca.ref_traj_gen(F.SPECS[c]))
        for v in (0, 1):
            d = obca.unpack(recs[2 * c + v])
            _bits(d["ref"], ref[v, 5:13], "reference window")
            _bits(d["init"], obca.executed_path(v, 0.5, F.SPECS[c]), "init")
            assert (d["rho"], d["min_dis"], d["max_x"], d["r"], d["q"], d["prob"]) == tuple(
                F.ROWS[k][c] for k in ("rho", "min_dis", "max_x", "r", "q", "prob"))
        e = obca.edge_unpack(erecs[c])
        assert (e["rho"], e["min_dis"], e["x_bound"], e["round_decimals"], e["prob"]) == tuple(
            F.ROWS[k][c] for k in ("rho", "min_dis", "x_bound", "round_decimals", "prob"))


def test_scalar_arguments_keep_todays_planner():
    """No spec, scalars only: the attributes and the first records are what they were."""
    pl = obca.OBCAPlanner(E.OracleBatch(), n_scenarios=2, prob=[1, 0], t_step0=12)
    assert (pl.rho, pl.min_dis, pl.max_admm_iter, pl.conv_thres, pl.round_decimals, pl.start, pl.max_iter) == \
        (1.0, 0.1, 50, 0.1, 4, 1, 60)
    assert pl.specs is None and len(pl.ref_traj) == 2 and pl.n_ref == 51
    for v in (0, 1):
        _bits(pl.ref_traj[v], _ref_traj_gen_fixed()[v], "ref_traj")
    for s, p in enumerate((1, 0)):
        _bar_bits(pl.bar_prev[s], obca.seeded_bar_state(12, p), "seed")
    assert pl.x_bound_s.tolist() == [1000.0, 1000.0] and pl.max_iter_s.tolist() == [60, 60]
