"""Off-preset cases of the PI-ADMM loop shared by tests/test_offpreset_cases.py (CPU: every case is
proved a sound test -- oracle against the C++ baseline or against itself perturbed, no near tie,
the engagement its group needs) and tests/test_gpu_offpreset.py (GPU: both kernels against the
oracle on the same cases, host-stepped and in one launch).  A plain module: nothing runs on import;
oracle runs are computed on demand and cached, so the tests of one case share one run.

Groups (``Case.group``) and the engagement a case must show (``Case.engage``):

  Q  QP coefficients            "q": a pair QP ran and a step took more than one outer iteration
  D  per-edge PI (dual_mode 1)  "sat": >= 5 iterations with some |lam| == windup_sat and D != 0;
                                "nowindup": windup = 0 and |lam| beyond windup_sat
  G  global PI (dual_mode 2)    "g": a loop of >= 20 iterations and the saturation reached;
                                "clamp": rho at rho_min, at rho_max and strictly between in one run
  T  delay tightening           "t": d_eff differs from dis_thres by > 1e-3
  S  edges of size              H = 3 and H = 33 (big mode), Q + D together

Kernels: a job of disjoint pairs (v, v+1) under dual modes 0 / 1 runs on the fused kernel
(csrc/piadmm_device.hip) and, with PIADMM_GRAPH=1, on the graph kernel (csrc/piadmm_graph.hip);
chains, all-pairs crossings and the global PI law run on the graph kernel alone (``Case.kernels``).

Coverage (COVERAGE below, asserted by tests/test_offpreset_cases.py::test_coverage_table): every
field is off its preset's value in a case of every kernel that reads it, and the fields marked *
also under both position models and both collide_sq_thres settings (casadi_default: linear, d^2
against dis_thres; matlab_pi: nonlinear, d^2 against dis_thres^2).

  field                                   kernels        cases
  dt*, L*                                 fused, graph   q_dt_L_*, q_chain_cd, q_cross_mp, s_*
  Pnorm*, Pcost*, rho*                    fused, graph   q_cost_*, q_chain_cd, q_cross_mp
  beta*, dis_thres*                       fused, graph   q_beta_dis_*, q_chain_mp, q_cross_cd
  u_max*, du_max*                         fused, graph   q_box_*, q_chain_mp, q_cross_cd
  round_decimals 2*, 6*                   fused, graph   q_round2_*, q_round6_*, q_chain_mp, q_cross_cd
  eps_pri*, eps_dual*                     fused, graph   q_round2_eps_cd, q_round6_eps_mp
  kI, theta1, theta2, windup_sat, windup  fused, graph   d_*, g_*
  tight_p, avg_delay, var_delay           fused, graph   t_* (both collide_sq_thres settings)
  rho_num, rho_min, rho_max               graph          g_clamp, g_adp, g_trad
  d_gain, dual_init, ki_adapt, pi_trad    graph          g_gains_old, g_adp, g_*ki, g_trad
"""
import dataclasses
import functools

import numpy as np

from oracle import piadmm_oracle as O
from piadmm import config, scenario
from piadmm.scenario import Scenario

TOL = 1e-8          # the suite's GPU parity bar (tests/test_gpu_outer_iter.py)
CPU_TOL = 1e-10     # oracle against the C++ baseline / against itself perturbed


@dataclasses.dataclass(frozen=True)
class Case:
    name: str
    group: str          # Q, D, G, T or S
    preset: str
    H: int
    kw: tuple           # config overrides, (field, value) pairs
    scn: tuple          # ("tiled", seed) | ("intersection",) | ("crossing", seed) | ("chain", seed)
    steps: int
    engage: tuple       # engagement tags, see the module docstring

    @property
    def cfg(self):
        return config.PRESETS[self.preset](H=self.H, **dict(self.kw))

    @property
    def preset_cfg(self):
        return config.PRESETS[self.preset](H=self.H)

    def scenario(self):
        n = self.steps + 2
        kind = self.scn[0]
        if kind == "tiled":
            return scenario.tiled(2, self.H, n_steps=n, seed=self.scn[1])
        if kind == "intersection":
            return scenario.intersection(self.H, n_steps=n)
        if kind == "crossing":
            return scenario.crossing(4, self.H, n_steps=n, seed=self.scn[1])
        if kind == "chain":
            return scenario.crossing(3, self.H, n_steps=n, seed=self.scn[1], pairs="chain")
        raise ValueError(kind)

    @property
    def kernels(self):
        """The kernels the case runs on (the dispatch rule of piadmm_set_scenario)."""
        c = self.cfg
        graph_only = (self.scn[0] in ("crossing", "chain") or c.dual_mode == config.DUAL_PI_GLOBAL
                      or c.no_collision_gate or c.dual_init != 0.0)
        return ("graph",) if graph_only else ("fused", "graph")

    def off_preset(self):
        """Fields whose value differs from the preset's."""
        c, p = self.cfg, self.preset_cfg
        return {f for f in config.PIADMMConfig.__dataclass_fields__ if getattr(c, f) != getattr(p, f)}


def _c(name, group, preset, H, scn, steps, engage, **kw):
    return Case(name, group, preset, H, tuple(sorted(kw.items())), tuple(scn), steps, tuple(engage))


CD, MP, OLD, ADP = "casadi_default", "matlab_pi", "casadi_old_pi", "matlab_adp_pi"
TILES = ("tiled", 5)

CASES = [
    # ---- Q: QP coefficients, each bundle under casadi_default and matlab_pi.  beta is small: the
    # hinge is an exact penalty, so any beta above the hinge rows' multipliers gives the same answer
    _c("q_dt_L_cd", "Q", CD, 8, TILES, 26, ["q"], dt=0.08, L=2.5, max_outer=30),
    _c("q_dt_L_mp", "Q", MP, 8, TILES, 26, ["q"], dt=0.08, L=2.5, max_outer=30),
    _c("q_cost_cd", "Q", CD, 8, TILES, 24, ["q"], Pnorm=1.5, Pcost=3.0, rho=1.2, max_outer=30),
    _c("q_cost_mp", "Q", MP, 8, TILES, 24, ["q"], Pnorm=2.5, Pcost=3.0, rho=1.2, max_outer=30),
    _c("q_beta_dis_cd", "Q", CD, 8, TILES, 24, ["q"], beta=1.0, dis_thres=3.0, max_outer=30),
    _c("q_beta_dis_mp", "Q", MP, 8, TILES, 24, ["q"], beta=1.0, dis_thres=3.0, max_outer=30),
    _c("q_box_cd", "Q", CD, 8, TILES, 24, ["q"], u_max=0.3, du_max=0.2, max_outer=30),
    _c("q_box_mp", "Q", MP, 8, TILES, 24, ["q"], u_max=0.3, du_max=0.2, max_outer=30),
    _c("q_round2_eps_cd", "Q", CD, 8, TILES, 24, ["q"], round_decimals=2, eps_pri=0.5, eps_dual=0.02, max_outer=30),
    _c("q_round2_mp", "Q", MP, 8, TILES, 24, ["q"], round_decimals=2, max_outer=30),
    # 6 decimals: one value in 500 lies within 1e-9 of a rounding boundary, so the windows are
    # short and the seeds are those whose window holds no such value
    _c("q_round6_cd", "Q", CD, 8, ("tiled", 3), 20, ["q"], round_decimals=6, max_outer=30),
    _c("q_round6_eps_mp", "Q", MP, 8, ("tiled", 6), 20, ["q"], round_decimals=6, eps_pri=0.5, eps_dual=0.02,
       max_outer=30),
    # agents in two or three pairs: the x-step's sum over neighbours, several pair QPs per agent
    _c("q_chain_cd", "Q", CD, 8, ("chain", 3), 24, ["q"], dt=0.08, L=2.5, Pnorm=1.5, Pcost=3.0, rho=1.2,
       eps_pri=5.0, max_outer=30),
    _c("q_chain_mp", "Q", MP, 8, ("chain", 3), 20, ["q"], beta=5.0, dis_thres=3.0, u_max=0.3, du_max=0.2,
       round_decimals=2, max_outer=20),
    _c("q_cross_mp", "Q", MP, 8, ("crossing", 1), 22, ["q"], dt=0.08, L=2.5, Pnorm=2.5, Pcost=3.0, rho=1.2,
       eps_pri=0.5, max_outer=20),
    _c("q_cross_cd", "Q", CD, 8, ("crossing", 2), 18, ["q"], beta=1.0, dis_thres=3.0, u_max=0.3, du_max=0.2,
       round_decimals=6, max_outer=20),
    # ---- D: the per-edge PI law
    _c("d_sat", "D", MP, 8, TILES, 24, ["sat"], windup_sat=4.0, max_outer=30),
    _c("d_sat_theta", "D", MP, 8, TILES, 24, ["sat"], theta1=4.0, theta2=1.5, windup_sat=4.0, max_outer=30),
    _c("d_kI", "D", MP, 8, TILES, 24, ["sat"], kI=0.7, windup_sat=6.0, max_outer=30),
    _c("d_nowindup", "D", MP, 8, TILES, 24, ["nowindup"], windup=0, theta1=8.0, max_outer=30),
    _c("d_sat_warm", "D", MP, 8, TILES, 24, ["sat"], windup_sat=4.0, warm_duals=1, max_outer=30),
    _c("d_sat_cross", "D", MP, 8, ("crossing", 1), 22, ["sat"], windup_sat=4.0, theta1=4.0, theta2=1.5, kI=2.0,
       max_outer=20),
    _c("d_sat_cross_warm", "D", MP, 8, ("crossing", 1), 22, ["sat"], windup_sat=4.0, warm_duals=1, max_outer=20),
    # ---- G: the global PI law (graph kernel), H = 10 as in the preset tests
    _c("g_clamp", "G", OLD, 10, ("intersection",), 16, ["g", "clamp"], rho_num=6.0, rho_min=0.8, rho_max=2.5,
       max_outer=30),
    _c("g_gains_old", "G", OLD, 10, ("intersection",), 14, ["g"], theta1=4.0, theta2=1.5, kI=2.0, windup_sat=8.0,
       d_gain=1.5, max_outer=30),
    _c("g_adp", "G", ADP, 10, ("intersection",), 16, ["g", "clamp"], theta1=4.0, theta2=2.0, kI=2.0, windup_sat=12.0,
       d_gain=0.5, dual_init=1e-3, rho_num=3.0, max_outer=30),
    _c("g_adp_fixedki", "G", ADP, 10, ("intersection",), 16, ["g"], ki_adapt=0, kI=1.5, windup_sat=12.0,
       max_outer=30),
    _c("g_old_adaptki", "G", OLD, 10, ("intersection",), 14, ["g"], ki_adapt=1, windup_sat=8.0, dual_init=1e-3,
       max_outer=30),
    _c("g_trad", "G", OLD, 10, ("intersection",), 14, ["g", "clamp"], pi_trad=1, windup_sat=8.0, rho_num=6.0,
       rho_max=3.0, max_outer=30),
    # ---- T: delay tightening
    _c("t_cd", "T", CD, 8, TILES, 24, ["t"], tighten=1, tight_p=0.8, avg_delay=0.08, var_delay=0.04, max_outer=30),
    _c("t_mp", "T", MP, 8, TILES, 24, ["t"], tighten=1, tight_p=0.8, avg_delay=0.08, var_delay=0.04, max_outer=30),
    _c("t_chain_cd", "T", CD, 8, ("chain", 3), 24, ["t"], tighten=1, tight_p=0.9, avg_delay=0.1, var_delay=0.05,
       max_outer=30),
    _c("t_cross_mp", "T", MP, 8, ("crossing", 1), 22, ["t"], tighten=1, tight_p=0.8, avg_delay=0.08, var_delay=0.04,
       max_outer=20),
    # ---- S: edges of size (Q + D)
    _c("s_H3", "S", MP, 3, TILES, 26, ["q", "sat"], windup_sat=4.0, dt=0.12, Pnorm=2.5, max_outer=30),
    _c("s_H33", "S", MP, 33, TILES, 3, ["q", "sat"], windup_sat=4.0, dt=0.08, Pnorm=2.5, max_outer=12),
]
BY_NAME = {c.name: c for c in CASES}
IDS = [c.name for c in CASES]
GPU_PARAMS = [(c, k) for c in CASES for k in c.kernels]
GPU_IDS = [f"{c.name}-{k}" for c, k in GPU_PARAMS]

BOTH, GRAPH = ("fused", "graph"), ("graph",)
# field (or (field, value)) -> (kernels that must see it off-preset, also under both models?)
COVERAGE = {
    "dt": (BOTH, True), "L": (BOTH, True), "Pnorm": (BOTH, True), "Pcost": (BOTH, True), "rho": (BOTH, True),
    "beta": (BOTH, True), "u_max": (BOTH, True), "du_max": (BOTH, True), "dis_thres": (BOTH, True),
    ("round_decimals", 2): (BOTH, True), ("round_decimals", 6): (BOTH, True),
    "eps_pri": (BOTH, True), "eps_dual": (BOTH, True),
    "kI": (BOTH, False), "theta1": (BOTH, False), "theta2": (BOTH, False), "windup_sat": (BOTH, False),
    "windup": (BOTH, False),
    "tight_p": (BOTH, True), "avg_delay": (BOTH, True), "var_delay": (BOTH, True),
    "rho_num": (GRAPH, False), "rho_min": (GRAPH, False), "rho_max": (GRAPH, False), "d_gain": (GRAPH, False),
    "dual_init": (GRAPH, False), "ki_adapt": (GRAPH, False), "pi_trad": (GRAPH, False),
}


def coverage_gaps(cases=None):
    """COVERAGE entries the cases do not meet: [(field, what is missing)]."""
    cases = CASES if cases is None else cases
    gaps = []
    for key, (kernels, both_models) in COVERAGE.items():
        field, value = key if isinstance(key, tuple) else (key, None)
        hit = [c for c in cases if field in c.off_preset() and (value is None or getattr(c.cfg, field) == value)]
        for k in kernels:
            if not any(k in c.kernels for c in hit):
                gaps.append((key, f"no {k}-kernel case"))
        if both_models:
            for pm, cs in ((0, 0), (1, 1)):
                if not any(c.cfg.pos_model == pm and c.cfg.collide_sq_thres == cs for c in hit):
                    gaps.append((key, f"no case with pos_model {pm}, collide_sq_thres {cs}"))
    return gaps


# ----------------------------------------------------------------------------- oracle runs
@dataclasses.dataclass
class OracleRun:
    recs: list          # StepRecord per MPC step
    states: list        # per step: the on_iter states (with rho_pi added) of every outer iteration
    rho_pi: list        # per step: the pair penalties after the step
    d_eff: list         # per step: the pairs' safety distances
    ties: list          # near-tie events at the log's default tolerance


def run_oracle(case, scn=None):
    cfg = case.cfg
    scn = case.scenario() if scn is None else scn
    orc = O.Oracle(cfg, scn)
    out = OracleRun([], [], [], [], orc.ties.events)
    for _ in range(case.steps):
        out.d_eff.append(np.array([O.safety_distance(cfg, orc.xt, scn.spd, int(a), int(b)) for a, b in scn.edges]))
        sts = []
        out.recs.append(orc.mpc_step(on_iter=lambda it, st: sts.append(dict(st, rho_pi=orc.rho_pi.copy()))))
        out.states.append(sts)
        out.rho_pi.append(orc.rho_pi.copy())
    return out


@functools.lru_cache(maxsize=None)
def oracle_run(name):
    """The oracle over the case's window (every QP certified, or qp_exact raises); cached, and
    shared by every test of the case: leave it unchanged."""
    return run_oracle(BY_NAME[name])


def perturbed_scenario(case, eps=1e-15):
    s = case.scenario()
    return Scenario(spd=s.spd, xt0=s.xt0 * (1.0 + eps), ref=s.ref, edges=s.edges, n_steps=s.n_steps)


def engagement(case, run):
    """The counts the engagement assertions are made of."""
    cfg = case.cfg
    W = cfg.windup_sat
    m = dict(z_steps=0, multi_steps=0, max_iters=0, sat_iters=0, max_D=0.0, max_lam=0.0, rho_regimes=set(),
             d_eff_gap=0.0)
    for rec, sts, d_eff in zip(run.recs, run.states, run.d_eff):
        m["z_steps"] += any(len(r) for r in rec.resid)      # a residual is recorded once a pair QP ran
        m["multi_steps"] += int(rec.iters.max() > 1)
        m["max_iters"] = max(m["max_iters"], int(rec.iters.max()))
        if d_eff.size:
            m["d_eff_gap"] = max(m["d_eff_gap"], float(np.max(np.abs(d_eff - cfg.dis_thres))))
        for st in sts:
            sat = bool(np.any(np.abs(st["lam"]) == W))
            m["sat_iters"] += sat and bool(np.any(st["D"] != 0.0))
            m["max_D"] = max(m["max_D"], float(np.max(np.abs(st["D"]))))
            m["max_lam"] = max(m["max_lam"], float(np.max(np.abs(st["lam"]))))
            for r in st["rho_pi"]:
                m["rho_regimes"].add("min" if r == cfg.rho_min else "max" if r == cfg.rho_max else "interior")
    return m


def check_engagement(case, m):
    cfg = case.cfg
    for tag in case.engage:
        if tag == "q":
            assert m["z_steps"] >= 1 and m["multi_steps"] >= 1, m
        elif tag == "sat":
            assert cfg.windup == 1 and m["sat_iters"] >= 5 and m["max_D"] > 0.0, m
        elif tag == "nowindup":
            assert cfg.windup == 0 and m["max_lam"] > cfg.windup_sat and m["max_D"] == 0.0, m
        elif tag == "g":
            assert m["max_iters"] >= 20 and m["sat_iters"] >= 1, m
        elif tag == "clamp":
            assert m["rho_regimes"] == {"min", "max", "interior"}, m
        elif tag == "t":
            assert cfg.tighten == 1 and m["d_eff_gap"] > 1e-3, m
        else:
            raise ValueError(tag)


# ----------------------------------------------------------------------------- GPU host stepping
def close(a, b, what, it, scale=1.0):
    np.testing.assert_allclose(a, b, rtol=TOL, atol=TOL * scale, err_msg=f"{what} after outer iteration {it}")


def excess(a, b, scale=1.0, rtol=TOL, atol=TOL):
    """max |a - b| / (atol scale + rtol |b|): <= 1 where assert_allclose passes."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    if a.size == 0:
        return 0.0
    return float(np.max(np.abs(a - b) / (atol * scale + rtol * np.abs(b))))


def check_iterations(s, t, states, rec, check_sd=True):
    """Host-step MPC step t on the GPU (piadmm_outer_iter / piadmm_step_finish) against the oracle's
    states of the same step: pos_old, hat, lam, S, D after every outer iteration at TOL, the stop
    flag at the same iteration, xt and u after the propagation.  Returns the worst deviation in
    units of the tolerance (see :func:`excess`)."""
    worst = 0.0
    for it, ost in enumerate(states):
        stop = s.outer_iter(it, t)
        g = s.state()
        close(g["pos_old"], ost["pos_old"], "pos_old", it)
        close(g["hat"], ost["hat"], "hat", it)
        close(g["lam"], ost["lam"], "lam", it)
        worst = max(worst, excess(g["pos_old"], ost["pos_old"]), excess(g["hat"], ost["hat"]),
                    excess(g["lam"], ost["lam"]))
        if check_sd:
            close(g["S"], ost["S"], "S", it)
            # D = lam_sat - lam_raw with lam_raw = S + K_P e: a difference of O(|S|) quantities, so
            # its absolute error scales with |S| (the integral grows over the step's iterations)
            sc = max(1.0, float(np.max(np.abs(ost["S"])))) if ost["S"].size else 1.0
            close(g["D"], ost["D"], "D", it, scale=sc)
            worst = max(worst, excess(g["S"], ost["S"]), excess(g["D"], ost["D"], sc))
        assert stop == ost["stop"], f"stop flag at outer iteration {it}"
    xt, u = s.step_finish()
    np.testing.assert_allclose(xt, rec.xt, rtol=TOL, atol=TOL)
    np.testing.assert_allclose(u, rec.u, rtol=TOL, atol=TOL)
    return max(worst, excess(xt, rec.xt), excess(u, rec.u))


def step_by_iterations(s, orc, t, check_sd=True):
    """Host-step MPC step t on the GPU and compare every iteration with the oracle's."""
    states = []
    rec = orc.mpc_step(on_iter=lambda it, st: states.append(st))
    check_iterations(s, t, states, rec, check_sd)
    return len(states), rec
