"""The off-preset cases of tests/_offpreset_cases.py are sound tests before they judge a kernel
(tests/test_gpu_offpreset.py): over every case's window the oracle certifies each QP (qp_exact
raises otherwise); the independent C++ baseline (oracle/piadmm_cpu.cpp, dual modes 0 / 1) computes
the same run -- equal iteration counts, u, xt and residual histories within 1e-10, no uncertified
QP; the global PI law (dual mode 2, which the baseline does not cover) is held against the oracle
itself restarted from xt0 (1 + 1e-15), as tools/crossing_sensitivity.py does, within the same
1e-10; no discrete decision of the window falls within the near-tie logs' default tolerance 1e-9
of its threshold; and the case shows the engagement its group exists for (saturation with a
non-zero back-calculation, the three regimes of the rho clamp, a tightened distance, ...)."""
import numpy as np
import pytest

import _offpreset_cases as C
from oracle import cpu_bopt


def test_coverage_table():
    """Every field of COVERAGE is off its preset's value on every kernel that reads it (and under
    both position models / collision thresholds where the table asks): the table in the module's
    docstring, checked."""
    assert C.coverage_gaps() == []
    assert 25 <= len(C.CASES) <= 35
    assert len(set(C.IDS)) == len(C.IDS)
    for c in C.CASES:
        assert c.steps <= 26 and (c.H in (3, 33) or 8 <= c.H <= 12), c.name
        unknown = {k for k, _ in c.kw} - set(c.cfg.__dataclass_fields__)
        assert not unknown, (c.name, unknown)
    # the saturation branch runs on both kernels, and on the graph kernel's own pair loop
    sat = [c for c in C.CASES if "sat" in c.engage]
    assert any("fused" in c.kernels for c in sat) and any(c.kernels == ("graph",) for c in sat)
    assert {c.H for c in C.CASES if c.group == "S"} == {3, 33}


def test_coverage_check_sees_a_gap():
    """The coverage check is not vacuous: without the G cases the graph-only fields are gaps, and
    without the matlab_pi Q cases the second position model is."""
    gaps = dict(C.coverage_gaps([c for c in C.CASES if c.group != "G"]))
    assert {"rho_num", "rho_min", "rho_max", "d_gain", "dual_init", "ki_adapt", "pi_trad"} <= set(gaps)
    gaps = C.coverage_gaps([c for c in C.CASES if c.preset != C.MP])
    assert ("dt", "no case with pos_model 1, collide_sq_thres 1") in gaps


def _key_id(key):
    return key if isinstance(key, str) else f"{key[0]}={key[1]}"


# eps_pri and eps_dual are off their presets' values in several cases, but no value tried moved a run
# that also has a step of several iterations (the Q engagement): these loops end after two
# iterations with the edge positions unchanged and the primal residual far below either eps_pri
# (casadi_default also aliases the dual residual to 0 after the first iteration); only tolerances
# large enough to stop every loop after its first iteration change the counts.  The two fields are
# covered (off-preset on both kernels), not shown to matter.
NOT_SHOWN_TO_MATTER = {"eps_pri", "eps_dual"}


@pytest.mark.parametrize("key", [k for k in C.COVERAGE if k not in NOT_SHOWN_TO_MATTER],
                         ids=[_key_id(k) for k in C.COVERAGE if k not in NOT_SHOWN_TO_MATTER])
def test_covered_field_changes_the_compared_outputs(key):
    """A case covers a field only if the field's value reaches what the GPU tests compare: the
    first case that sets the field, re-run on the oracle with that one field back at the preset's
    value, must part from the case's own run (another iteration count, or u / xt apart by more
    than 1e-6: a hundred times the GPU bar) inside the window.  A kernel that read a stale or
    wrong value of the field would therefore fail that case."""
    field, value = key if isinstance(key, tuple) else (key, None)
    case = next(c for c in C.CASES if field in c.off_preset() and (value is None or getattr(c.cfg, field) == value))
    run = C.oracle_run(case.name)
    kw = dict(case.kw, kI=case.cfg.kI)            # explicit: matlab_pi ties kI to rho otherwise
    kw[field] = getattr(case.preset_cfg, field)
    back = C.Case(case.name, case.group, case.preset, case.H, tuple(sorted(kw.items())), case.scn, case.steps, ())
    assert back.off_preset() == case.off_preset() - {field}
    orc = C.O.Oracle(back.cfg, back.scenario())
    for ro in run.recs:
        rb = orc.mpc_step()
        if (not np.array_equal(rb.iters, ro.iters) or np.max(np.abs(rb.u - ro.u)) > 1e-6
                or np.max(np.abs(rb.xt - ro.xt)) > 1e-6):
            return
    pytest.fail(f"{case.name}: {field} at the preset's value gives the same run")


@pytest.mark.parametrize("name", C.IDS)
def test_case_is_sound(name):
    case = C.BY_NAME[name]
    cfg = case.cfg
    run = C.oracle_run(name)                      # every QP certified, or this raises
    assert run.ties == [], run.ties[:5]
    if cfg.dual_mode in (0, 1):
        scn = case.scenario()
        r = cpu_bopt.run(cfg, scn, case.steps, threads=2)
        assert r["counters"]["inexact"] == 0
        assert len(r["ties"][1]) == 0 and sum(r["ties"][0].values()) == 0, r["ties"][0]
        for k, ro in enumerate(run.recs):
            np.testing.assert_array_equal(r["iters"][k], ro.iters, err_msg=f"step {k}")
            np.testing.assert_allclose(r["u"][k], ro.u, rtol=0, atol=C.CPU_TOL, err_msg=f"u, step {k}")
            np.testing.assert_allclose(r["xt"][k], ro.xt, rtol=0, atol=C.CPU_TOL, err_msg=f"xt, step {k}")
            for c, hist in enumerate(ro.resid):
                res = np.array(hist, np.float64).reshape(-1, 2)
                mine = r["resid"][k, c]
                np.testing.assert_allclose(mine[:len(res)], res, rtol=0, atol=C.CPU_TOL, err_msg=f"resid, step {k}")
                assert np.all(np.isnan(mine[len(res):]))
    else:
        other = C.run_oracle(case, C.perturbed_scenario(case))
        assert other.ties == []
        for k, (ra, rb) in enumerate(zip(run.recs, other.recs)):
            np.testing.assert_array_equal(ra.iters, rb.iters, err_msg=f"step {k}")
            np.testing.assert_allclose(rb.u, ra.u, rtol=0, atol=C.CPU_TOL, err_msg=f"u, step {k}")
            np.testing.assert_allclose(rb.xt, ra.xt, rtol=0, atol=C.CPU_TOL, err_msg=f"xt, step {k}")
            for ha, hb in zip(ra.resid, rb.resid):
                np.testing.assert_allclose(np.array(hb), np.array(ha), rtol=0, atol=C.CPU_TOL, err_msg=f"resid, step {k}")
    m = C.engagement(case, run)
    print(name, m)
    C.check_engagement(case, m)
