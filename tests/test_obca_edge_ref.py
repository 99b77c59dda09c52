"""The case sets of the OBCA-ADMM edge step (tests/_obca_edge_ref.py) are sound: each covers
what it is named for, the restatement converges on them and its converged answers are KKT points
of the slot NLP by the independent certificate `kkt_residual_edge`; and the host forms of
piadmm.obca (lambda_update, check_converge, seeded_bar_state, edge_record) against the
reference's lines.  No GPU.
"""
import numpy as np
import pytest

import _obca_edge_ref as E
from piadmm import obca


def _slots(name):
    return [(k, t, p, r) for k, rec in enumerate(E.case_set(name)) for t, (p, r) in enumerate(E.solve_record(rec))]


@pytest.mark.parametrize("name", E.CERTIFIED)
def test_certified_sets_converge_to_kkt_points(name):
    slots = _slots(name)
    conv = [s for s in slots if s[3].status == E.CONVERGED]
    assert len(conv) >= 0.9 * len(slots)
    for k, t, p, r in conv:
        kk = E.kkt_residual_edge(p, r.z, r.y_eq, r.y_in, r.y_bnd)
        assert kk["stat"] <= 1e-9 * kk["gscale"], (name, k, t, kk)
        assert kk["feas"] <= 1e-8 and kk["comp"] <= 1e-8, (name, k, t, kk)


def test_consistent_equals_the_closed_form():
    for k, t, p, r in _slots("consistent"):
        assert r.status == E.CONVERGED
        want = np.minimum(np.maximum(p.w + p.lb / p.rho, p.lo), p.hi)
        np.testing.assert_allclose(r.z, want, rtol=0, atol=1e-9)


def test_exchanged_gives_the_equality_work():
    n = sum(np.linalg.norm(E.constraints(p.w, p.prob)[0]) > 1e-3 for _, _, p, _ in _slots("exchanged"))
    assert n >= 10


def test_pressed_activates_the_range_row():
    hit = [(p, r) for _, _, p, r in _slots("pressed") if E.constraints(p.w, p.prob)[2] < p.min_dis]
    assert len(hit) >= 5
    assert all(r.y_in > 1e-6 for _, r in hit)


def test_bounds_activates_bound_rows():
    n = sum(bool(np.any(np.abs(r.y_bnd) > 0)) for _, _, _, r in _slots("bounds"))
    assert n >= 5


def test_truncated_stops_at_max_iter():
    slots = _slots("truncated")
    assert {p.max_iter for _, _, p, _ in slots} == {1, 2}
    assert sum(r.status == E.MAX_ITER and r.iters == p.max_iter for _, _, p, r in slots) >= 5


def test_zero_start_is_reported():
    slots = _slots("zero_start")
    assert all(p.start == 0 for _, _, p, _ in slots)
    assert any(r.status != E.CONVERGED for _, _, _, r in slots)


def test_analytic_derivatives_equal_the_complex_step():
    rng = np.random.default_rng(0)
    for prob in (1, 0):
        z = np.concatenate([[3.0, 1.0, 12.0, 0.3, 0.1], rng.uniform(0, 1, 4), [9.0, -2.0, 8.0, -0.2, 0.0], rng.uniform(0, 1, 4)])
        g_eq, Jeq, g_in, gin, Heq, Hin = E.constraints(z, prob, hess=True)
        J = np.zeros((3, 18))
        for j in range(18):
            zc = z.astype(complex)
            zc[j] += 1e-30j
            J[:, j] = E._g_c(zc, prob).imag / 1e-30
        np.testing.assert_allclose(np.vstack([Jeq, gin]), J, rtol=1e-12, atol=1e-12)
        np.testing.assert_allclose(np.concatenate([g_eq, [g_in]]), E._g_c(z.astype(complex), prob).real, rtol=1e-12, atol=1e-12)
        # Hessians: central differences of the analytic gradients
        h = 1e-6
        for j in range(18):
            zp, zm = z.copy(), z.copy()
            zp[j] += h
            zm[j] -= h
            a, b = E.constraints(zp, prob), E.constraints(zm, prob)
            np.testing.assert_allclose(Hin[j], (a[3] - b[3]) / (2 * h), rtol=0, atol=1e-6)
            np.testing.assert_allclose(Heq[:, j], (a[1] - b[1]) / (2 * h), rtol=0, atol=1e-6)


def test_host_forms():
    bar = obca.seeded_bar_state(8, prob=1)
    # seeded state: the coupled equality holds and the boxes are apart (check_converge, :225-235)
    assert obca.check_converge(bar, 0.1, 0.1)
    far = {k: v.copy() for k, v in bar.items()}
    far["lamb_ij"][0] *= 2.0
    assert not obca.check_converge(far, 0.1, 0.1)
    # lambda_update (:330-335)
    bar["Z_bar"] = obca.local_z(bar) - 0.25
    out = obca.lambda_update(bar, 2.0)
    np.testing.assert_allclose(out["lamb_bar"], bar["lamb_bar"] + 0.5)
    # edge_record round trip and the defaults of :282-295
    d = obca.edge_unpack(obca.edge_record(bar, prob=0))
    np.testing.assert_array_equal(d["local_x"], bar["local_x"])
    np.testing.assert_array_equal(d["lamb_ij"], bar["lamb_ij"])
    np.testing.assert_array_equal(d["lamb_bar"], bar["lamb_bar"])
    assert (d["prob"], d["round_decimals"], d["start"], d["x_bound"], d["mu_max"], d["g_max"]) == (0, 4, 1, 1000.0, 1e5, 1000.0)
    assert obca.EDGE_REC >= obca._E_PAR + 9 and obca.EDGE_OUT >= obca._EO_DRES + 7


def test_edge_step_restatement_rounds_and_updates():
    rec = E.case_set("exchanged")[0]
    st = E.edge_step(rec)
    np.testing.assert_array_equal(st["Z_bar"], np.round(st["Z"], 4))
    d = obca.edge_unpack(rec)
    bar = dict(local_x=d["local_x"], lamb_ij=d["lamb_ij"], lamb_bar=d["lamb_bar"], Z_bar=st["Z_bar"])
    np.testing.assert_allclose(st["lamb_bar"], obca.lambda_update(bar, d["rho"])["lamb_bar"], rtol=0, atol=1e-15)


# ---------------------------------------------------------------------------------------------
# OBCAPlanner's host logic on the CPU (the two launches answered by the restatements) against the
# plain loop written from the script
# ---------------------------------------------------------------------------------------------
def _run(n_scen, prob, steps, **kw):
    stages = []
    pl = obca.OBCAPlanner(E.OracleBatch(), n_scenarios=n_scen, prob=prob, t_step0=12, round_decimals=-1,
                          on_stage=lambda name, inp, outp: stages.append((name, inp, outp)), **kw)
    return pl, stages, pl.run(steps)


def test_planner_equals_the_plain_loop_and_shifts_the_previous_iterate():
    pl, stages, rec = _run(3, [1, 0, 1], 2, max_admm_iter=2, primal_thres=[0.01, 0.01, np.inf],
                           dual_thres=[0.01, 0.01, np.inf])
    iters = E.check_planner_structure(pl, stages, rec, 12)
    assert np.all(iters[:, 2] == 1) and np.all(iters[:, :2] >= 2)
    shifts = [s for s in stages if s[0] == "shift"]
    for s, (prob, thr) in enumerate(((1, 0.01), (0, 0.01), (1, np.inf))):
        ref = E.planner(2, prob, 12, max_admm_iter=2, primal_thres=thr, dual_thres=thr, round_decimals=-1)
        np.testing.assert_array_equal(np.asarray(rec.iter_num_record)[:, s], ref["iter_num_record"])
        np.testing.assert_array_equal(np.asarray(rec.state_record)[:, s], np.asarray(ref["state_record"]))
        np.testing.assert_array_equal(np.asarray(rec.lambda_record)[:, s], np.asarray(ref["lambda_record"]))
        for step in range(2):
            for key, val in ref["shift_in"][step].items():
                np.testing.assert_array_equal(shifts[step][1]["bar_prev"][s][key], val)


def test_planner_update_lamb_ij():
    pl, stages, rec = _run(1, 1, 1, max_admm_iter=0, update_lamb_ij=1)
    _, inp, outp = [s for s in stages if s[0] == "exchange"][0]
    for v in (0, 1):
        np.testing.assert_array_equal(outp["bar"][0]["lamb_ij"][v], inp["fullx"][0][v][:, 5:])
    ref = E.planner(1, 1, 12, max_admm_iter=0, update_lamb_ij=1, round_decimals=-1)
    np.testing.assert_array_equal(np.asarray(rec.lambda_record)[:, 0], np.asarray(ref["lambda_record"]))
    off = _run(1, 1, 1, max_admm_iter=0, update_lamb_ij=0)[2]
    assert not np.array_equal(np.asarray(off.lambda_record), np.asarray(rec.lambda_record))
