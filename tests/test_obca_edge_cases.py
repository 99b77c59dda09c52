"""The hard-branch case sets of the OBCA-ADMM edge step (tests/_obca_edge_cases.py) proved on the
CPU from the restatement's trace: the slots kept are stable under a relative 1e-13 perturbation
of the record, their converged answers are KKT points of the slot NLP, the coverage table holds,
and every moved field changes what the parity tests compare.  No GPU.
"""
import functools

import numpy as np
import pytest

import _obca_edge_cases as K
import _obca_edge_ref as E
from piadmm import obca

Z_STABLE = 1e-9          # 100 times below the GPU bar on Z (ATOL 1e-7)
Y_STABLE = 1e-9          # and on the multipliers (MULT_TOL 1e-7, of max(1, |y|)): a degenerate vertex


def _rel(got, ref):
    got, ref = np.atleast_1d(got), np.atleast_1d(ref)
    return float(np.abs(got - ref).max() / max(1.0, np.abs(ref).max()))


@functools.lru_cache(maxsize=None)
def _unstable(name):
    """[(record, slot)] of a set that fail the stability filter under a draw of K.STABILITY_SEEDS."""
    return sorted(set().union(*(_unstable_under(name, seed) for seed in K.STABILITY_SEEDS)))


def _unstable_under(name, seed):
    rng = np.random.default_rng([seed, K.SET_NAMES.index(name)])
    out = []
    for k, rec in enumerate(K.case_set(name)):
        pert = rec.copy()
        pert[:obca._E_PAR] *= 1.0 + 1e-13 * rng.uniform(-1.0, 1.0, obca._E_PAR)
        for t, (p, r) in enumerate(E.solve_record(rec)):
            r2 = E.solve_slot(E.Slot(pert, t))
            same = (r2.status, r2.iters, r2.qp_steps) == (r.status, r.iters, r.qp_steps)
            if not same or not float(np.abs(r2.z - r.z).max()) <= Z_STABLE:
                out.append((k, t))
            elif r.status in E.WRITES_ITERATE and not max(_rel(r2.y_eq, r.y_eq), _rel(r2.y_in, r.y_in),
                                                          _rel(r2.y_bnd, r.y_bnd)) <= Y_STABLE:
                out.append((k, t))
    return out


def _kept(name):
    recs = K.case_set(name)
    sol = [E.solve_record(rec) for rec in recs]
    return [(k, t) + sol[k][t] for k, t in K.kept(name)]


def test_trace_leaves_the_result_alone():
    n = 0
    for rec in E.case_set("pressed"):
        for t in range(obca.NT):
            p = E.Slot(rec, t)
            a, tr = E.solve_slot(p), []
            b = E.solve_slot(p, trace=tr)
            assert (a.status, a.iters, a.qp_steps, a.cost, a.y_in) == (b.status, b.iters, b.qp_steps, b.cost, b.y_in)
            for x, y in ((a.z, b.z), (a.y_eq, b.y_eq), (a.y_bnd, b.y_bnd)):
                np.testing.assert_array_equal(x, y)
            assert len(tr) == b.iters and all(x["qst"] == 0 for x in tr)
            n += sum(len(x["active"]) for x in tr)
    assert n > 0
    # and gi_qp's counter: same answer, bit for bit, on a QP that drops rows
    rec = K.case_set("tight_mu")[4]
    hit = 0
    for t, (p, r) in enumerate(E.solve_record(rec)):
        hit += sum(x["drops"] for x in r.trace)
        plain = E.solve_slot(p)
        assert (plain.status, plain.iters, plain.qp_steps) == (r.status, r.iters, r.qp_steps)
        np.testing.assert_array_equal(plain.z, r.z)
    assert hit > 0


@pytest.mark.parametrize("name", K.SET_NAMES)
def test_sets_are_small_and_the_excluded_slots_are_the_unstable_ones(name):
    recs = K.case_set(name)
    assert len(recs) <= 20
    bad = _unstable(name)
    print(f"{name}: {len(recs)} records, unstable {bad}")
    assert len(bad) <= 0.10 * len(recs) * obca.NT
    assert sorted(K.EXCLUDED[name]) == bad, (name, bad)


@pytest.mark.parametrize("name", K.SET_NAMES)
def test_kept_converged_slots_are_kkt_points(name):
    conv = [s for s in _kept(name) if s[3].status == E.CONVERGED]
    assert len(conv) >= 5
    for k, t, p, r in conv:
        kk = E.kkt_residual_edge(p, r.z, r.y_eq, r.y_in, r.y_bnd)
        assert kk["stat"] <= 1e-9 * kk["gscale"], (name, k, t, kk)
        assert kk["feas"] <= 1e-8 and kk["comp"] <= 1e-8, (name, k, t, kk)


def test_coverage_table():
    slots = {name: _kept(name) for name in K.RECIPES}
    for branch, names in K.COVERAGE.items():
        count = {name: sum(K.reaches(branch, p, r) for _, _, p, r in slots[name]) for name in slots}
        print(f"{branch:24s} " + "  ".join(f"{a} {b}" for a, b in count.items()))
        for name in names:
            assert count[name] >= 1, (branch, name)
        assert sum(count[name] for name in names) >= K.MIN_SLOTS, (branch, count)
    for branch in K.NOT_REACHED:
        assert branch not in K.COVERAGE
        for name in slots:
            assert not any(K.reaches(branch, p, r) for _, _, p, r in slots[name]), (branch, name)
    # the table has a line for every hard branch of the SQP
    assert set(K.COVERAGE) | set(K.NOT_REACHED) >= {
        "modification", "tau_ladder", "previous_rows_in_Ga", "qp_drop", "qp_dual_step_drop", "upper_range_row", "lower_upper_and_range",
        "two_halvings", "cold_converged", "max_iter_60", "hessian_fail", "linesearch_fail", "qp_step_limit"}


def _compared(rec):
    """What the parity tests compare of one record, kept apart per slot."""
    st = E.edge_step(rec)
    sol = E.solve_record(rec)
    return [(r.status, r.iters, r.qp_steps, r.z.tobytes(), st["Z_bar"][:, t].tobytes(), st["lamb_bar"][:, t].tobytes())
            for t, (_, r) in enumerate(sol)]


@pytest.mark.parametrize("name", K.SET_NAMES)
def test_every_moved_field_changes_a_kept_slot(name):
    recs, org = K.case_set(name), K.origin(name)
    keep = set(K.kept(name))
    fields = sorted({f for _, moved in org for f in moved})
    assert fields
    for f in fields:
        found = False
        for k, (base, moved) in enumerate(org):
            if f not in moved:
                continue
            # the record with this one field put back
            back = recs[k].copy()
            if f == "lamb_bar":
                back[obca._E_LB:obca._E_LB + 126] = base[obca._E_LB:obca._E_LB + 126]
            else:
                back[obca._E_PAR + K.FIELDS[f]] = base[obca._E_PAR + K.FIELDS[f]]
            a, b = _compared(recs[k]), _compared(back)
            if any(a[t] != b[t] for t in range(obca.NT) if (k, t) in keep):
                found = True
                break
        assert found, (name, f)
