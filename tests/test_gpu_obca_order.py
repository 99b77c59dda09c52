"""The longest-first scenario order of the device-resident OBCA-ADMM plan (k_plan_work and
k_plan_order in csrc/piadmm_obca_plan_attach.hip behind piadmm_obca_order_plan / piadmm_obca_order;
OBCADevicePlanner(order=True, work_init=...), OBCABatch.order), against the host statements
piadmm.obca.plan_order / plan_work.

Bars.  Everything here is integers or copies: the sorted lists and the work record are
integer-equal to the host statements, and because every scenario's answer is independent of its
place in the list, every per-scenario item of an ordered plan is bit-equal to the plain plan's.

What ACTIVE shows: the list the last iterate ran with.  The list an iterate leaves for the next one
is therefore checked one iterate later, against plan_order of the set the earlier iterate kept and
of the work record read after that earlier iterate (k_plan_order reads the record k_plan_work of
the same iterate has written)."""
import numpy as np
import pytest

import _obca_dual_cases as C
import _obca_fleet_cases as F
import _obca_order_cases as R
import test_gpu_obca_plan as P
from piadmm import _lib, obca

pytestmark = pytest.mark.gpu

SETUP, _bits = P.SETUP, P._bits
CASES = [0, 1, 2, 3]
PLANS = {"setup": (dict(SETUP, n_scenarios=3), C.GAINS),
         "fleet": (F.fleet_kwargs(CASES, 12), C.fleet_gains(CASES))}
ITEMS = ("STATE", "STATE_PREV", "X", "CTRL", "ITERS", "STATUS_MASK", "PRIMAL", "DUAL", "LAMBDA", "STOP", "CONVERGE")
TRACE_ITEMS = ("STATES", "CLEARANCE", "ITERS", "STATUS_MASK", "PRIMAL", "DUAL", "LAMBDA", "SUMMARY")


@pytest.fixture(scope="module")
def batches():
    """(the handle under test, a second handle)."""
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    b, ref = obca.OBCABatch(0), obca.OBCABatch(0)
    yield b, ref
    b.close()
    ref.close()


# ---------------------------------------------------------------------------------------------
# 1. the kernel alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", R.SIZES)
@pytest.mark.parametrize("kind", R.KINDS)
def test_kernel_alone(batches, kind, m):
    b, _ = batches
    lst, work = R.alone_case(kind, m)
    assert len(lst) == m and len(set(lst.tolist())) == m
    if kind == "subset":
        assert len(work) == R.SUBSET_N and (m == 1 or np.any(np.diff(lst) < 0))
    if kind == "clamp" and m >= 63:
        assert (work >= R.CLAMP).any() and (work < R.CLAMP).any()
    lst_in, work_in = lst.copy(), work.copy()
    got = b.order(lst, work)
    assert np.array_equal(lst, lst_in) and np.array_equal(work, work_in)
    want = obca.plan_order(lst, work)
    assert got.dtype == want.dtype == np.int32
    assert got.tolist() == want.tolist(), (kind, m)
    # a function of the set alone: the sorted list comes out of any order of the same entries
    assert b.order(lst[::-1].copy(), work).tolist() == want.tolist()
    if kind == "equal":
        assert got.tolist() == sorted(lst.tolist())


# ---------------------------------------------------------------------------------------------
# 2. the ordered plan computes the same plan
# ---------------------------------------------------------------------------------------------
def _same(po, pp, where):
    for key in ITEMS:
        _bits(po.get(key), pp.get(key), f"{key} {where}")
    if po.dual_par is not None:
        for key in ("DUAL_S", "DUAL_D"):
            _bits(po.get(key), pp.get(key), f"{key} {where}")


@pytest.mark.parametrize("law", [False, True])
@pytest.mark.parametrize("plan", ["setup", "fleet"])
def test_the_ordered_plan_computes_the_same_plan(batches, plan, law):
    b, ref = batches
    kw, gains = PLANS[plan]
    extra = dict(dual=gains) if law else {}
    n = kw["n_scenarios"]
    po = obca.OBCADevicePlanner(b, order=True, work_init=R.reversing_work(n), **kw, **extra)
    pp = obca.OBCADevicePlanner(ref, **kw, **extra)
    if law:
        po.trace_begin(2)
        pp.trace_begin(2)
    lists, stops = [], []
    for step in range(2):
        left, i_iter = n, 0
        while left:
            i_iter += 1
            left = po.iterate()
            assert pp.iterate() == left
            act_o, act_p = po.get("ACTIVE").tolist(), pp.get("ACTIVE").tolist()
            assert sorted(act_o) == act_p
            lists.append(act_o)
            _same(po, pp, f"after iterate {i_iter} of step {step}")
        stops.append(po.get("ITERS").tolist())
        po.shift()
        pp.shift()
        _same(po, pp, f"after the shift of step {step}")
    # the coverage this test stands on: the seeded first list is the reverse of the identity, and
    # the compaction ran on it (the stop iterates differ between the scenarios)
    assert lists[0] == list(range(n))[::-1]
    assert max(stops[0]) == 3 and min(stops[0]) == 1 and len(lists[1]) < n
    if plan == "fleet" and not law:
        assert stops == [F.STOP_ITERS, F.STOP_ITERS]
    if law:
        for key in TRACE_ITEMS:
            _bits(po.trace_get(key), pp.trace_get(key), f"trace {key}")
        assert po.trace_rows() == 2
    po.close()
    pp.close()


# ---------------------------------------------------------------------------------------------
# 3. the list is the stated order, the record the stated work
# ---------------------------------------------------------------------------------------------
def test_the_list_is_the_stated_order(batches):
    b, _ = batches
    kw = PLANS["fleet"][0]
    n = kw["n_scenarios"]
    seed = R.reversing_work(n)
    pl = obca.OBCADevicePlanner(b, order=True, work_init=seed, **kw)
    work = pl.work()
    assert work.dtype == np.int32 and work.tolist() == seed.tolist()
    kept = list(range(n))
    lists = []
    for step in range(2):
        i_iter = 0
        while kept:
            i_iter += 1
            left = pl.iterate()
            act = pl.get("ACTIVE").tolist()
            assert act == obca.plan_order(kept, work).tolist(), (step, i_iter, act, kept, work.tolist())
            lists.append(act)
            # the record: this iterate's work for the scenarios that ran (the IST items follow the
            # list the iterate ran with), unchanged for the others
            want = work.copy()
            want[act] = obca.plan_work(pl.get("LOCAL_IST"), pl.get("EDGE_IST"))
            work = pl.work()
            assert work.tolist() == want.tolist(), (step, i_iter)
            stop = pl.get("STOP")
            kept = [s for s in act if not stop[s]]
            assert left == len(kept)
        pl.shift()
        assert pl.work().tolist() == work.tolist()          # the shift sorts by the record, it does not write it
        kept = list(range(n))
    # one more iterate shows the list the second shift left
    pl.iterate()
    act = pl.get("ACTIVE").tolist()
    assert act == obca.plan_order(kept, work).tolist()
    lists.append(act)
    # guaranteed by work_init, whatever the solves count:
    assert lists[0] == list(range(n))[::-1]
    assert [len(v) for v in lists[:3]] == [4, 3, 2]          # stop iterates [3, 3, 2, 1]: the compaction ran
    later = [v for v in lists[1:] if v != sorted(v)]
    print(f"ordered lists {lists}; lists after the first that are not ascending: {len(later)} of {len(lists) - 1}; "
          f"work after 2 steps {work.tolist()}")
    pl.close()


# ---------------------------------------------------------------------------------------------
# 4. position independence under ordering
# ---------------------------------------------------------------------------------------------
def _final(pl):
    return dict(STATE=pl.get("STATE"), X=pl.get("X"), ITERS=pl.get("ITERS"), LAMBDA=pl.get("LAMBDA"),
                iter_num_record=np.asarray(pl.record.iter_num_record))


@pytest.fixture(scope="module")
def alone(batches):
    """Each of the four cases run alone, unordered, for 2 MPC steps (computed once, never changed)."""
    b, _ = batches
    out = []
    for c in range(4):
        pl = obca.OBCADevicePlanner(b, **F.single_kwargs(c, 12))
        pl.run(2)
        out.append(_final(pl))
        pl.close()
    return out


@pytest.mark.parametrize("n", [1, 5, 70])
def test_position_independence_under_ordering(batches, alone, n):
    b, _ = batches
    cases = [k % 4 for k in range(n)]
    seed = R.random_work(n, 7 + n)
    pl = obca.OBCADevicePlanner(b, order=True, work_init=seed, **F.fleet_kwargs(cases, 12))
    pl.iterate()
    first = pl.get("ACTIVE").tolist()
    assert first == obca.plan_order(range(n), seed).tolist()
    if n > 1:
        assert first != sorted(first)                       # the seed does reorder the list
    pl.close()
    pl = obca.OBCADevicePlanner(b, order=True, work_init=seed, **F.fleet_kwargs(cases, 12))
    pl.run(2)
    got = _final(pl)
    pl.close()
    for k, c in enumerate(cases):
        for key in ("STATE", "X", "ITERS", "LAMBDA"):
            _bits(got[key][k], alone[c][key][0], f"{key} of scenario {k}")
        _bits(got["iter_num_record"][:, k], alone[c]["iter_num_record"][:, 0], f"stop iterates of scenario {k}")
    assert got["iter_num_record"].tolist() == [[F.STOP_ITERS[c] for c in cases]] * 2


# ---------------------------------------------------------------------------------------------
# 5. attach, detach, refusals
# ---------------------------------------------------------------------------------------------
def test_attach_detach_and_refusals(batches):
    b, ref = batches
    lib = b._lib
    kw = PLANS["fleet"][0]
    n = kw["n_scenarios"]
    probe = np.zeros((n, 2), np.int32)
    code = obca.PLAN_GET["WORK"][0]

    def no_order():
        assert lib.piadmm_obca_plan_get(b._h, code, probe.ctypes.data, probe.nbytes) == _lib.E_STATE
        assert b"no order attached" in lib.piadmm_obca_last_error(b._h)

    # no plan open
    assert lib.piadmm_obca_order_plan(b._h, 1, None) == _lib.E_STATE
    assert b"no open plan" in lib.piadmm_obca_last_error(b._h)
    pl = obca.OBCADevicePlanner(b, **kw)
    start = pl.get("STATE")
    no_order()
    # mode 2, a negative seed (the row is named): PIADMM_E_ARG, nothing attached
    assert lib.piadmm_obca_order_plan(b._h, 2, None) == _lib.E_ARG
    assert b"mode 0 (detach) or 1 (attach)" in lib.piadmm_obca_last_error(b._h)
    bad = R.reversing_work(n)
    bad[2, 1] = -1
    assert lib.piadmm_obca_order_plan(b._h, 1, _lib.iptr(bad)) == _lib.E_ARG
    assert b"obca_order_plan: row 2: " in lib.piadmm_obca_last_error(b._h)
    no_order()
    # the kernel-alone call: a repeated or out-of-range entry, m > n, negative work
    out = np.zeros(3, np.int32)
    w3 = np.zeros((3, 2), np.int32)
    for lst in ([0, 1, 1], [0, 1, 3], [0, -1, 2]):
        a = np.array(lst, np.int32)
        assert lib.piadmm_obca_order(b._h, _lib.iptr(a), 3, _lib.iptr(w3), 3, _lib.iptr(out)) == _lib.E_ARG
        assert b"obca_order: list[" in lib.piadmm_obca_last_error(b._h)
    a = np.arange(3, dtype=np.int32)
    assert lib.piadmm_obca_order(b._h, _lib.iptr(a), 3, _lib.iptr(w3), 2, _lib.iptr(out)) == _lib.E_ARG
    assert lib.piadmm_obca_order(b._h, _lib.iptr(a), 0, _lib.iptr(w3), 3, _lib.iptr(out)) == _lib.E_ARG
    neg = w3.copy()
    neg[1, 0] = -4
    assert lib.piadmm_obca_order(b._h, _lib.iptr(a), 3, _lib.iptr(neg), 3, _lib.iptr(out)) == _lib.E_ARG
    assert b"obca_order: row 1: " in lib.piadmm_obca_last_error(b._h)
    assert not out.any()
    _bits(pl.get("STATE"), start, "the plan is unchanged")
    # attaching with zero work leaves the list as it was: the next iterate runs the ascending list
    pl.set_order()
    assert not pl.work().any()
    pl.iterate()
    assert pl.get("ACTIVE").tolist() == list(range(n))
    # mid-step: neither attaching nor detaching, and the record stays
    work = pl.work()
    for mode in (1, 0):
        assert lib.piadmm_obca_order_plan(b._h, mode, None) == _lib.E_STATE
        assert b"only at a step boundary" in lib.piadmm_obca_last_error(b._h)
    with pytest.raises(_lib.PiadmmError, match="only at a step boundary") as ei:
        pl.set_order(R.reversing_work(n))
    assert ei.value.code == _lib.E_STATE
    assert pl.work().tolist() == work.tolist()
    while pl.counts()[1]:
        pl.iterate()
    pl.shift()
    # at the boundary a seed replaces the record and re-sorts the list at once
    pl.set_order(R.reversing_work(n))
    assert pl.work().tolist() == R.reversing_work(n).tolist()
    # detaching restores the ascending list; the step then equals that of a plan that never had the order
    pl.clear_order()
    assert not pl.order
    no_order()
    state = pl.get("STATE")
    t_step = int(pl.get("T_STEP")[0])
    never = obca.OBCADevicePlanner(ref, state=state, **dict(kw, t_step0=t_step))
    _bits(never.get("STATE"), state, "same start")
    pl.iterate()
    never.iterate()
    assert pl.get("ACTIVE").tolist() == list(range(n))
    for key in ("LOCAL_REC", "LOCAL_OUT", "LOCAL_IST", "EDGE_REC", "EDGE_OUT", "EDGE_IST"):
        _bits(pl.get(key), never.get(key), f"{key} after detaching")
    while pl.counts()[1]:
        assert pl.iterate() == never.iterate()
    pl.shift()
    never.shift()
    for key in ITEMS:
        _bits(pl.get(key), never.get(key), f"{key} after detaching")
    never.close()
    # the end of the plan frees the record: a new plan has none
    pl.set_order()
    pl.close()
    assert lib.piadmm_obca_order_plan(b._h, 0, None) == _lib.E_STATE
    again = obca.OBCADevicePlanner(b, **kw)
    no_order()
    again.close()


# ---------------------------------------------------------------------------------------------
# 6. Python
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["run", "run_traced"])
def test_python_records(batches, how):
    b, ref = batches
    kw = dict(SETUP, n_scenarios=3)
    pp = obca.OBCADevicePlanner(ref, **kw)
    po = obca.OBCADevicePlanner(b, order=True, work_init=R.reversing_work(3), **kw)
    assert po.order and not pp.order
    tp, to = getattr(pp, how)(3), getattr(po, how)(3)
    for k in ("state_record", "iter_num_record", "lambda_record"):
        _bits(np.asarray(getattr(po.record, k)), np.asarray(getattr(pp.record, k)), k)
    for ro, rp in zip(po.record.status_record, pp.record.status_record):
        assert sorted(ro) == sorted(rp)
        for key in ro:
            _bits(np.asarray(ro[key]), np.asarray(rp[key]), f"status_record {key}")
    if how == "run_traced":
        for f in ("states", "clearance", "iters", "status_mask", "primal", "dual", "min_clearance", "min_row",
                  "min_clearance_tight", "iters_sum", "lamb"):
            _bits(getattr(to, f), getattr(tp, f), f"trace {f}")
    _bits(po.get("STATE"), pp.get("STATE"), "STATE")
    assert po.work().shape == (3, 2) and po.t_step == pp.t_step == SETUP["t_step0"] + 3
    po.close()
    pp.close()
