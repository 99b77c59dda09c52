"""The ownership of the device OBCA plan's memory (csrc/piadmm_obca_plan.h: dev_buf, the attach and
detach of every feature, plan_end and a second fleet_begin on the same handle), across features at
once; the attach / detach tests of each feature touch it one feature at a time.

Handle A carries a plan through every attachment (the order, the dual law, feedback with a tape and
noise -- or the clocks, which refuse feedback -- and a trace), one MPC step, the replacement of each
attachment by another, the detachment of all of them and piadmm_obca_plan_end; then a second
piadmm_obca_fleet_begin on other inputs and two traced steps.  A fresh handle B runs that second
plan alone.  The plan is bit-exact and deterministic, so whatever an earlier plan of the handle
owned, freed or left behind must not show: state, controls, iterates, status masks and the trace's
states of A and B are compared bit for bit.

n = 3 is one partial workgroup of PW = 4 waves, n = 5 one full and one partial; n_ref = 12, trace and
tape capacity 2, a reference and a parameter row per scenario."""
import numpy as np
import pytest

import _obca_dual_cases as D
import _obca_fleet_cases as F
import _obca_noise_cases as Z
import test_gpu_obca_plan as P
from piadmm import obca

pytestmark = pytest.mark.gpu

_bits = P._bits
N_REF, CAP = 12, 2
FIRST = {3: ([0, 1, 2], 12), 5: ([0, 1, 2, 3, 1], 12)}       # the plan that goes: cases, the reference's first row
LAST = {3: ([2, 0, 1], 5), 5: ([3, 2, 1, 0, 2], 5)}          # the plan that is compared: other cases, another row


def _kwargs(cases, t0, c0=None):
    """A fleet of `cases` on rows t0 .. t0 + 11 of each scenario's reference; scenario s is seeded at
    row c0[s] of those (0 without clocks), as the planner's constructor seeds a plan."""
    kw = F.fleet_kwargs(cases, 0)
    specs = kw.pop("specs")
    c0 = [0] * len(cases) if c0 is None else c0
    ref = np.stack([np.stack(obca.ref_traj_gen(sp))[:, t0:t0 + N_REF] for sp in specs])
    state = []
    for sp, p, c in zip(specs, kw["prob"], c0):
        init = np.stack([obca.executed_path(v, (t0 + c) * obca.DT, sp) for v in (0, 1)])
        state.append(obca.pack_state(obca.seeded_bar_state(t0 + c, p, spec=sp), init))
    return dict(kw, ref_traj=np.ascontiguousarray(ref), state=np.stack(state))


def _last_plan(batch, n):
    """The second plan's two traced steps: what is compared."""
    pl = obca.OBCADevicePlanner(batch, **_kwargs(*LAST[n]))
    pl.trace_begin(CAP)
    assert pl.trace_run(2) == 2
    got = {k: pl.get(k).copy() for k in ("STATE", "CTRL", "ITERS", "STATUS_MASK")}
    got.update({"TRACE_" + k: pl.trace_get(k).copy() for k in ("STATES", "ITERS", "STATUS_MASK")})
    pl.trace_end()
    pl.close()
    return got


def _feedback_life(b, n):
    cases, t0 = FIRST[n]
    rng = np.random.default_rng(n)
    tapes = rng.normal(0.0, Z.SIGMA, (2, n, CAP, 2, 5))
    pars = (np.stack([obca.feedback_row(method=s % 2, n_sub=1 + s) for s in range(n)]), obca.feedback_row(gain_a=0.9))
    noises = (dict(par=np.stack([obca.noise_row(sigma=Z.SIGMA)] * n), streams=np.arange(n)[::-1] + 2 ** 32, seed=2 ** 63 + 5, k0=7),
              dict(par=obca.noise_row(sigma=Z.SIGMA, trunc=1.5), seed=3))
    pl = obca.OBCADevicePlanner(b, order=True, dual=D.fleet_gains(cases), feedback=dict(par=pars[0], tape=tapes[0]),
                                noise=noises[0], **_kwargs(cases, t0))
    pl.trace_begin(CAP)
    pl.step()
    # every attachment again, as a replacement, with other arguments
    pl.set_order(np.arange(2 * n, dtype=np.int32).reshape(n, 2))
    pl.set_dual(**D.GAINS)
    pl.set_feedback(par=pars[1], tape=tapes[1])
    pl.set_noise(**noises[1])
    pl.trace_begin(CAP, keep_lambda=False)
    assert pl.trace_rows() == 0 and pl.feedback_steps() == 0
    pl.clear_noise()
    pl.clear_feedback()
    pl.clear_dual()
    pl.clear_order()
    pl.trace_end()
    pl.close()


def _clock_life(b, n):
    cases, t0 = FIRST[n]
    rows = np.array([[s % 3, N_REF - (s % 2)] for s in range(n)], np.int32)       # mixed phases and lengths
    pl = obca.OBCADevicePlanner(b, order=True, dual=D.fleet_gains(cases), clock=rows,
                                **_kwargs(cases, t0, c0=rows[:, 0]))
    pl.trace_begin(CAP)
    pl.step()
    pl.trace_end()                      # an admission and an import refuse a trace
    pl.admit([1], np.array([[1, N_REF]], np.int32))
    blob = pl.export_tenants([1])       # the staging buffer grows here, once: the import fits it
    pl.import_tenants([1], blob)
    assert pl.export_tenants([1]) == blob
    pl.trace_begin(CAP)
    pl.step()
    # every attachment again, as a replacement, with other arguments
    pl.set_order(np.arange(2 * n, dtype=np.int32).reshape(n, 2))
    pl.set_dual(**D.GAINS)
    pl.set_clock(None)                  # everyone on the plan's step over the whole reference: detachable
    pl.trace_begin(CAP, keep_lambda=False)
    assert pl.trace_rows() == 0 and pl.alive().all()
    pl.clear_clock()
    pl.clear_dual()
    pl.clear_order()
    pl.trace_end()
    pl.close()


@pytest.mark.parametrize("n", [3, 5])
@pytest.mark.parametrize("life", [_feedback_life, _clock_life], ids=["feedback", "clock"])
def test_second_plan_of_a_used_handle_is_a_fresh_handles(life, n):
    from piadmm.solver import device_count
    if device_count() < 1:
        pytest.fail("no HIP device visible: the GPU tests need an MI355X")
    a, b = obca.OBCABatch(0), obca.OBCABatch(0)
    try:
        life(a, n)
        got, want = _last_plan(a, n), _last_plan(b, n)
    finally:
        a.close()
        b.close()
    assert got["TRACE_STATES"].shape == (CAP + 1, n, 2, 5) and got["TRACE_ITERS"].all()
    for key in want:
        _bits(got[key], want[key], key)
