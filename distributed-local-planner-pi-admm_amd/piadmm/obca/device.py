"""The same loop, device-resident (csrc/piadmm_obca_plan.hip behind piadmm_obca_plan_*)."""
import ctypes
from collections import ChainMap

import numpy as np

from .. import _lib, io
from .._lib import DELAY_PAR, DUAL_PAR, FEEDBACK_PAR, FLEET_PAR, NOISE_PAR
from .attach import clock_rows, clock_tick, dual_rows
from .batch import OBCAEdgeResult, OBCAResult
from .feedback import DELAY_GET, NOISE_GET, _draw_rows, delay_row, feedback_args, noise_row
from .ledger import LEDGER_GET, LEDGER_REC, ledger_unpack
from .loop import LOOP_GET
from .model import (DT, EDGE_OUT, EDGE_REC, FLEET_ROW, N_HORZ, NT, NU, NX, OUT, REC, _spec, executed_path, ref_traj_gen,
                    seeded_bar_state)
from .planner import _planner_init, _spec_of
from .stats import TRACE_GET, TRACE_LAMBDA, OBCAFleetStats, OBCARunRecord, OBCATrace, _stats_call, trace_gather_unpack
from .tenant import PLAN_GET, PLAN_STATE, pack_state, tenant_unpack, unpack_state

# every item of piadmm_obca_plan_get: name -> (code, dtype)
_GET = ChainMap(LOOP_GET, DELAY_GET, NOISE_GET, PLAN_GET)


def _loop_args(n, plant, noise, delay, streams, each=None):
    """(plant, noise, delay, streams) as a loop call takes them, unchecked: the rows of each kind as
    rows x width (None stays None; each: the rows a kind must have), streams as n int64 or None."""
    def rows_of(par, width):
        if par is None:
            return None
        par = _draw_rows(par, width, None, n)[0]
        assert each is None or par.shape[0] == each, par.shape
        return par
    if streams is not None:
        streams = np.ascontiguousarray(streams, np.int64).reshape(-1)
        assert streams.shape == (n,), streams.shape
    return rows_of(plant, FEEDBACK_PAR), rows_of(noise, NOISE_PAR), rows_of(delay, DELAY_PAR), streams


class OBCADevicePlanner:
    """`OBCAPlanner` with the loop on the device: the planner state stays resident on the batch's
    handle and one ADMM iterate is a fixed chain of launches (csrc/piadmm_obca_plan.hip); the host
    reads back the number of scenarios still active.  Same constructor arguments, same seeding
    (`seeded_bar_state`, `executed_path`) and the same OBCARunRecord fields as OBCAPlanner.

    Without on_stage a step is one `piadmm_obca_plan_step`; status_record then keeps one entry per
    MPC step: the iterate each scenario stopped at and, per scenario, the OR of (1 << status) over
    its local and its edge solves (nothing is silent).  With on_stage the step goes iterate by
    iterate, the callback sees the six stages of OBCAPlanner built from `get`, and status_record
    keeps one entry per iterate as OBCAPlanner's does.

    The planner takes the batch's device buffers over (include/piadmm.h): `batch.upload` / `solve`
    / `solve_edge` on the same batch end the plan.

    With `specs`, a reference per scenario (ref_traj n x 2 x n_ref x 5) or a sequence for any
    parameter of FLEET_ROW the plan is a fleet (`self.fleet`): it is opened by
    piadmm_obca_fleet_begin with one reference and one parameter row (`par`) per scenario.
    Otherwise it is opened by piadmm_obca_plan_begin, as ever.

    With order=True every active list is kept longest first by the work of each scenario's last
    solves (piadmm_obca_order_plan; `work_init` n x 2 seeds the record, `work()` reads it): the
    per-scenario results are the same bit for bit, ACTIVE and the LOCAL_ / EDGE_ items follow the
    list's order.

    With clock= every scenario has its own MPC step and reference length (piadmm_obca_clock_plan):
    clock is n x 2 rows (c0, len), or True for everyone at t_step0 over the whole reference.
    Scenario s is seeded at its own c0 and reads its reference at its own step; once c + 8 > len it
    is retired and frozen while the others go on.  `clock()` reads the record, `admit` puts new
    tenants into slots, `run` / `run_traced` stop when nothing is alive.  t_step counts the plan's
    steps.

    Running tenants move as records (piadmm_obca_tenant_export / _import): `export_tenants` of any
    plan, `import_tenants` into a clocked fleet plan, `compact()` for a new planner with the alive
    tenants only, `save` / `load` for a checkpoint of the whole plan; a moved tenant continues bit
    for bit.

    With feedback=dict(par=, tape=) a step closes through a plant instead of with init_state = X[1]
    (piadmm_obca_feedback_plan, `propagate`): par one plant row or n (`feedback_row`; None: the
    nominal plant), tape n x cap x 2 x 5 disturbance rows or None.  `set_feedback` / `clear_feedback`
    attach and detach it at a step boundary, `feedback_steps()` counts the steps closed since,
    `measure(slots, states)` writes states measured outside over init_state
    (piadmm_obca_feedback_measure; any plan, no trace).  `run_traced` works with it unchanged: the
    trace's states and clearances are those of the states the vehicles reached.  Not together with
    clock or the tenant calls.

    With noise=dict(par=, streams=, seed=, k0=) on top of feedback the disturbance is drawn on the
    device (piadmm_obca_noise_plan, k_plan_noise; `noise_tape` is the statement): scenario s at the
    step k since the feedback's attachment gets the row of stream streams[s] (None: s) at step index
    k0 + k, added behind the tape's row if there is a tape.  `set_noise` / `clear_noise` attach and
    detach it; `set_feedback` and `clear_feedback` drop it.  A scenario is re-run alone from (seed,
    its stream id, k0): a plan of the worst few with streams = their ids draws what they drew.

    With delay=dict(par=, streams=, seed=, k0=, tape=) the exchange is stale (piadmm_obca_delay_plan,
    k_plan_delay and k_plan_exchange_stale; `delay_tau` and `stale_states` are the statements): every
    vehicle sends the halfspaces of its plan interpolated back by its latency of the open step,
    `get("DELAY_TAU")`.  `set_delay` / `clear_delay` attach and detach it at a step boundary;
    independent of feedback and noise, not together with clock or the tenant calls.

    With clock= and loop=dict(plant=, noise=, delay=, streams=, seed=, k0=) the closed loop runs under
    the per-scenario clocks (piadmm_obca_loop_plan; `loop_draw` is the statement of its draws): a
    step closes through the plant under the noise row of stream streams[s] at step index k0 + c, c the
    scenario's own clock, and with delay rows the exchange is stale by the latency at k0 + c of the
    open step, `loop_tau()`.  plant one row or n (None: the nominal plant), noise / delay one row or
    n (None: that kind is absent).  `set_loop` / `clear_loop` attach and detach it at a step boundary,
    `admit(..., loop=dict(plant=, noise=, delay=, streams=))` gives an admitted tenant its own rows and
    stream; the tenant records, `compact`, `save` and `load` carry it.

    With clock= the tenant ledger records a service (piadmm_obca_ledger_begin; `OBCALedger` is the
    statement): `ledger_begin(cap)` opens a record per alive tenant, every closed step updates it on the
    device, and a tenant that retires or that `admit` / `import_tenants` replace is appended --
    `ledger_records`, `ledger_running`, `ledger_stats`, `ledger_clear`, `ledger_end`.  Not together
    with a trace; `admit` and `import_tenants` work under it."""

    def __init__(self, batch, n_scenarios, prob=1, t_step0=0, rho=1.0, min_dis=0.1, max_admm_iter=50,
                 primal_thres=0.01, dual_thres=0.01, round_decimals=4, start=1, update_lamb_ij=0, max_iter=60,
                 conv_thres=0.1, on_stage=None, max_x=150.0, max_y=20.0, r=1e4, q=1e5, x_bound=1000.0,
                 mu_max=100000.0, g_max=1000.0, ref_traj=None, state=None, specs=None, dual=None, order=False,
                 work_init=None, clock=None, feedback=None, noise=None, delay=None, loop=None):
        self._lib = batch._lib
        any_seq, (ref, ref_each), rows, t0 = _planner_init(
            self, batch, n_scenarios, prob, t_step0, primal_thres, dual_thres, update_lamb_ij, on_stage, specs,
            ref_traj, clock, rho=rho, min_dis=min_dis, conv_thres=conv_thres, max_x=max_x, max_y=max_y, r=r, q=q,
            x_bound=x_bound, mu_max=mu_max, g_max=g_max, max_admm_iter=max_admm_iter, max_iter=max_iter,
            round_decimals=round_decimals, start=start)
        self.fleet = bool(any_seq or ref_each or self.specs is not None)
        if state is None:
            seeds = {}
            for s, p in enumerate(self.prob):
                key = (p, _spec_of(self, s), t0[s])
                if key not in seeds:
                    seeds[key] = pack_state(seeded_bar_state(t0[s], p, spec=key[1]), self.init_state[s])
            state = (np.stack([seeds[(p, _spec_of(self, s), t0[s])] for s, p in enumerate(self.prob)]) if self.n
                     else np.zeros((0, PLAN_STATE)))
        state = np.ascontiguousarray(state, np.float64)
        assert state.shape == (self.n, PLAN_STATE)
        prob_a = np.ascontiguousarray(self.prob if self.n else [0], np.int32)
        if not self.fleet:
            self.par = None
            self.cfg = _lib.ObcaPlanCfgC(
                n_scenarios=self.n, t_step0=self.t_step, max_admm_iter=self.max_admm_iter,
                round_decimals=int(round_decimals), start=int(start), update_lamb_ij=int(update_lamb_ij),
                max_sqp_iter=int(max_iter), n_ref=self.n_ref, rho=self.rho, min_dis=self.min_dis,
                conv_thres=float(conv_thres), max_x=max_x, max_y=max_y, r=r, q=q, x_bound=x_bound, mu_max=mu_max,
                g_max=g_max)
            self._check(self._lib.piadmm_obca_plan_begin(batch._h, ctypes.byref(self.cfg), _lib.iptr(prob_a),
                                                         _lib.dptr(self.primal_thres), _lib.dptr(self.dual_thres),
                                                         _lib.dptr(ref), _lib.dptr(state)))
        else:
            # cfg carries what stays shared; the rows carry the rest
            self.par = np.zeros((self.n, FLEET_PAR))
            for j, name in enumerate(FLEET_ROW):
                self.par[:, j] = getattr(self, name + "_s")
            if not ref_each:
                ref = np.ascontiguousarray(self.ref_traj_s)
            self.cfg = _lib.ObcaPlanCfgC(n_scenarios=self.n, t_step0=self.t_step, update_lamb_ij=int(update_lamb_ij),
                                         n_ref=self.n_ref)
            self._check(self._lib.piadmm_obca_fleet_begin(batch._h, ctypes.byref(self.cfg), _lib.iptr(prob_a),
                                                          _lib.dptr(self.primal_thres), _lib.dptr(self.dual_thres),
                                                          _lib.dptr(ref), _lib.dptr(self.par), _lib.dptr(state)))
        self.dual_par = None
        self._feedback = None
        self._noise = None
        self._delay = None
        self._loop = None
        if dual is not None:
            self.set_dual(**dual)
        self.order = False
        if order:
            self.set_order(work_init)
        else:
            assert work_init is None, "work_init seeds the order's record: pass order=True"
        self._clock = None
        if clock is not None:
            self.set_clock(None if clock is True else rows)
        if feedback is not None:
            self.set_feedback(**feedback)
        if noise is not None:
            self.set_noise(**noise)
        if delay is not None:
            self.set_delay(**delay)
        if loop is not None:
            self.set_loop(**loop)
        self.record = OBCARunRecord()
        self.record.state_record.append(np.stack(self.init_state))

    def set_loop(self, plant=None, noise=None, delay=None, streams=None, seed=0, k0=0):
        """Attach the loop (piadmm_obca_loop_plan; a step boundary only, a clock attached): plant one
        plant row or n (None: the nominal plant), noise one noise row or n (None: no noise), delay one
        delay row or n (None: the plain exchange), streams n stream ids (None: 0 .. n-1), seed a
        uint64, k0 the step index of clock 0.  A second call replaces the first.  The library checks
        the arguments."""
        plant, noise, delay, streams = _loop_args(self.n, plant, noise, delay, streams)
        self._check(self._lib.piadmm_obca_loop_plan(
            self.batch._h, 1, _lib.dptr(plant), 0 if plant is None else len(plant), _lib.dptr(noise),
            0 if noise is None else len(noise), _lib.dptr(delay), 0 if delay is None else len(delay),
            _lib.i64ptr(streams), ctypes.c_uint64(int(seed)), int(k0)))
        self._loop = dict(plant=1 if plant is None else len(plant), noise=None if noise is None else len(noise),
                          delay=None if delay is None else len(delay), seed=int(seed), k0=int(k0))

    def clear_loop(self):
        """Detach the loop (a step boundary only): a step closes with init_state = X[1] and the exchange
        is the plain one again."""
        self._check(self._lib.piadmm_obca_loop_plan(self.batch._h, 0, None, 0, None, 0, None, 0, None, 0, 0))
        self._loop = None

    def loop_tau(self):
        """The open step's latencies, n x 2 (the LOOP_TAU item; zeros without delay rows)."""
        return self.get("LOOP_TAU")

    def set_delay(self, par=None, streams=None, seed=0, k0=0, tape=None):
        """Attach the communication delay (piadmm_obca_delay_plan; a step boundary only, no clock):
        par one delay row or n rows (`delay_row`; None: the default row), streams n stream ids (None:
        0 .. n-1), seed a uint64, k0 the step index of the open step, tape n x cap x 2 recorded
        latencies or None.  A second call replaces the first.  The library checks the arguments."""
        rows, streams = _draw_rows(delay_row() if par is None else par, DELAY_PAR, streams, self.n)
        if tape is not None:
            tape = np.ascontiguousarray(tape, np.float64)
            assert tape.ndim == 3 and tape.shape[0] == self.n and tape.shape[2] == 2, tape.shape
        self._check(self._lib.piadmm_obca_delay_plan(
            self.batch._h, 1, _lib.dptr(rows), rows.shape[0], _lib.i64ptr(streams), ctypes.c_uint64(int(seed)), int(k0),
            _lib.dptr(tape), 0 if tape is None else tape.shape[1]))
        self._delay = (rows, streams, int(seed), int(k0), tape)

    def clear_delay(self):
        """Detach the delay (a step boundary only): the exchange is the plain one again."""
        self._check(self._lib.piadmm_obca_delay_plan(self.batch._h, 0, None, 0, None, 0, 0, None, 0))
        self._delay = None

    def set_feedback(self, par=None, tape=None):
        """Attach the plant (piadmm_obca_feedback_plan; a step boundary only, no clock): par one plant
        row or n rows (None: the nominal plant), tape n x cap x 2 x 5 disturbance rows or None.  A
        second call replaces the first and starts its tape again; an attached noise is dropped."""
        rows, tape = feedback_args(self.n, dict(par=par, tape=tape))
        self._check(self._lib.piadmm_obca_feedback_plan(self.batch._h, 1, None if par is None else _lib.dptr(rows),
                                                        rows.shape[0], _lib.dptr(tape),
                                                        0 if tape is None else tape.shape[1]))
        self._feedback = (rows, tape)
        self._noise = None

    def clear_feedback(self):
        """Detach the plant (a step boundary only): a step closes with init_state = X[1] again.  An
        attached noise goes with it."""
        self._check(self._lib.piadmm_obca_feedback_plan(self.batch._h, 0, None, 0, None, 0))
        self._feedback = None
        self._noise = None

    def set_noise(self, par=None, streams=None, seed=0, k0=0):
        """Attach the device-side noise (piadmm_obca_noise_plan; a step boundary only, feedback
        attached): par one noise row or n rows (`noise_row`; None: the zero row), streams n stream ids
        (None: 0 .. n-1), seed a uint64, k0 the step index of the feedback's step 0.  A second call
        replaces the first.  The library checks the arguments."""
        rows, streams = _draw_rows(noise_row() if par is None else par, NOISE_PAR, streams, self.n)
        self._check(self._lib.piadmm_obca_noise_plan(self.batch._h, 1, _lib.dptr(rows), rows.shape[0], _lib.i64ptr(streams),
                                                     ctypes.c_uint64(int(seed)), int(k0)))
        self._noise = (rows, streams, int(seed), int(k0))

    def clear_noise(self):
        """Detach the noise (a step boundary only): the tape alone, or nothing, disturbs the plant."""
        self._check(self._lib.piadmm_obca_noise_plan(self.batch._h, 0, None, 0, None, 0, 0))
        self._noise = None

    def feedback_steps(self):
        """The steps closed since the attachment (PLAN_GET FEEDBACK_STEPS)."""
        return int(self.get("FEEDBACK_STEPS")[0])

    def measure(self, slots, states):
        """init_state of both state copies of the scenarios `slots` (ascending, distinct) = the
        measured `states` (m x 2 x 5), one scatter launch (piadmm_obca_feedback_measure; a step
        boundary, no trace); nothing else changes."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        states = np.ascontiguousarray(states, np.float64)
        assert states.shape == (len(slots), 2, NX), states.shape
        self._check(self._lib.piadmm_obca_feedback_measure(self.batch._h, len(slots), _lib.iptr(slots),
                                                           _lib.dptr(states)))
        self.init_state = list(self.init_state)
        for k, s in enumerate(slots):
            self.init_state[int(s)] = states[k].copy()

    def set_clock(self, clock_init=None):
        """Attach the per-scenario clocks (piadmm_obca_clock_plan; a step boundary only): clock_init
        n x 2 rows (c0, len), or None for everyone at the plan's step over the whole reference."""
        t_plan = int(self.get("T_STEP")[0])
        rows = clock_rows(self.n, True if clock_init is None else clock_init, t_plan, self.n_ref)
        self._check(self._lib.piadmm_obca_clock_plan(self.batch._h, 1, None if clock_init is None else _lib.iptr(rows)))
        self._clock = np.concatenate((rows, np.ones((self.n, 1), np.int32)), axis=1)

    def clear_clock(self):
        """Detach the clocks (a step boundary only; every scenario alive, on one step, over the whole
        reference): the plan is plain again at that step."""
        self._check(self._lib.piadmm_obca_clock_plan(self.batch._h, 0, None))
        if self._clock is not None:
            self.t_step = int(self._clock[0, 0])
        self._clock = None

    def clock(self):
        """The record (c, len, alive) per scenario, n x 3 (PLAN_GET CLOCK)."""
        return self.get("CLOCK")

    def alive(self):
        """The scenarios the next step runs: every one without a clock, else the alive ones."""
        return np.ones(self.n, bool) if self._clock is None else self._clock[:, 2].astype(bool)

    def admit(self, slots, clock, state=None, ref=None, par=None, prob=None, primal_thres=None, dual_thres=None,
              specs=None, loop=None):
        """New tenants into `slots` of the clocked plan (piadmm_obca_clock_admit; a step boundary, no
        trace): clock m x 2 rows (c0, len); state m x 556, ref m x 2 x n_ref x 5, par m x FLEET_PAR,
        prob, primal_thres, dual_thres m each -- None keeps what the slot has.  With specs= (one
        OvertakeSpec per tenant) a missing ref is the spec's reference and a missing state the
        state seeded at the tenant's c0, as the constructor seeds it.  With the loop attached the
        slot keeps its loop rows and stream id and its latency is drawn at the new c0; loop=dict(plant=,
        noise=, delay=, streams=) then sets them (piadmm_obca_loop_admit: m rows of a kind, which the
        loop must hold per scenario; m stream ids; None keeps)."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        m = len(slots)
        clock = np.ascontiguousarray(clock, np.int32)
        assert clock.shape == (m, 2), clock.shape
        if prob is not None:
            prob = np.ascontiguousarray(np.broadcast_to(np.asarray(prob, np.int32), (m,)))
        if specs is not None:
            specs = [_spec(sp) for sp in specs]
            assert len(specs) == m
            if ref is None:
                ref = np.stack([np.stack(ref_traj_gen(sp)) for sp in specs])
            if state is None:
                pr = [self.prob[s] for s in slots] if prob is None else prob
                state = np.stack([pack_state(seeded_bar_state(int(c), int(p_), spec=sp),
                                             np.stack([executed_path(v, int(c) * DT, sp) for v in (0, 1)]))
                                  for sp, c, p_ in zip(specs, clock[:, 0], pr)])

        def arr(a, shape):
            if a is None:
                return None
            a = np.ascontiguousarray(a, np.float64)
            assert a.shape == shape, (a.shape, shape)
            return a
        state, ref = arr(state, (m, PLAN_STATE)), arr(ref, (m, 2, self.n_ref, NX))
        par = arr(par, (m, FLEET_PAR))
        primal_thres, dual_thres = arr(primal_thres, (m,)), arr(dual_thres, (m,))
        self._check(self._lib.piadmm_obca_clock_admit(self.batch._h, m, _lib.iptr(slots), _lib.iptr(clock),
                                                      _lib.dptr(state), _lib.dptr(ref), _lib.dptr(par), _lib.iptr(prob),
                                                      _lib.dptr(primal_thres), _lib.dptr(dual_thres)))
        self._mirror(slots, clock, 1, state, ref, par, prob, primal_thres, dual_thres, specs)
        if loop is not None:
            # last: a refusal here leaves the slots admitted, on their earlier loop rows, and the copies true
            self.loop_admit(slots, **loop)

    def _mirror(self, slots, clock, alive, state, ref, par, prob, primal_thres, dual_thres, specs):
        """The host's copies of what `slots` now hold: their clock rows (c, len) and alive flags, and
        of the rest what is not None (None keeps the copy)."""
        self._clock[slots, :2] = clock
        self._clock[slots, 2] = alive
        if ref is not None:
            self.ref_traj_s = np.array(self.ref_traj_s)
            self.ref_traj_s[slots] = ref
            self.ref_traj = None
        if par is not None:
            self.par[slots] = par
            for j, name in enumerate(FLEET_ROW):
                col = getattr(self, name + "_s").astype(np.float64)
                col[slots] = par[:, j]
                setattr(self, name + "_s", col)
        if primal_thres is not None:
            self.primal_thres[slots] = primal_thres
        if dual_thres is not None:
            self.dual_thres[slots] = dual_thres
        for k, s in enumerate(slots):
            if state is not None:
                self.init_state[s] = unpack_state(state[k])[1]
            if prob is not None:
                self.prob[s] = int(prob[k])
            if specs is not None and self.specs is not None:
                self.specs[s] = specs[k]

    def loop_admit(self, slots, plant=None, noise=None, delay=None, streams=None):
        """The loop rows and stream ids of `slots` (piadmm_obca_loop_admit; a step boundary, no trace):
        m rows of a kind the loop holds per scenario, m stream ids; None keeps what the slot has."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        m = len(slots)
        plant, noise, delay, streams = _loop_args(m, plant, noise, delay, streams, each=m)
        self._check(self._lib.piadmm_obca_loop_admit(self.batch._h, m, _lib.iptr(slots), _lib.dptr(plant), _lib.dptr(noise),
                                                     _lib.dptr(delay), _lib.i64ptr(streams)))

    # -- running tenants: export, import, compaction, checkpoints (piadmm_obca_tenant_export / _import) --
    TENANT_ITEMS = ("STATE", "STATE_PREV", "CTRL", "CTRL_PREV", "X", "LAMBDA", "PRIMAL", "DUAL", "PRIMAL_THRES",
                    "DUAL_THRES", "PAR", "REF", "ITERS", "STOP", "CONVERGE", "PROB", "STATUS_MASK")

    def tenant_items(self):
        """Every piadmm_obca_plan_get item a tenant record holds, by name: what `tenant_pack` takes."""
        names = self.TENANT_ITEMS
        if self.dual_par is not None:
            names += ("DUAL_S", "DUAL_D", "DUAL_S_PREV", "DUAL_D_PREV", "DUAL_PAR")
        if self.order:
            names += ("WORK",)
        if self._clock is not None:
            names += ("CLOCK", "WINDOW")
        if self._loop is not None:
            names += ("LOOP_PLANT", "LOOP_TAU", "LOOP_STREAMS", "LOOP_SEED")
            names += ("LOOP_NOISE",) if self._loop["noise"] else ()
            names += ("LOOP_DELAY",) if self._loop["delay"] else ()
        return {k: self.get(k) for k in names}

    def export_tenants(self, slots) -> bytes:
        """The running tenants in `slots` as one blob (piadmm_obca_tenant_export; a step boundary only):
        `tenant_unpack` reads it, `import_tenants` of any clocked fleet plan with the same n_ref,
        update_lamb_ij, law and order continues them bit for bit.  The plan is not changed."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        size = ctypes.c_int64()
        self._check(self._lib.piadmm_obca_tenant_export_bytes(self.batch._h, len(slots), ctypes.byref(size)))
        blob = np.zeros(size.value, np.uint8)
        self._check(self._lib.piadmm_obca_tenant_export(self.batch._h, len(slots), _lib.iptr(slots), blob.ctypes.data,
                                                      blob.nbytes))
        return blob.tobytes()

    def import_tenants(self, slots, tenants):
        """The tenants of a blob of `export_tenants` into `slots` (piadmm_obca_tenant_import; a clocked
        fleet plan at a step boundary, without a trace).  Nothing is zeroed: a slot holds what the
        tenant had, a retired tenant stays retired."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        blob = np.frombuffer(tenants, np.uint8) if isinstance(tenants, (bytes, bytearray, memoryview)) \
            else np.ascontiguousarray(tenants, np.uint8)
        self._check(self._lib.piadmm_obca_tenant_import(self.batch._h, len(slots), _lib.iptr(slots), blob.ctypes.data,
                                                      blob.nbytes))
        # a retired tenant stays retired; the tenant's reference is its own, not a spec's
        t = tenant_unpack(blob)
        self._mirror(slots, t["CLOCK"][:, :2], t["CLOCK"][:, 0] + N_HORZ <= t["CLOCK"][:, 1], t["STATE"], t["REF"],
                     t["PAR"], t["PROB"], t["PRIMAL_THRES"], t["DUAL_THRES"], [None] * len(slots))
        if self.dual_par is not None and len(self.dual_par) == self.n:
            self.dual_par[slots] = t["DUAL_PAR"]

    @classmethod
    def from_tenants(cls, batch, tenants, t_step=0, dual_par=None, on_stage=None):
        """A new clocked fleet plan on `batch` that holds exactly the tenants of a blob, in its order:
        opened through piadmm_obca_fleet_begin on the tenants' own rows and references, the clock
        attached, then the law and the order when the blob carries them, then the import.  dual_par:
        the one gains row the plan shares (None: a row per tenant, the blob's).  The plan counts its
        steps from t_step; the library opens it at min(t_step, n_ref - 8), which a clocked plan
        only shows in T_STEP."""
        t = tenant_unpack(tenants)
        m, par = t["m"], t["PAR"]
        kw = {name: par[:, j] for j, name in enumerate(FLEET_ROW)}
        pl = cls(batch, m, prob=[int(p) for p in t["PROB"]], t_step0=min(int(t_step), t["n_ref"] - N_HORZ),
                 primal_thres=t["PRIMAL_THRES"], dual_thres=t["DUAL_THRES"], update_lamb_ij=t["update_lamb_ij"],
                 ref_traj=t["REF"], state=t["STATE"], clock=True, on_stage=on_stage, **kw)
        if t["law"]:
            pl._set_dual_rows(t["DUAL_PAR"] if dual_par is None else np.asarray(dual_par, np.float64).reshape(1, DUAL_PAR))
        if t["order"]:
            pl.set_order()
        if t["loop"]:
            # a row per tenant of every kind the blob carries, the blob's; the seed and k0 of its header
            pl.set_loop(plant=t["LOOP_PLANT"], noise=t["LOOP_NOISE"] if t["loop"] & 2 else None,
                        delay=t["LOOP_DELAY"] if t["loop"] & 4 else None, streams=t["LOOP_STREAMS"],
                        seed=int(t["LOOP_SEED"][0]), k0=int(t["LOOP_SEED"][1]))
        pl.import_tenants(np.arange(m), tenants)
        pl.t_step = int(t_step)
        pl.record.state_record[0] = np.stack(pl.init_state)
        return pl

    def _shared_gains(self):
        """The one gains row a plan of more than one scenario shares, else None."""
        shared = self.dual_par is not None and len(self.dual_par) == 1 and self.n > 1
        return self.dual_par[0].copy() if shared else None

    def compact(self):
        """A new planner on the same batch that holds only the alive tenants, in ascending order of
        their slots (`compact_slots` on the result: where each was).  The batch holds one plan, so
        this planner ends as the new one opens; the tenants continue bit for bit."""
        alive = np.flatnonzero(self.alive())
        if not len(alive):
            raise ValueError("compact: no tenant alive")
        blob = self.export_tenants(alive)
        pl = type(self).from_tenants(self.batch, blob, t_step=int(self.get("T_STEP")[0]), dual_par=self._shared_gains(),
                                     on_stage=self.on_stage)
        pl.compact_slots = alive
        return pl

    def _trace_attached(self):
        try:
            self.trace_rows()
            return True
        except Exception:
            return False

    def save(self, path):
        """Checkpoint of the whole plan at a step boundary (piadmm.io.save_plan_checkpoint, one
        .npz): the blob of all n tenants, the plan cfg, T_STEP, which attachments were on and the
        shared gains row if any.  A trace is not saved (the file says one was attached; it stays
        readable here)."""
        cfg = {f: getattr(self.cfg, f) for f, _ in self.cfg._fields_}
        return io.save_plan_checkpoint(path, self.export_tenants(np.arange(self.n)), int(self.get("T_STEP")[0]), cfg,
                                       dict(fleet=self.fleet, clock=self._clock is not None,
                                            law=self.dual_par is not None, order=bool(self.order),
                                            trace=self._trace_attached()), self._shared_gains())

    @classmethod
    def load(cls, batch, path, on_stage=None):
        """The plan `save` wrote, reopened on `batch` (`from_tenants` at the saved T_STEP) so that its
        next steps are the uninterrupted run's, bit for bit.  It is a fleet plan whatever the saved
        one was; a plan saved without a clock gets its clock detached again."""
        ck = io.load_plan_checkpoint(path)
        pl = cls.from_tenants(batch, ck["tenants"], t_step=ck["t_step"], dual_par=ck["dual_par"], on_stage=on_stage)
        if not ck["attached"]["clock"] and pl.alive().all():
            pl.clear_clock()
        return pl

    def _set_dual_rows(self, rows):
        rows = np.ascontiguousarray(rows, np.float64).reshape(-1, DUAL_PAR)
        self._check(self._lib.piadmm_obca_dual_plan(self.batch._h, _lib.dptr(rows), rows.shape[0]))
        self.dual_par = rows

    def set_order(self, work_init=None):
        """Attach the longest-first order (piadmm_obca_order_plan; a step boundary only), its record
        zero or seeded with work_init (n x 2: Q, I per scenario)."""
        if work_init is not None:
            work_init = np.ascontiguousarray(work_init, np.int32)
            assert work_init.shape == (self.n, 2), work_init.shape
        self._check(self._lib.piadmm_obca_order_plan(self.batch._h, 1, _lib.iptr(work_init)))
        self.order = True

    def clear_order(self):
        """Detach the order: every list is ascending again (a step boundary only)."""
        self._check(self._lib.piadmm_obca_order_plan(self.batch._h, 0, None))
        self.order = False

    def work(self):
        """The order's record (Q, I) per scenario, n x 2 (PLAN_GET WORK)."""
        return self.get("WORK")

    def _check(self, rc):
        if rc != 0:
            msg = self._lib.piadmm_obca_last_error(self.batch._h)
            err = _lib.PiadmmError(f"libpiadmm error {rc}: {msg.decode() if msg else ''}")
            err.code = rc
            raise err

    def set_dual(self, **dual):
        """Attach the PI anti-windup dual law (piadmm_obca_dual_plan; a step boundary only): kP, kI,
        windup_sat, d_gain, windup, each one value or one per scenario.  `dual_par` keeps the rows."""
        rows = dual_rows(self.n, dual)
        self._check(self._lib.piadmm_obca_dual_plan(self.batch._h, _lib.dptr(rows), rows.shape[0]))
        self.dual_par = rows

    def clear_dual(self):
        """Detach the law: the plan runs the plain lambda_update again (a step boundary only)."""
        self._check(self._lib.piadmm_obca_dual_plan(self.batch._h, None, 0))
        self.dual_par = None

    def counts(self):
        """(scenarios submitted to the last iterate, scenarios still active, iterates run in the open step)."""
        c = np.zeros(3, np.int32)
        self._check(self._lib.piadmm_obca_plan_get(self.batch._h, PLAN_GET["COUNTS"][0], c.ctypes.data, c.nbytes))
        return int(c[0]), int(c[1]), int(c[2])

    def get(self, what):
        """One item of the resident plan (include/piadmm.h, piadmm_obca_plan_get), shaped: a name of
        PLAN_GET, of NOISE_GET, of DELAY_GET or of LOOP_GET."""
        code, dt = _GET[what]
        out = np.zeros(self._shape(what), dt)
        self._check(self._lib.piadmm_obca_plan_get(self.batch._h, code, out.ctypes.data, out.nbytes))
        return out

    def _shape(self, what):
        """The shape of item `what` of `get`: m = the scenarios of the last iterate (a PLAN_GET item
        reads the counts first), rows of an attachment = what the planner handed it (1 without one)."""
        n, m = self.n, (self.counts()[0] if what in PLAN_GET and what != "COUNTS" else 0)
        rows = n if self.fleet else 1
        lp = self._loop or dict(plant=1, noise=1, delay=1)

        def held(attached):
            return 1 if attached is None else len(attached[0])
        return {"STATE": (n, PLAN_STATE), "STATE_PREV": (n, PLAN_STATE), "CTRL": (n, 2, NT * NU),
                "CTRL_PREV": (n, 2, NT * NU), "X": (n, 2, N_HORZ, NX), "ITERS": (n,), "ACTIVE": (m,),
                "PRIMAL": (n,), "DUAL": (n,), "STOP": (n,), "CONVERGE": (n,), "LOCAL_REC": (2 * m, REC),
                "LOCAL_OUT": (2 * m, OUT), "LOCAL_IST": (2 * m, 3), "EDGE_REC": (m, EDGE_REC),
                "EDGE_OUT": (m, EDGE_OUT), "EDGE_IST": (m, NT, 3), "T_STEP": (1,), "LAMBDA": (n, 2, NT, 9),
                "COUNTS": (3,), "STATUS_MASK": (n, 2), "REF": (rows, 2, self.n_ref, NX),
                "PAR": (rows, FLEET_PAR), "DUAL_S": (n, 2, NT, 9), "DUAL_D": (n, 2, NT, 9),
                "DUAL_PAR": (1 if self.dual_par is None else len(self.dual_par), DUAL_PAR), "WORK": (n, 2),
                "CLOCK": (n, 3), "WINDOW": (n, 2, N_HORZ, NX), "PRIMAL_THRES": (n,), "DUAL_THRES": (n,),
                "PROB": (n,), "DUAL_S_PREV": (n, 2, NT, 9), "DUAL_D_PREV": (n, 2, NT, 9),
                "FEEDBACK_PAR": (held(self._feedback), FEEDBACK_PAR), "FEEDBACK_STEPS": (1,),
                "NOISE_PAR": (held(self._noise), NOISE_PAR), "NOISE_STREAMS": (n,), "NOISE_SEED": (2,),
                "DELAY_PAR": (held(self._delay), DELAY_PAR), "DELAY_TAU": (n, 2), "DELAY_STREAMS": (n,),
                "DELAY_SEED": (3,),
                "LOOP_PLANT": (lp["plant"], FEEDBACK_PAR), "LOOP_NOISE": (lp["noise"] or 1, NOISE_PAR),
                "LOOP_DELAY": (lp["delay"] or 1, DELAY_PAR), "LOOP_TAU": (n, 2), "LOOP_STREAMS": (n,),
                "LOOP_SEED": (3,)}[what]

    def iterate(self):
        """One ADMM iterate of the open MPC step; the number of scenarios still active."""
        left = ctypes.c_int32()
        self._check(self._lib.piadmm_obca_plan_iterate(self.batch._h, ctypes.byref(left)))
        return left.value

    def _tick(self, steps=1):
        """The host's copy of the clocks after `steps` closed steps (the record is deterministic)."""
        for _ in range(steps if self._clock is not None else 0):
            self._clock = clock_tick(self._clock, self._clock[:, 2])

    def shift(self):
        self._check(self._lib.piadmm_obca_plan_shift(self.batch._h))
        self._tick()

    def close(self):
        """End the plan (the batch stays usable after its next upload)."""
        if self.batch._h:
            self._lib.piadmm_obca_plan_end(self.batch._h)

    def _close_step(self, iters, status):
        if self._clock is None and self._feedback is None:      # the loop needs a clock: it reads STATE below
            X = self.get("X")
            self.init_state = [X[s, :, 1].copy() for s in range(self.n)]
        else:
            # a retired scenario's init_state is frozen, an admitted one's X is zero until it runs;
            # with feedback init_state is the state the vehicle reached, not X[1]
            st = self.get("STATE")
            self.init_state = [unpack_state(st[s])[1] for s in range(self.n)]
        self.record.state_record.append(np.stack(self.init_state))
        self.record.iter_num_record.append(np.asarray(iters, int))
        self.record.lambda_record.append(self.get("LAMBDA"))
        self.record.status_record.extend(status)
        self.t_step += 1

    def step(self):
        """One MPC step of every scenario."""
        if self.on_stage is not None:
            return self._step_staged()
        iters = np.zeros(self.n, np.int32)
        self._check(self._lib.piadmm_obca_plan_step(self.batch._h, _lib.iptr(iters)))
        self._tick()
        mask = self.get("STATUS_MASK")
        self._close_step(iters, [dict(t_step=self.t_step, iters=iters.copy(), local_status_mask=mask[:, 0].copy(),
                                      edge_status_mask=mask[:, 1].copy())])

    def _step_staged(self):
        n = self.n
        status = []
        left, i_iter = int(self.alive().sum()), 0
        while left:
            i_iter += 1
            before = self.get("STATE")
            ctrl_prev = self.get("CTRL_PREV")
            left = self.iterate()
            active = [int(s) for s in self.get("ACTIVE")]
            after = self.get("STATE")
            recs = self.get("LOCAL_REC")
            res = OBCAResult(self.get("LOCAL_OUT"), self.get("LOCAL_IST"))
            self.on_stage("local", dict(recs=recs, scenarios=list(active), i_iter=i_iter, t_step=self.t_step),
                          dict(result=res))
            fullx = [[res.bar_fullx(2 * k + v) for v in (0, 1)] for k in range(len(active))]
            bar_in = [unpack_state(before[s])[0] for s in active]
            # the exchange leaves Z_bar and lamb_bar as they were; the edge answer replaces them later
            bar_ex = []
            for k, s in enumerate(active):
                b = unpack_state(after[s])[0]
                b["Z_bar"], b["lamb_bar"] = bar_in[k]["Z_bar"].copy(), bar_in[k]["lamb_bar"].copy()
                bar_ex.append(b)
            self.on_stage("exchange", dict(bar=bar_in, fullx=fullx, scenarios=list(active)), dict(bar=bar_ex))
            conv = [bool(c) for c in self.get("CONVERGE")[active]]
            self.on_stage("converge", dict(bar=bar_ex), dict(if_converge=conv))
            erecs = self.get("EDGE_REC")
            eres = OBCAEdgeResult(self.get("EDGE_OUT"), self.get("EDGE_IST"))
            self.on_stage("edge", dict(recs=erecs, scenarios=list(active)), dict(result=eres))
            status.append(dict(t_step=self.t_step, i_iter=i_iter, scenarios=list(active), local_status=res.status.copy(),
                               edge_status=eres.status.copy(), if_converge=conv))
            ctrl = self.get("CTRL")
            self.on_stage("residual",
                          dict(ctrl=[ctrl[s] for s in active], ctrl_prev=[ctrl_prev[s] for s in active],
                               lamb_bar=[unpack_state(after[s])[0]["lamb_bar"] for s in active],
                               lamb_bar_prev=[b["lamb_bar"] for b in bar_in], i_iter=i_iter, scenarios=list(active)),
                          dict(primal=self.get("PRIMAL")[active], dual=self.get("DUAL")[active],
                               stop=self.get("STOP")[active].astype(bool)))
        iters = self.get("ITERS")
        frozen = self.get("STATE_PREV")
        X = self.get("X")
        self.shift()
        nxt = self.get("STATE")
        self.on_stage("shift", dict(bar_prev=[unpack_state(frozen[s])[0] for s in range(n)],
                                    X=[[X[s, 0], X[s, 1]] for s in range(n)], iters=iters.astype(int)),
                      dict(bar_next=[unpack_state(nxt[s])[0] for s in range(n)],
                           init_state=[unpack_state(nxt[s])[1] for s in range(n)]))
        self._close_step(iters, status)

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            if not self.alive().any():
                break
            self.step()
        return self.record

    def steps_left(self):
        """The steps the longest-lived scenario has left (None without a clock: the plan's reference
        decides)."""
        if self._clock is None:
            return None
        c = self._clock[self._clock[:, 2] != 0]
        return int((c[:, 1] - N_HORZ - c[:, 0] + 1).max()) if len(c) else 0

    def trace_begin(self, cap_steps, keep_lambda=True):
        """Attach a device-side run record of capacity cap_steps to the plan (a step boundary only)."""
        self._check(self._lib.piadmm_obca_trace_begin(self.batch._h, int(cap_steps),
                                                      TRACE_LAMBDA if keep_lambda else 0))
        self._trace_lambda = bool(keep_lambda)

    def trace_run(self, n_steps):
        """n_steps MPC steps on the device, recorded; the number completed."""
        done = ctypes.c_int32()
        rc = self._lib.piadmm_obca_trace_run(self.batch._h, int(n_steps), ctypes.byref(done))
        self._tick(done.value)
        self._check(rc)
        return done.value

    def trace_rows(self):
        r = np.zeros(1, np.int32)
        self._check(self._lib.piadmm_obca_trace_get(self.batch._h, TRACE_GET["ROWS"][0], r.ctypes.data, r.nbytes))
        return int(r[0])

    def trace_get(self, what):
        """One item of the attached trace (include/piadmm.h, piadmm_obca_trace_get), shaped."""
        code, dt = TRACE_GET[what]
        n, R = self.n, (self.trace_rows() if what not in ("ROWS", "SUMMARY") else 0)
        shape = {"STATES": (R + 1, n, 2, NX), "CLEARANCE": (R + 1, n, 2), "ITERS": (R, n), "STATUS_MASK": (R, n, 2),
                 "PRIMAL": (R, n), "DUAL": (R, n), "LAMBDA": (R, n, 2, NT, 9), "SUMMARY": (n, 4), "ROWS": (1,)}[what]
        out = np.zeros(shape, dt)
        self._check(self._lib.piadmm_obca_trace_get(self.batch._h, code, out.ctypes.data, out.nbytes))
        return out

    def trace_end(self):
        self._check(self._lib.piadmm_obca_trace_end(self.batch._h))

    def trace_stats(self, edges, worst=1) -> OBCAFleetStats:
        """The fleet statistics of the attached trace, reduced on the device in place
        (piadmm_obca_stats_trace): only the results come back.  `fleet_stats_host` on the arrays
        `trace_get` returns is the same statement."""
        def call(*a):
            return self._lib.piadmm_obca_stats_trace(self.batch._h, *a)
        # without a trace the call itself says so: R only sizes the result arrays
        r = np.zeros(1, np.int32)
        got = self._lib.piadmm_obca_trace_get(self.batch._h, TRACE_GET["ROWS"][0], r.ctypes.data, r.nbytes)
        rc, out = _stats_call(call, self.n, int(r[0]) if got == 0 else 0, edges, worst)
        self._check(rc)
        return out

    def trace_gather_bytes(self, m):
        size = ctypes.c_int64()
        self._check(self._lib.piadmm_obca_gather_trace_bytes(self.batch._h, int(m), ctypes.byref(size)))
        return int(size.value)

    def trace_gather(self, slots, nbytes=None):
        """Every row of the scenarios `slots` (distinct, any order) of the attached trace, gathered on
        the device (piadmm_obca_gather_trace): name -> array with column k = scenario slots[k], as
        `trace_gather_unpack` shapes them.  nbytes: the blob's size, when the caller knows better."""
        slots = np.ascontiguousarray(slots, np.int32).reshape(-1)
        m = len(slots)
        size = self.trace_gather_bytes(m) if nbytes is None else int(nbytes)
        blob = np.zeros(max(size, 1), np.uint8)
        self._check(self._lib.piadmm_obca_gather_trace(self.batch._h, m, _lib.iptr(slots), blob.ctypes.data, size))
        return trace_gather_unpack(blob[:size], self.trace_rows(), m, getattr(self, "_trace_lambda", None))

    def trace_worst(self, edges, K):
        """(statistics, the gathered record of the K worst scenarios by plain minimum clearance)."""
        st = self.trace_stats(edges, worst=K)
        return st, self.trace_gather(st.worst)

    # -- the tenant ledger (piadmm_obca_ledger_begin): a record per tenant that survives retirement and admission --
    def ledger_begin(self, cap_tenants, flags=0):
        """Attach a ledger of cap_tenants records (a clocked plan at a step boundary, without a trace):
        every alive slot's tenant takes its slot number as its id, the id counter starts at n."""
        self._check(self._lib.piadmm_obca_ledger_begin(self.batch._h, int(cap_tenants), int(flags)))

    def _ledger_get(self, what, count):
        code, dt = LEDGER_GET[what]
        out = np.zeros(count, dt)
        self._check(self._lib.piadmm_obca_ledger_get(self.batch._h, code, out.ctypes.data, out.nbytes))
        return out

    def ledger_count(self):
        return int(self._ledger_get("COUNT", 1)[0])

    def ledger_next_id(self):
        return int(self._ledger_get("NEXT_ID", 1)[0])

    def ledger_records(self):
        """The appended records, in the order of appending (`ledger_unpack` of the RECORDS item)."""
        return ledger_unpack(self._ledger_get("RECORDS", self.ledger_count() * LEDGER_REC))

    def ledger_running(self):
        """The open record of every slot (the RUNNING item): reason 0, id -1 where the slot holds no tenant."""
        return ledger_unpack(self._ledger_get("RUNNING", self.n * LEDGER_REC))

    def ledger_clear(self):
        """count = 0, so that a service drains the records and goes on; ids keep counting."""
        self._check(self._lib.piadmm_obca_ledger_clear(self.batch._h))

    def ledger_stats(self, edges, worst=1) -> OBCAFleetStats:
        """The statistics of the appended records, reduced on the device in place
        (piadmm_obca_ledger_stats): `worst` holds positions in the ledger; the rows' results of the
        R = 1 view are not brought back (row_min, row_arg, row_below stay zero).  `ledger_stats_host`
        on `ledger_records()` is the same statement."""
        def call(edges_p, B, K, st, hist, row_min, row_arg, row_below, worst_p):
            return self._lib.piadmm_obca_ledger_stats(self.batch._h, edges_p, B, K, st, hist, worst_p)
        rc, out = _stats_call(call, 0, 1, edges, worst)
        self._check(rc)
        return out

    def ledger_end(self):
        self._check(self._lib.piadmm_obca_ledger_end(self.batch._h))

    def trace(self, keep_lambda=True):
        """The attached trace as an OBCATrace."""
        summary = self.trace_get("SUMMARY")
        return OBCATrace(states=self.trace_get("STATES"), clearance=self.trace_get("CLEARANCE"),
                         iters=self.trace_get("ITERS"), status_mask=self.trace_get("STATUS_MASK"),
                         primal=self.trace_get("PRIMAL"), dual=self.trace_get("DUAL"),
                         min_clearance=summary[:, 0].copy(), min_row=summary[:, 1].astype(np.int64),
                         min_clearance_tight=summary[:, 2].copy(), iters_sum=summary[:, 3].astype(np.int64),
                         lamb=self.trace_get("LAMBDA") if keep_lambda else None)

    def run_traced(self, n_steps, keep_lambda=True):
        """`run` with the record kept on the device: one piadmm_obca_trace_begin, one
        piadmm_obca_trace_run of n_steps MPC steps and the downloads at the end, instead of the
        per-step downloads of `step`.  Fills `record` as `run` does (status_record with the per-step
        entry of the un-staged `step`; lambda_record only with keep_lambda), advances t_step and
        init_state, and returns the OBCATrace with the clearances.  Staged stepping stays on `run`."""
        if self.on_stage is not None:
            raise ValueError("run_traced does not stage: use run() with on_stage")
        n_steps = int(n_steps)
        if self._clock is not None:
            n_steps = min(n_steps, self.steps_left())      # with nothing alive: an empty trace
        self.trace_begin(max(n_steps, 1), keep_lambda)
        if n_steps:
            self.trace_run(n_steps)
        tr = self.trace(keep_lambda)
        self.trace_end()
        for k in range(tr.iters.shape[0]):
            iters = tr.iters[k].copy()
            self.init_state = [tr.states[k + 1, s].copy() for s in range(self.n)]
            self.record.state_record.append(np.stack(self.init_state))
            self.record.iter_num_record.append(np.asarray(iters, int))
            if keep_lambda:
                self.record.lambda_record.append(tr.lamb[k].copy())
            self.record.status_record.append(dict(t_step=self.t_step, iters=iters.copy(),
                                                  local_status_mask=tr.status_mask[k, :, 0].copy(),
                                                  edge_status_mask=tr.status_mask[k, :, 1].copy()))
            self.t_step += 1
        return tr
