"""The consensus loop (decentralized_overtaking_ADMM.py:31-102) for many scenarios at once."""
import numpy as np

from .. import _lib
from .attach import clock_rows, clock_tick, dual_rows, lambda_update_pi, shift_dual
from .feedback import NOISE_K_MAX, delay_args, delay_tau, feedback_args, noise_args, noise_tape, propagate
from .ledger import LEDGER_ADMITTED, LEDGER_IMPORTED, LEDGER_RETIRED, OBCALedger
from .loop import loop_args, loop_draw
from .model import (DT, EDGE_WRITES_ITERATE, FLEET_ROW, N_HORZ, NT, NU, NX, _per_scenario, _spec, bar_state_update, check_converge,
                    edge_record, executed_path, iterate_next_state, local_record, ref_traj_gen, seeded_bar_state)
from .stats import OBCARunRecord
from .tenant import tenant_unpack, unpack_state


def _scenario_refs(pl, specs, ref_traj):
    """pl.specs, pl.ref_traj (the shared reference, None when each scenario has its own),
    pl.ref_traj_s (n x 2 x n_ref x 5, a broadcast view of a shared one) and pl.n_ref; returns
    (the references to upload, whether they are per scenario).  ref_traj: 2 x n_ref x 5 for all,
    or n x 2 x n_ref x 5; without it the references of `specs`."""
    n = pl.n
    pl.specs = None if specs is None else [_spec(sp) for sp in specs]
    assert pl.specs is None or len(pl.specs) == n
    if ref_traj is None and pl.specs is not None:
        ref = np.stack([np.stack(ref_traj_gen(sp)) for sp in pl.specs]) if n else np.zeros((0, 2, 51, NX))
        pl.ref_traj = None
    else:
        pl.ref_traj = ref_traj_gen() if ref_traj is None else ref_traj
        ref = np.stack([np.asarray(r_, np.float64) for r_ in pl.ref_traj])
        if ref.ndim == 4:
            pl.ref_traj = None
    ref = np.ascontiguousarray(ref, np.float64)
    each = ref.ndim == 4
    assert ref.shape[-3] == 2 and ref.shape[-1] == NX and (not each or ref.shape[0] == n), ref.shape
    pl.n_ref = ref.shape[-2]
    pl.ref_traj_s = ref if each else np.broadcast_to(ref, (n,) + ref.shape)
    return ref, each


def _spec_of(pl, s):
    return None if pl.specs is None else pl.specs[s]


def _planner_init(pl, batch, n_scenarios, prob, t_step0, primal_thres, dual_thres, update_lamb_ij, on_stage, specs,
                  ref_traj, clock, *, rho, min_dis, conv_thres, max_admm_iter, max_iter, round_decimals, start, **row):
    """The constructor statements the two planners share (row: the other FLEET_ROW arguments).  Returns (whether
    any was a sequence, what `_scenario_refs` returns, the clock's rows or None, the step each scenario starts at)."""
    pl.batch = batch
    pl.n = int(n_scenarios)
    pl.prob = [int(prob)] * pl.n if np.isscalar(prob) else [int(p) for p in prob]
    assert len(pl.prob) == pl.n
    pl.t_step = int(t_step0)
    pl.rho = float(rho) if np.ndim(rho) == 0 else None
    pl.min_dis = float(min_dis) if np.ndim(min_dis) == 0 else None
    pl.max_admm_iter = int(max_admm_iter) if np.ndim(max_admm_iter) == 0 else None
    pl.primal_thres = np.broadcast_to(np.asarray(primal_thres, np.float64), (pl.n,)).copy()
    pl.dual_thres = np.broadcast_to(np.asarray(dual_thres, np.float64), (pl.n,)).copy()
    pl.conv_thres = conv_thres if np.ndim(conv_thres) == 0 else None
    pl.round_decimals, pl.start, pl.max_iter = (v if np.ndim(v) == 0 else None for v in (round_decimals, start, max_iter))
    pl.update_lamb_ij = update_lamb_ij
    any_seq = _per_scenario(pl, pl.n, rho=rho, min_dis=min_dis, conv_thres=conv_thres, **row, max_admm_iter=max_admm_iter,
                            max_iter=max_iter, round_decimals=round_decimals, start=start)
    pl.on_stage = on_stage
    refs = _scenario_refs(pl, specs, ref_traj)
    # every scenario is seeded at the step it starts at: its own c0 with a clock
    rows = None if clock is None else clock_rows(pl.n, clock, pl.t_step, pl.n_ref)
    t0 = [pl.t_step] * pl.n if rows is None else [int(c) for c in rows[:, 0]]
    pl.init_state = [np.stack([executed_path(v, t0[s] * DT, _spec_of(pl, s)) for v in (0, 1)]) for s in range(pl.n)]
    return any_seq, refs, rows, t0


class OBCAPlanner:
    """The OBCA-ADMM overtaking planner on the GPU.  Per ADMM iterate, in the script's order: one
    local launch over all still-active scenarios x 2 vehicles (:49-63), bar_state_update (:66),
    check_converge (:67), one edge launch with the fused lambda_update (:71-79), the residuals
    (:82-85); a scenario stops at both residuals <= the thresholds or i_iter > max_admm_iter (:86)
    and is not resubmitted.  Then the horizon shift -- of the PREVIOUS iterate's bar_state, as :87
    is written -- and init_state = X[1] (:99).

    prob, primal_thres, dual_thres: one value or one per scenario.  update_lamb_ij: 0 leaves lamb_ij untouched (the
    commented-out :220), 1 takes each vehicle's local Lambda.  on_stage(name, inputs, outputs) sees
    every stage: "local", "exchange", "converge", "edge", "residual", "shift".

    Every parameter of FLEET_ROW is one value or one per scenario (`rho_s`, `min_dis_s`, ... keep
    the value of each scenario; the scalar attributes keep a scalar argument and are None for a
    sequence).  specs: one OvertakeSpec per scenario, giving its reference, init_state and seeded
    state; ref_traj: one reference (2 x n_ref x 5) or one per scenario (`ref_traj_s`).

    dual: None keeps lambda_update; dict(kP=, kI=, windup_sat=, d_gain=, windup=), each one value or
    one per scenario, replaces it by the PI anti-windup law (`lambda_update_pi`), the integrator
    shifted with the state (`shift_dual`).  OBCADevicePlanner takes the same argument.

    clock: None keeps the one step of all scenarios; n x 2 rows (c0, len), or True for everyone at
    t_step0 over the whole reference, gives every scenario its own step (`clock`, n x 3: c, len,
    alive, ticked by `clock_tick`): it is seeded at c0, reads its reference at c, and once
    c + 8 > len it is retired -- skipped by every later step, its state frozen, its stop iterate 0.

    feedback: None closes a step with init_state = X[1]; dict(par=, tape=) closes it through the
    plant instead (`propagate`): init_state = propagate(the closing step's init_state, the first
    control of the stopping local solution, par, tape[s][k]) with k the steps since the attachment.
    par: one plant row or n (`feedback_row`; None: the nominal plant), tape: n x cap x 2 x 5
    disturbance rows or None.  `measure` overwrites init_state with states measured outside.
    OBCADevicePlanner takes the same argument.  Not together with clock.

    noise: None, or dict(par=, streams=, seed=, k0=) on top of feedback: the disturbance of scenario
    s at the step k since the feedback's attachment is tape[s][k] (if any) plus the row
    `noise_tape` draws for stream streams[s] at step index k0 + k -- a pure function of (seed,
    stream, step index), so no tape is kept.  `set_noise` / `clear_noise` attach and detach it; a
    new `set_feedback` and `clear_feedback` drop it.  OBCADevicePlanner takes the same argument and
    draws the same disturbances (k_plan_noise).

    delay: None, or dict(par=, streams=, seed=, k0=, tape=): communication delay in the exchange.
    Vehicle v of scenario s sends, at every iterate of the step k since the attachment, the
    halfspaces and local_x of `stale_states(X, tau)` in place of its local states, with tau =
    `delay_tau`'s latency of stream streams[s] at step index k0 + k (tape n x cap x 2: recorded
    latencies added in front); what it keeps for itself (controls, X, init_state) is unchanged.
    `set_delay` / `clear_delay` attach and detach it; independent of feedback and noise, not together
    with clock.  OBCADevicePlanner takes the same argument (piadmm_obca_delay_plan).

    loop: None, or with clock= dict(plant=, noise=, delay=, streams=, seed=, k0=): the same closed loop
    under the per-scenario clocks, its step index each scenario's own clock c (`loop_draw`).  A step
    closes, for the scenarios it ran, with init_state = propagate(the closing step's init_state, the
    first control, plant[s], the noise row of stream streams[s] at step index k0 + c); with delay rows
    the open step's latency of an alive scenario is `delay_tau`'s at k0 + c (`loop_tau`), a retired
    one's stays.  OBCADevicePlanner takes the same argument (piadmm_obca_loop_plan).

    ledger: with clock=, True keeps the tenant ledger of piadmm_obca_ledger_begin in NumPy (`ledger`, an
    OBCALedger; `ledger_cap` bounds it): a record per tenant, opened at its clock and entry state, updated
    by every step it closes, appended when its clock retires it (reason 1) or `admit` / `import_tenants`
    replace it (2 / 3).  `set_ledger` / `clear_ledger` attach and detach it at a step boundary."""

    def __init__(self, batch, n_scenarios, prob=1, t_step0=0, rho=1.0, min_dis=0.1, max_admm_iter=50,
                 primal_thres=0.01, dual_thres=0.01, round_decimals=4, start=1, update_lamb_ij=0, max_iter=60,
                 conv_thres=0.1, on_stage=None, max_x=150.0, max_y=20.0, r=1e4, q=1e5, x_bound=1000.0,
                 mu_max=100000.0, g_max=1000.0, ref_traj=None, specs=None, dual=None, clock=None, feedback=None,
                 noise=None, delay=None, loop=None, ledger=False, ledger_cap=None):
        _, _, rows, t0 = _planner_init(
            self, batch, n_scenarios, prob, t_step0, primal_thres, dual_thres, update_lamb_ij,
            on_stage or (lambda name, inputs, outputs: None), specs, ref_traj, clock, rho=rho, min_dis=min_dis,
            conv_thres=conv_thres, max_x=max_x, max_y=max_y, r=r, q=q, x_bound=x_bound, mu_max=mu_max, g_max=g_max,
            max_admm_iter=max_admm_iter, max_iter=max_iter, round_decimals=round_decimals, start=start)
        self.clock = None
        if rows is not None:
            assert (rows[:, 0] >= 0).all() and (rows[:, 1] <= self.n_ref).all() \
                and (rows[:, 0] + N_HORZ <= rows[:, 1]).all(), rows
            self.clock = np.concatenate((rows, np.ones((self.n, 1), np.int32)), axis=1)
        self.bar_prev = [seeded_bar_state(t0[s], p, spec=_spec_of(self, s)) for s, p in enumerate(self.prob)]
        self.lamb_last = [np.zeros((2, NT, 9)) for _ in range(self.n)]
        # the PI anti-windup dual law (dual=dict(kP=, kI=, windup_sat=, d_gain=, windup=), each one
        # value or one per scenario): S = lamb_bar, D = 0, as piadmm_obca_dual_plan attaches it
        self.dual_par = None if dual is None else dual_rows(self.n, dual)
        if dual is not None:
            self.dual_S = [b["lamb_bar"].copy() for b in self.bar_prev]
            self.dual_D = [np.zeros((2, NT, 9)) for _ in range(self.n)]
        self.feedback = None
        self.noise = None
        if feedback is not None:
            self.set_feedback(**feedback)
        if noise is not None:
            self.set_noise(**noise)
        self.delay = None
        if delay is not None:
            self.set_delay(**delay)
        self.loop = None
        if loop is not None:
            self.set_loop(**loop)
        self.ledger = None
        if ledger:
            self.set_ledger(ledger_cap)
        self.record = OBCARunRecord()
        self.record.state_record.append(np.stack(self.init_state))

    def _stream(self, s):
        return -1 if self.loop is None else int(self.loop["streams"][s])

    def set_ledger(self, cap=None):
        """Attach the ledger (see the class; a clock must be attached, as piadmm_obca_ledger_begin
        refuses otherwise): every alive slot's tenant takes its slot number, the id counter starts at n."""
        if self.clock is None:
            err = _lib.PiadmmError("obca_ledger_begin: no clock attached")
            err.code = _lib.E_STATE
            raise err
        self.ledger = OBCALedger(self.n, cap)
        for s in range(self.n):
            if self.clock[s, 2]:
                self.ledger.open(s, s, int(self.clock[s, 0]), self.init_state[s], self.prob[s], self._stream(s))

    def clear_ledger(self):
        self.ledger = None

    def _replace(self, slots, reason, fill):
        """What an admission and an import share: the alive tenants of `slots` leave the ledger's open
        records in the order of `slots`, `fill(k, s)` puts the new tenant into slot s, and every new alive
        tenant takes the next id, in that order."""
        slots = [int(s) for s in slots]
        assert self.clock is not None and len(set(slots)) == len(slots)
        if self.ledger is not None:
            leaving = [s for s in slots if self.ledger.running[s]["id"] >= 0 and self.clock[s, 2]]
            if self.ledger.cap is not None and self.ledger.count + len(leaving) > self.ledger.cap:
                raise ValueError("ledger full")
            for s in leaving:
                self.ledger.close(s, reason, self.t_step, self._stream(s))
        self.bar_prev, self.init_state, self.prob = list(self.bar_prev), list(self.init_state), list(self.prob)
        if self.loop is not None:
            self.loop = dict(self.loop, streams=self.loop["streams"].copy())      # the caller's array stays as it is
        for k, s in enumerate(slots):
            fill(k, s)
        if self.loop is not None:
            self._loop_open()
        if self.ledger is not None:
            for s in slots:
                if self.clock[s, 2]:
                    self.ledger.admit(s, int(self.clock[s, 0]), self.init_state[s], self.prob[s], self._stream(s))
                else:
                    self.ledger.running[s]["id"] = -1

    def admit(self, slots, clock, specs=None, bar=None, init_state=None, ref=None, prob=None, streams=None):
        """New tenants into `slots` of the clocked planner, as OBCADevicePlanner.admit: clock m x 2 rows
        (c0, len); with specs= a missing ref is the spec's reference, a missing bar the state seeded at
        the tenant's c0 and a missing init_state the executed path there; ref m x 2 x n_ref x 5, prob m,
        streams m stream ids of the loop -- None keeps what the slot has."""
        clock = np.asarray(clock, np.int32).reshape(len(slots), 2)
        specs = None if specs is None else [_spec(sp) for sp in specs]
        self.ref_traj_s = np.array(self.ref_traj_s)
        self.ref_traj = None

        def fill(k, s):
            c0, sp = int(clock[k, 0]), None if specs is None else specs[k]
            if prob is not None:
                self.prob[s] = int(np.broadcast_to(prob, (len(slots),))[k])
            if ref is not None or sp is not None:
                self.ref_traj_s[s] = np.stack(ref_traj_gen(sp)) if ref is None else ref[k]
            if bar is not None or sp is not None:
                self.bar_prev[s] = seeded_bar_state(c0, self.prob[s], spec=sp) if bar is None else self._copy(bar[k])
            if init_state is not None or sp is not None:
                self.init_state[s] = (np.stack([executed_path(v, c0 * DT, sp) for v in (0, 1)]) if init_state is None
                                      else np.array(init_state[k], np.float64))
            if self.specs is not None and sp is not None:
                self.specs[s] = sp
            self.lamb_last[s] = np.zeros((2, NT, 9))
            if self.dual_par is not None:
                self.dual_S[s], self.dual_D[s] = self.bar_prev[s]["lamb_bar"].copy(), np.zeros((2, NT, 9))
            if streams is not None:
                self.loop["streams"][s] = int(streams[k])
            self.clock[s] = (c0, int(clock[k, 1]), 1)
        self._replace(slots, LEDGER_ADMITTED, fill)

    def import_tenants(self, slots, tenants):
        """The tenants of a blob of OBCADevicePlanner.export_tenants into `slots`: the state, the
        reference, prob, the thresholds, the parameter row, the clock and, with the loop, the stream id
        of each; a retired tenant stays retired.  The dual law's integrator and the loop's rows do not travel here."""
        t = tenant_unpack(tenants)
        assert t["m"] == len(slots) and t["n_ref"] == self.n_ref
        self.ref_traj_s = np.array(self.ref_traj_s)
        self.ref_traj = None

        def fill(k, s):
            self.bar_prev[s], self.init_state[s] = unpack_state(t["STATE"][k])
            self.prob[s] = int(t["PROB"][k])
            self.ref_traj_s[s] = t["REF"][k]
            self.primal_thres[s], self.dual_thres[s] = t["PRIMAL_THRES"][k], t["DUAL_THRES"][k]
            for j, name in enumerate(FLEET_ROW):
                col = getattr(self, name + "_s").astype(np.float64)
                col[s] = t["PAR"][k, j]
                setattr(self, name + "_s", col)
            self.lamb_last[s] = t["LAMBDA"][k].reshape(2, NT, 9).copy()
            if self.loop is not None and t["loop"]:
                self.loop["streams"][s] = int(t["LOOP_STREAMS"][k])
            c, ln = int(t["CLOCK"][k, 0]), int(t["CLOCK"][k, 1])
            self.clock[s] = (c, ln, 1 if c + N_HORZ <= ln else 0)
        self._replace(slots, LEDGER_IMPORTED, fill)

    def set_loop(self, plant=None, noise=None, delay=None, streams=None, seed=0, k0=0):
        """Attach the loop (see the class; a clock must be attached and neither feedback nor delay, as
        piadmm_obca_loop_plan refuses otherwise)."""
        loop = loop_args(self.n, plant, noise, delay, streams, seed, k0)
        why = ("feedback is attached" if self.feedback is not None else "the delay is attached" if self.delay is not None
               else "no clock attached" if self.clock is None else None)
        if why is not None:
            err = _lib.PiadmmError(f"obca_loop_plan: {why}")
            err.code = _lib.E_STATE
            raise err
        self.loop = loop
        self._loop_tau = np.zeros((self.n, 2))
        self._loop_open()

    def clear_loop(self):
        self.loop = None

    def _loop_open(self):
        """The open step's latencies of the alive scenarios at their clocks; a retired one's stay."""
        if self.loop["delay"] is not None:
            alive = self.clock[:, 2] != 0
            tau = loop_draw(self.n, np.where(alive, self.clock[:, 0], 0), None, self.loop["delay"], self.loop["streams"],
                            self.loop["seed"], self.loop["k0"])[1]
            self._loop_tau[alive] = tau[alive]

    def loop_tau(self):
        """The open step's latencies, n x 2 (the LOOP_TAU item of OBCADevicePlanner.get)."""
        assert self.loop is not None, "no loop attached"
        return self._loop_tau.copy()

    def set_delay(self, par=None, streams=None, seed=0, k0=0, tape=None):
        """Attach the communication delay (see the class): from the next step on the exchange is
        stale.  The step count starts again."""
        delay = delay_args(self.n, par, streams, seed, k0, tape)
        if self.clock is not None:
            err = _lib.PiadmmError("obca_delay_plan: a clock is attached (obca_clock_plan: the delay counts the "
                                   "plan's steps, not per-scenario clocks)")
            err.code = _lib.E_STATE
            raise err
        self.delay = delay
        self._delay_steps = 0

    def clear_delay(self):
        self.delay = None

    def delay_tau(self):
        """The open step's latencies, n x 2 (the DELAY_TAU item of OBCADevicePlanner.get)."""
        assert self.delay is not None, "no delay attached"
        par, streams, seed, k0, tape = self.delay
        k = self._delay_steps
        assert tape is None or k < tape.shape[1], "latency tape exhausted"
        assert k0 + k < NOISE_K_MAX, "delay step index exhausted"
        return delay_tau(self.n, 1, par, streams, seed, k0 + k, None if tape is None else tape[:, k:k + 1])[:, 0]

    def set_feedback(self, par=None, tape=None):
        """Attach the plant (see the class): from the next step on a step closes through `propagate`.
        The step count starts again, so an attached noise is dropped."""
        assert self.clock is None, "feedback and clock do not go together"
        self.feedback = feedback_args(self.n, dict(par=par, tape=tape))
        self._feedback_steps = 0
        self.noise = None

    def clear_feedback(self):
        self.feedback = None
        self.noise = None

    def set_noise(self, par=None, streams=None, seed=0, k0=0):
        """Attach the noise (see the class; feedback must be attached, as piadmm_obca_noise_plan
        refuses without it)."""
        noise = noise_args(self.n, par, streams, seed, k0)
        if self.feedback is None:
            err = _lib.PiadmmError("obca_noise_plan: no feedback attached (obca_feedback_plan: the noise enters "
                                   "through the plant step)")
            err.code = _lib.E_STATE
            raise err
        self.noise = noise

    def clear_noise(self):
        self.noise = None

    def feedback_steps(self):
        """The steps closed since the attachment."""
        assert self.feedback is not None, "no feedback attached"
        return self._feedback_steps

    def measure(self, slots, states):
        """init_state of the scenarios `slots` = the measured `states` (m x 2 x 5); nothing else changes."""
        states = np.asarray(states, np.float64)
        assert states.shape == (len(slots), 2, NX) and np.isfinite(states).all(), states.shape
        self.init_state = list(self.init_state)
        for k, s in enumerate(slots):
            self.init_state[int(s)] = states[k].copy()

    @staticmethod
    def _copy(bar):
        return {k: v.copy() for k, v in bar.items()}

    def step(self):
        """One MPC step of every scenario."""
        n = self.n
        if self.feedback is not None and self.feedback[1] is not None:
            assert self._feedback_steps < self.feedback[1].shape[1], "disturbance tape exhausted"
        if self.clock is None:
            assert self.t_step + N_HORZ <= self.n_ref, "reference exhausted"
            ran = list(range(n))
            t_of = [self.t_step] * n
        else:
            # every scenario at its own step; the retired ones are skipped
            ran = [s for s in range(n) if self.clock[s, 2]]
            assert ran, "no scenario alive"
            t_of = [int(c) for c in self.clock[:, 0]]
        if self.ledger is not None and self.ledger.cap is not None:
            # before anything changes, as piadmm_obca_plan_step refuses: every tenant the tick retires needs a place
            out = sum(1 for s in ran if self.clock[s, 0] + 1 + N_HORZ > self.clock[s, 1])
            if self.ledger.count + out > self.ledger.cap:
                raise ValueError("ledger full")
        tau = None if self.delay is None else self.delay_tau()
        if self.loop is not None:
            assert (self.loop["k0"] + self.clock[ran, 0] + 1 < NOISE_K_MAX).all(), "loop step index exhausted"
            tau = self.loop_tau() if self.loop["delay"] is not None else None
        bar = [self._copy(b) for b in self.bar_prev]
        bar_prev = [self._copy(b) for b in self.bar_prev]
        x0_step = [np.array(x, np.float64) for x in self.init_state]
        ctrl_prev = [np.zeros((2, NT * NU)) for _ in range(n)]
        X = [None] * n
        U0 = [None] * n
        iters = np.zeros(n, int)
        shift_in = [None] * n
        masks, resid = np.zeros((n, 2), np.int64), np.zeros((n, 2))      # what the ledger keeps of the step
        active = list(ran)
        i_iter = 0
        while active:
            i_iter += 1
            # ---- vehicle side: one launch, scenarios x vehicles ----
            recs = np.ascontiguousarray(np.stack([
                local_record(bar[s], v, t_of[s], self.init_state[s][v], self.ref_traj_s[s], rho=self.rho_s[s],
                             min_dis=self.min_dis_s[s], prob=self.prob[s], max_x=self.max_x_s[s],
                             max_y=self.max_y_s[s], r=self.r_s[s], q=self.q_s[s], max_iter=self.max_iter_s[s])
                for s in active for v in (0, 1)]))
            res = self.batch.solve(recs)
            self.on_stage("local", dict(recs=recs, scenarios=list(active), i_iter=i_iter, t_step=self.t_step),
                          dict(result=res))
            fullx = [[res.bar_fullx(2 * k + v) for v in (0, 1)] for k in range(len(active))]
            ctrl = [np.stack([np.append(res.U[2 * k + v][:, 0], res.U[2 * k + v][:, 1]) for v in (0, 1)])
                    for k in range(len(active))]
            for k, s in enumerate(active):
                X[s] = [res.X[2 * k].copy(), res.X[2 * k + 1].copy()]
                U0[s] = np.stack([res.U[2 * k + v][0] for v in (0, 1)])
            # ---- information exchange ----
            before = [bar[s] for s in active]
            for k, s in enumerate(active):
                if tau is None:
                    bar[s] = bar_state_update(bar[s], fullx[k], prob=self.prob[s])
                else:
                    bar[s] = bar_state_update(bar[s], fullx[k], prob=self.prob[s], tau=tau[s],
                                              fullX=[res.X[2 * k + v] for v in (0, 1)])
                if self.update_lamb_ij:
                    bar[s]["lamb_ij"] = np.stack([fullx[k][v][:, 5:] for v in (0, 1)])
            self.on_stage("exchange", dict(bar=before, fullx=fullx, scenarios=list(active)),
                          dict(bar=[self._copy(bar[s]) for s in active]))
            conv = [check_converge(bar[s], self.conv_thres_s[s], self.min_dis_s[s]) for s in active]
            self.on_stage("converge", dict(bar=[self._copy(bar[s]) for s in active]), dict(if_converge=conv))
            # ---- RSU side: one launch, the dual update fused ----
            erecs = np.ascontiguousarray(np.stack([
                edge_record(bar[s], rho=self.rho_s[s], min_dis=self.min_dis_s[s], prob=self.prob[s],
                            max_iter=self.max_iter_s[s], round_decimals=self.round_decimals_s[s],
                            start=self.start_s[s], x_bound=self.x_bound_s[s], mu_max=self.mu_max_s[s],
                            g_max=self.g_max_s[s]) for s in active]))
            eres = self.batch.solve_edge(erecs)
            self.on_stage("edge", dict(recs=erecs, scenarios=list(active)), dict(result=eres))
            lamb_prev = [bar[s]["lamb_bar"].copy() for s in active]
            if self.dual_par is None:
                for k, s in enumerate(active):
                    bar[s]["Z_bar"] = eres.Z_bar[k].copy()
                    bar[s]["lamb_bar"] = eres.lamb_bar[k].copy()
            else:
                # the law instead of the fused update: the integrator before this iterate is the
                # one the previous iterate's bar_state corresponds to (B16)
                dual_before = {s: (self.dual_S[s], self.dual_D[s]) for s in active}
                dres_pi = np.zeros((len(active), NT))
                for k, s in enumerate(active):
                    bar[s]["Z_bar"] = eres.Z_bar[k].copy()
                    wrote = [int(c) in EDGE_WRITES_ITERATE for c in eres.status[k]]
                    bar[s], self.dual_S[s], self.dual_D[s], dres_pi[k] = lambda_update_pi(
                        bar[s], self.dual_S[s], self.dual_D[s], self.dual_par[s % len(self.dual_par)], wrote)
            self.record.status_record.append(dict(t_step=self.t_step, i_iter=i_iter, scenarios=list(active),
                                                  local_status=res.status.copy(), edge_status=eres.status.copy(),
                                                  if_converge=conv))
            # ---- residuals (:82-86) ----
            primal = np.array([np.abs(ctrl[k] - ctrl_prev[s]).sum() for k, s in enumerate(active)])
            if self.dual_par is None:
                dual = eres.dual_residual()
            else:
                dual = np.zeros(len(active))
                for t in range(NT):
                    dual = dual + dres_pi[:, t]
            stop = ((primal <= self.primal_thres[active]) & (dual <= self.dual_thres[active])) \
                | (i_iter > self.max_admm_iter_s[active])
            self.on_stage("residual",
                          dict(ctrl=ctrl, ctrl_prev=[ctrl_prev[s] for s in active],
                               lamb_bar=[bar[s]["lamb_bar"] for s in active], lamb_bar_prev=lamb_prev, i_iter=i_iter,
                               scenarios=list(active)),
                          dict(primal=primal, dual=dual, stop=stop))
            nxt = []
            for k, s in enumerate(active):
                for v in (0, 1):
                    masks[s, 0] |= 1 << int(res.status[2 * k + v])
                for c in np.asarray(eres.status[k]).reshape(-1):
                    masks[s, 1] |= 1 << int(c)
                if stop[k]:
                    iters[s] = i_iter
                    resid[s] = primal[k], dual[k]
                    shift_in[s] = bar_prev[s]           # :87: the previous iterate's bar_state (B16)
                    if self.dual_par is not None:
                        self.dual_S[s], self.dual_D[s] = dual_before[s]
                else:
                    bar_prev[s] = self._copy(bar[s])
                    ctrl_prev[s] = ctrl[k]
                    nxt.append(s)
            active = nxt
        # ---- next time step (:87, :99-103): of the scenarios this step ran ----
        self.bar_prev, self.init_state = list(self.bar_prev), list(self.init_state)
        for s in ran:
            self.bar_prev[s] = iterate_next_state(shift_in[s])
            if self.dual_par is not None:
                self.dual_S[s], self.dual_D[s] = shift_dual(self.dual_S[s], self.dual_D[s])
            self.init_state[s] = np.stack([X[s][0][1], X[s][1][1]])
            self.lamb_last[s] = bar[s]["lamb_bar"]
        if self.feedback is not None:
            # the vehicle instead of the prediction: from the closing step's init_state under the
            # stopping solution's first control (every scenario ran: no clock with feedback)
            par, tape = self.feedback
            w = None if tape is None else tape[:, self._feedback_steps]
            if self.noise is not None:
                # the step's row of every stream, the tape's row in front
                zpar, streams, seed, k0 = self.noise
                wn = noise_tape(n, 1, zpar, streams, seed, k0 + self._feedback_steps)[:, 0]
                w = wn if w is None else w + wn
            nxt = propagate(np.stack(x0_step), np.stack(U0), par, w)
            self.init_state = [nxt[s] for s in range(n)]
            self._feedback_steps += 1
        if self.delay is not None:
            self._delay_steps += 1
        if self.loop is not None:
            # the same, for the scenarios the step ran, each at its own clock (before the tick)
            lp = self.loop
            for s in ran:
                w = None if lp["noise"] is None else loop_draw(1, self.clock[s:s + 1], lp["noise"][s % len(lp["noise"])], None,
                                                               lp["streams"][s:s + 1], lp["seed"], lp["k0"])[0]
                self.init_state[s] = propagate(x0_step[s][None], U0[s][None], lp["plant"][s % len(lp["plant"])], w)[0]
        self.on_stage("shift", dict(bar_prev=shift_in, X=X, iters=iters.copy()), dict(bar_next=self.bar_prev, init_state=self.init_state))
        self.record.state_record.append(np.stack(self.init_state))
        self.record.iter_num_record.append(iters)
        self.record.lambda_record.append(np.stack(self.lamb_last))
        if self.ledger is not None:
            # the open records take the step at the clock of the new state; the tick's retirees leave, ascending
            out = [s for s in ran if self.clock[s, 0] + 1 + N_HORZ > self.clock[s, 1]]
            for s in ran:
                self.ledger.step(s, int(self.clock[s, 0]) + 1, self.init_state[s], self.prob[s], iters[s], masks[s, 0],
                                 masks[s, 1], resid[s, 0], resid[s, 1], self._stream(s))
            for s in out:
                self.ledger.close(s, LEDGER_RETIRED, self.t_step)
        if self.clock is not None:
            self.clock = clock_tick(self.clock, self.clock[:, 2])
        if self.loop is not None:
            self._loop_open()
        self.t_step += 1

    def run(self, n_steps):
        for _ in range(int(n_steps)):
            if self.clock is not None and not self.clock[:, 2].any():
                break
            self.step()
        return self.record
