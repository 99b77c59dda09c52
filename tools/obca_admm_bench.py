#!/usr/bin/env python3
"""Times of the OBCA-ADMM edge step and of one full ADMM iterate on the GPU.

  edge launch      ms per launch of the edge kernel at --pairs vehicle pairs (x 7 slot problems),
                   HIP events around `repeats` launches, records resident
  full iterate     wall-clock ms of one ADMM iterate of OBCAPlanner on --scenarios seeded
                   scenarios: the local launch (scenarios x 2 problems), the host exchange
                   (bar_state_update, check_converge, record packing), the edge launch
  device iterate   the same MPC step of the same scenarios with the loop on the device
                   (OBCADevicePlanner.step: one piadmm_obca_plan_step, then the record's downloads),
                   wall-clock ms per ADMM iterate, and its ratio to the host iterate of this run

  --fleet          instead of the above: --scenarios different overtakes (obca.overtaking_fleet: own
                   speeds, gap, lane, rho and min_dis) through piadmm_obca_fleet_begin, and in the
                   same run the shared plan (piadmm_obca_plan_begin) on as many copies of the
                   default scenario from the same MPC step.  Per leg: wall-clock ms per ADMM
                   iterate of one piadmm_obca_plan_step (a warm-up step on its own plan first), the
                   mean local / edge SQP iterations and the status histogram over every solve of
                   the timed step (taken afterwards from an untimed iterate-by-iterate rerun, which
                   is bit-identical).  The two legs solve different problems: the SQP work tells
                   the solves' share of a difference from the glue's.  Written under the keys
                   "fleet" and "fleet_shared_leg" of the same JSON, the other keys kept.

  --trace          instead of the above: the same --steps MPC steps of --scenarios scenarios twice in one
                   process -- OBCADevicePlanner.run (a piadmm_obca_plan_step and the record's downloads
                   per step) and run_traced (one piadmm_obca_trace_run, the record and the clearances
                   kept on the device, downloaded once) -- wall-clock ms per step of each, whether
                   the two records are equal, and the smallest clearances.  Written under the key
                   "trace" of the same JSON, the other keys kept.

  --dual-pi        instead of the above, in one process on the shared plan of --scenarios scenarios:
                   (a) the plain plan and (b) the PI anti-windup law with kP = 0, kI = rho, windup = 0
                   (the same iterates to rounding, so the difference is the law's extra launch), each
                   the first MPC step of --repeats fresh plans, wall-clock ms per ADMM iterate, their
                   ratio and the spread of (a)'s own repeats; (c) one gain set (kP 0.5, kI = rho,
                   windup_sat 0.5, d_gain 0.5) on obca.overtaking_fleet(--scenarios, seed=0) next to
                   the plain fleet of the same run over --steps MPC steps: the histogram of stop
                   iterates, the edge statuses and the smallest clearances.  Information only.
                   Written under the key "dual_pi" of the same JSON, the other keys kept.

  --order          instead of the above, in one process at --scenarios scenarios over --steps MPC steps
                   from step 8 through run_traced, each leg the best of --repeats fresh plans after a
                   warm-up step on its own plan: (a) obca.overtaking_fleet(--scenarios, seed=0) without
                   the longest-first order (the yardstick: the launches of a plan that never heard of
                   it), (b) the same fleet with order=True, (c) the shared plan, (d) the shared plan
                   ordered (the overhead of the extra launches where there is nothing to gain), (e) a
                   fleet whose rows all equal the shared configuration (the glue's share of the
                   fleet's cost).  Per leg ms per iterate and per MPC step with the runs' range;
                   whether the records of (a) and (b) and of (c) and (d) are equal; and from an
                   untimed pass where the costliest scenarios sit in each iterate's list.  Written
                   under the key "order" of the same JSON, the other keys kept.

  --clock          instead of the above, in one process at --scenarios scenarios over --steps MPC steps
                   from step 8 through run_traced, the repeats of the legs alternating after a warm-up
                   step of each on its own plan: (a) obca.overtaking_fleet(--scenarios, seed=0) without a
                   clock (the yardstick: the launches of a plan that never heard of it), (b) the same
                   fleet with clock_init = NULL (everyone at step 8 over the whole reference: the same
                   results, the difference is the window, the list-taking shifts and the tick), and,
                   for information, (c) the fleet staggered, c0 drawn uniformly over the manoeuvre
                   (0 .. n_ref - 8), so scenarios retire while the others go on.  (b)/(a) is reported
                   next to the max/min spread of (a)'s own repeats; no ratio is fixed in advance.
                   Written under the key "clock" of the same JSON, the other keys kept.

  --migrate        instead of the above, in one process: all --scenarios tenants of
                   obca.overtaking_fleet(--scenarios, seed=0) (clocked, at step 8) move from one plan
                   into another on a second handle, two ways, the legs alternating over --repeats
                   repeats after one untimed repeat: (a) piadmm_obca_tenant_export + piadmm_obca_tenant_import
                   (one launch and one copy of the records each way), (b) the per-slot path there was
                   before: piadmm_obca_plan_get of STATE, REF, PAR, PROB and both thresholds, then one
                   piadmm_obca_clock_admit with every array (about fifteen synchronous copies or memsets
                   per slot).  (b) does less: an admission does not carry the running state, so this
                   compares upload mechanics only.  After each leg one MPC step of the destination is
                   timed next to the first step of a plan that never saw an import (the same work: the
                   source stands at its seeded state); that ratio is reported next to the fresh leg's
                   own spread.  No ratio is fixed in advance.  Written under the key "migrate" of the
                   same JSON, the other keys kept.

  --feedback       instead of the above, in one process at --scenarios scenarios of
                   obca.overtaking_fleet(--scenarios, seed=0) over --steps MPC steps from step 8 through
                   run_traced, the repeats of legs (a) and (b) alternating after a warm-up step of each
                   on its own plan, best of --repeats: (a) the plain fleet (the yardstick: the launches
                   of a plan that never heard of feedback), (b) the same fleet with the nominal plant and
                   a zero tape (piadmm_obca_feedback_plan: two more launches per MPC step, 2 x
                   --scenarios lanes of work next to the batched SQP launches).  (b)/(a) is reported
                   next to the max/min spread of (a)'s own repeats; no ratio is fixed in advance.  (c)
                   one run_traced each with prob = 0 and with prob = 1 for every scenario under the same
                   Gaussian tape (seed 0) on x and y, sigma = VAR_DELAY * the vehicle's reference speed
                   (the position scale of the delay statistics the tightening is built from): per
                   setting the share of scenarios whose smallest plain clearance over the run fell
                   below their min_dis.  Findings, not criteria.  Written under the key "feedback" of
                   the same JSON, the other keys kept.

  --stats          instead of the above, in one process: a traced run of --steps MPC steps from step 8 of
                   --scenarios scenarios of obca.overtaking_fleet(--scenarios, seed=0) under a Gaussian
                   disturbance tape (as --feedback's (c)), LAMBDA kept; then on that one trace, the
                   repeats alternating, best of --repeats: (a) trace_get of every item followed by
                   obca.fleet_stats_host (the yardstick: what a study had to do before), (b)
                   trace_stats + trace_gather of the 16 worst (piadmm_obca_stats_trace /
                   piadmm_obca_gather_trace: the reductions and the gather on the device).  Both
                   times, the bytes each leg brought to the host (exact, from the layouts) and whether
                   the two legs agree bit for bit.  No ratio is fixed in advance.  Written under the
                   key "stats" of the same JSON, the other keys kept.

  --noise          instead of the above, in one process at --scenarios scenarios of
                   obca.overtaking_fleet(--scenarios, seed=0) over --steps MPC steps from step 8 through
                   run_traced, the repeats of the legs alternating after a warm-up step of each on its
                   own plan, best of --repeats.  Setup, timed around the Python calls: (a) a tape from
                   numpy.random.default_rng(0).normal (generation, then piadmm_obca_feedback_plan's
                   finiteness check and upload of --scenarios x --steps x 80 bytes), (b)
                   piadmm_obca_noise_plan (one noise row, the stream ids, seed and k0).  The --steps
                   steps of both are timed too, but (a) and (b) draw different numbers and so run
                   different solves: no per-step claim is made from them.  The per-step cost of the one
                   extra launch is measured where the solves are the same: (p) the nominal plant under
                   a zero tape (--feedback's leg (b): the launches of the parent commit) against (z)
                   the same with a noise row of sigma = bias = 0 attached; (z)/(p) is reported next to
                   the max/min spread of (p)'s own repeats.  Stand-alone: piadmm_obca_noise_tape at
                   n = 65536, cap = 42 against the NumPy statement obca.noise_tape and against
                   rng.normal of the same shape, with the largest deviation from the statement.  No
                   ratio is fixed in advance.  Written under the key "noise" of the same JSON, the
                   other keys kept.

  --delay          instead of the above, in one process at --scenarios scenarios of
                   obca.overtaking_fleet(--scenarios, seed=0) over --steps MPC steps from step 8 through
                   run_traced.  The cost of the path, the repeats of the legs alternating after a
                   warm-up step of each, best of --repeats: (p) the nominal plant under a zero tape
                   (--noise's leg (p): the launches of the parent commit) against (d) the same with
                   the delay attached under a row that draws tau = 0 (k_plan_exchange_stale in
                   k_plan_exchange's place, one k_plan_delay launch per step); the two are the same
                   solves, so their records are compared; (d)/(p) is reported next to the max/min
                   spread of (p)'s own repeats and next to the (p) the key "noise" of the same JSON
                   holds from before.  The study: the nominal plant, no position noise, every message
                   tau ~ N(AVG_DELAY, VAR_DELAY) clipped to [0, DT] late, with prob = 0 and with
                   prob = 1, and the same two runs without the delay: the share of scenarios below
                   their own min_dis, the share touching, the median smallest plain clearance (the
                   columns of --feedback's disturbed runs).  One seed: findings.  Stand-alone:
                   piadmm_obca_delay_tau at n = 65536, cap = 42 once against obca.delay_tau.  No ratio
                   is fixed in advance.  Written under the key "delay" of the same JSON, the other
                   keys kept.

  --loop           instead of the above, in one process at --scenarios scenarios of
                   obca.overtaking_fleet(--scenarios, seed=0), every clock at step 8 over the whole
                   reference (clock_init = NULL), over --steps MPC steps through run_traced, the
                   repeats of the legs alternating after a warm-up step of each, best of
                   --repeats: (c) the clocked fleet without the loop against (l) the same with the
                   loop attached under rows that draw zero (the nominal plant, a noise row of sigma =
                   bias = 0, a delay row of tau_max = 0): k_loop_close, k_plan_set_init and k_loop_open
                   per shift, k_plan_exchange_stale in k_plan_exchange's place.  ms per MPC step of
                   both, (l)/(c) next to the max/min spread of (c)'s own repeats, and whether the two
                   records are equal: reported, not assumed -- (l) closes a step through the plant from
                   init_state under u0, (c) with X[1] of a solve that max_admm_iter may have cut short,
                   and where they differ the two run different solves and (l)/(c) prices no launch.
                   So a third leg, (p) the loop with the nominal plant alone (no noise or delay rows:
                   k_loop_close and k_plan_set_init per shift, the plain exchange), runs the solves of
                   (l): (l)/(p) prices the draws, k_loop_open and the stale exchange.
                   For comparison the keys "noise" and "delay" of the same JSON are quoted as they
                   stand (the one or two extra launches per step on an unclocked plan).  No ratio is
                   fixed in advance.  Written under the key "loop" of the same JSON, the other keys kept.

  --ledger         instead of the above, the --loop fleet (--scenarios clocked scenarios under the loop
                   with rows that draw zero, every clock at step 8 over the whole reference) over --steps
                   MPC steps of piadmm_obca_plan_step, the legs alternating after a warm-up step of each,
                   best of --repeats: (a) without a ledger, (b) with one (piadmm_obca_ledger_begin:
                   k_ledger_step per shift), (c) without one but with a download of STATE after every
                   step and obca.clearance + NumPy minima on the host, which is what a user does
                   without the ledger.  ms per MPC step, the max/min of each leg's repeats, the bytes
                   brought to the host per step, (b)/(a) next to (a)'s own spread.  Two more legs price
                   the append: the same fleet on references that end with the last step, so that all
                   --scenarios tenants retire at the last shift, without (ar) and with (br) a ledger.
                   Asserted: (a) and (b), and (ar) and (br), leave identical STATE and LAMBDA.  No
                   threshold is fixed in advance.  Written under the key "ledger" of the same JSON, the
                   other keys kept.

There is no CPU baseline on an equal footing (the C++ port of the local solver has no edge step);
the edge launch is reported next to the local launch so the reader sees its share of an iterate.
Writes one JSON (default profiles/obca_admm_bench.json) and prints it.
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "distributed-local-planner-pi-admm_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

from piadmm import obca  # noqa: E402


def edge_batch(n):
    """n edge records cycling over (t_step 0..41, prob): the seeded states with vehicle 0 pulled
    0.3 m towards vehicle 1, so the equality and the range row have work to do."""
    base = []
    for prob in (1, 0):
        for ts in range(42):
            bar = obca.seeded_bar_state(ts, prob)
            d = bar["local_x"][1, :, :2] - bar["local_x"][0, :, :2]
            bar["local_x"][0, :, :2] += 0.3 * d / np.linalg.norm(d, axis=1, keepdims=True)
            bar["local_x"][0, :, 3] += 0.01
            base.append(obca.edge_record(bar, prob=prob))
    return np.ascontiguousarray(np.stack([base[k % len(base)] for k in range(n)]))


def plan_leg(b, n, kw):
    """One MPC step of a device plan: timed as one piadmm_obca_plan_step, then rerun iterate by
    iterate for the solves' statistics."""
    dp = obca.OBCADevicePlanner(b, n, **kw)
    dp.step()
    dp.close()
    dp = obca.OBCADevicePlanner(b, n, **kw)
    fleet = dp.fleet
    t0 = time.perf_counter()
    dp.step()
    ms = (time.perf_counter() - t0) * 1e3
    iters = np.asarray(dp.record.iter_num_record[0])
    dp.close()
    dp = obca.OBCADevicePlanner(b, n, **kw)
    loc_st, loc_it, edge_st, edge_it, submitted = np.zeros(5, int), 0, np.zeros(5, int), 0, []
    left = n
    while left:
        left = dp.iterate()
        li, ei = dp.get("LOCAL_IST"), dp.get("EDGE_IST")
        submitted.append(len(ei))
        loc_st += np.bincount(li[:, 0], minlength=5)[:5]
        edge_st += np.bincount(ei[:, :, 0].ravel(), minlength=5)[:5]
        loc_it += int(li[:, 1].sum())
        edge_it += int(ei[:, :, 1].sum())
    same = bool(np.array_equal(dp.get("ITERS"), iters))
    dp.close()
    n_it = int(iters.max())
    return dict(entry="piadmm_obca_fleet_begin" if fleet else "piadmm_obca_plan_begin", scenarios=n,
                admm_iterates=n_it, step_ms=ms, iterate_ms=ms / max(n_it, 1), scenarios_submitted=submitted,
                stop_iterate_counts=np.bincount(iters, minlength=n_it + 1).tolist(),
                local_sqp_iters_mean=loc_it / max(int(loc_st.sum()), 1),
                edge_sqp_iters_mean=edge_it / max(int(edge_st.sum()), 1),
                local_status_counts=loc_st.tolist(), edge_status_counts=edge_st.tolist(),
                status_names=[obca.STATUS[k] for k in range(5)], rerun_stop_iterates_equal=same)


def fleet_main(a):
    b = obca.OBCABatch(0)
    n = a.scenarios
    common = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1)
    specs, par = obca.overtaking_fleet(n, seed=0)
    shared = plan_leg(b, n, common)
    fleet = plan_leg(b, n, dict(common, specs=specs, **par))
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["fleet"] = fleet
    out["fleet_shared_leg"] = shared
    out["fleet_over_shared_iterate"] = fleet["iterate_ms"] / shared["iterate_ms"]
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(fleet=fleet, fleet_shared_leg=shared,
                          fleet_over_shared_iterate=out["fleet_over_shared_iterate"])))


def trace_main(a):
    """The same --steps MPC steps of --scenarios scenarios twice in one process: OBCADevicePlanner.run
    (one piadmm_obca_plan_step per step, then the record's downloads) and run_traced (one
    piadmm_obca_trace_run, the record kept on the device and downloaded once at the end)."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1)
    warm = obca.OBCADevicePlanner(b, n, **kw)
    warm.step()
    warm.close()
    legs, recs = {}, {}
    for leg in ("run", "run_traced"):
        dp = obca.OBCADevicePlanner(b, n, **kw)
        t0 = time.perf_counter()
        tr = dp.run(K) if leg == "run" else dp.run_traced(K)
        ms = (time.perf_counter() - t0) * 1e3
        rec = dp.record
        dp.close()
        recs[leg] = rec
        iters = np.asarray(rec.iter_num_record)
        legs[leg] = dict(total_ms=ms, step_ms=ms / K, admm_iterates=int(iters.max(axis=1).sum()),
                         iterate_ms=ms / max(int(iters.max(axis=1).sum()), 1))
        if leg == "run_traced":
            legs[leg].update(min_clearance=float(tr.min_clearance.min()),
                             min_clearance_tight=float(tr.min_clearance_tight.min()),
                             scenarios_touching=int((tr.min_clearance == 0.0).sum()),
                             min_row_histogram=np.bincount(tr.min_row, minlength=K + 1).tolist())
    same = all(np.array_equal(np.asarray(getattr(recs["run"], k)), np.asarray(getattr(recs["run_traced"], k)))
               for k in ("state_record", "iter_num_record", "lambda_record"))
    res = dict(scenarios=n, steps=K, max_admm_iter=a.iterates - 1, run=legs["run"], run_traced=legs["run_traced"],
               traced_over_run_step=legs["run_traced"]["step_ms"] / legs["run"]["step_ms"], records_equal=same)
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["trace"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(trace=res)))


def dual_leg(b, n, kw, dual, repeats):
    """`repeats` timed first MPC steps of fresh plans (a warm-up step first), with or without the
    law: wall-clock ms per ADMM iterate of each, and the last step's iterates, duals and statuses."""
    warm = obca.OBCADevicePlanner(b, n, dual=dual, **kw)
    warm.step()
    warm.close()
    ms = []
    for _ in range(repeats):
        dp = obca.OBCADevicePlanner(b, n, dual=dual, **kw)
        t0 = time.perf_counter()
        dp.step()
        step_ms = (time.perf_counter() - t0) * 1e3
        iters = np.asarray(dp.record.iter_num_record[0])
        lamb = np.asarray(dp.record.lambda_record[0])
        mask = dp.record.status_record[0]["edge_status_mask"].copy()
        dp.close()
        ms.append(step_ms / max(int(iters.max()), 1))
    return dict(iterate_ms=min(ms), iterate_ms_runs=ms, admm_iterates=int(iters.max()),
                stop_iterate_counts=np.bincount(iters, minlength=int(iters.max()) + 1).tolist()), iters, lamb, mask


def dual_pi_main(a):
    """--dual-pi: (a) the plain shared plan, (b) the law with kP = 0, kI = rho, windup = 0 on it (the
    same iterates to rounding: the difference is the extra launch), both timed --repeats times in
    this process; (c) one gain set on overtaking_fleet(--scenarios, seed 0) next to the plain fleet
    of this run: stop iterates, statuses and the smallest clearances over --steps MPC steps."""
    b = obca.OBCABatch(0)
    n = a.scenarios
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1)
    plain, it_a, lam_a, _ = dual_leg(b, n, kw, None, a.repeats)
    law, it_b, lam_b, _ = dual_leg(b, n, kw, dict(kP=0.0, kI=1.0, windup=0), a.repeats)
    spread = max(plain["iterate_ms_runs"]) / min(plain["iterate_ms_runs"])
    ratio = law["iterate_ms"] / plain["iterate_ms"]
    res = dict(scenarios=n, repeats=a.repeats, max_admm_iter=a.iterates - 1, plain=plain, law_plain_gains=law,
               law_over_plain_iterate=ratio, plain_spread_max_over_min=spread,
               ratio_exceeds_plain_spread=bool(ratio > spread),
               stop_iterates_equal=bool(np.array_equal(it_a, it_b)),
               max_abs_lamb_bar_difference=float(np.abs(lam_a - lam_b).max()))
    # (c) information only: one gain set on the fleet, next to the plain fleet of the same run
    specs, par = obca.overtaking_fleet(n, seed=0)
    gains = dict(kP=0.5, kI=list(par["rho"]), windup_sat=0.5, d_gain=0.5, windup=1)
    fleet = {}
    for name, dual in (("plain", None), ("law", gains)):
        dp = obca.OBCADevicePlanner(b, n, specs=specs, dual=dual, **dict(kw, **par))
        tr = dp.run_traced(a.steps, keep_lambda=False)
        dp.close()
        edge = np.zeros(5, int)
        for bit in range(5):
            edge[bit] = int(((tr.status_mask[:, :, 1] >> bit) & 1).sum())
        fleet[name] = dict(stop_iterate_histogram=np.bincount(tr.iters.ravel(), minlength=a.iterates + 1).tolist(),
                           iterates_sum=int(tr.iters_sum.sum()),
                           steps_with_edge_status=edge.tolist(), status_names=[obca.STATUS[k] for k in range(5)],
                           min_clearance=float(tr.min_clearance.min()),
                           min_clearance_tight=float(tr.min_clearance_tight.min()),
                           scenarios_touching=int((tr.min_clearance == 0.0).sum()))
    res["fleet"] = dict(steps=a.steps, gains=dict(gains, kI="rho of each scenario"), **fleet)
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["dual_pi"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(dual_pi=res)))


def order_leg(b, n, kw, order, steps, repeats):
    """Best of `repeats` fresh plans (a warm-up step on its own plan first), each --steps MPC steps
    through run_traced, with or without the longest-first order; the last run's trace."""
    warm = obca.OBCADevicePlanner(b, n, order=order, **kw)
    state = warm.get("STATE")                     # the seeded state, so the later plans skip the host seeding
    warm.step()
    warm.close()
    ms, tr = [], None
    for _ in range(repeats):
        dp = obca.OBCADevicePlanner(b, n, order=order, state=state, **kw)
        t0 = time.perf_counter()
        tr = dp.run_traced(steps, keep_lambda=False)
        ms.append((time.perf_counter() - t0) * 1e3)
        dp.close()
    n_it = int(tr.iters.max(axis=1).sum())
    best = min(ms)
    return dict(order=bool(order), entry="piadmm_obca_fleet_begin" if dp.fleet else "piadmm_obca_plan_begin",
                admm_iterates=n_it, step_ms=best / steps, iterate_ms=best / max(n_it, 1),
                step_ms_runs=[v / steps for v in ms], iterate_ms_runs=[v / max(n_it, 1) for v in ms],
                spread_max_over_min=max(ms) / best,
                stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist()), tr


def order_predictor(b, n, kw, order, steps):
    """An untimed pass, iterate by iterate: where in each iterate's list the costliest scenarios sit.
    Per iterate: the list position (as a fraction of m) of the scenario with the iterate's largest Q
    (the first such in the list), and the share of the scenarios at or above the iterate's top-1 % Q
    that sit in the first quarter of the list."""
    dp = obca.OBCADevicePlanner(b, n, order=order, **kw)
    rows = []
    for step in range(steps):
        left, i_iter = n, 0
        while left:
            i_iter += 1
            left = dp.iterate()
            q = obca.plan_work(dp.get("LOCAL_IST"), dp.get("EDGE_IST"))[:, 0]
            m = len(q)
            top = np.sort(q)[::-1][max(int(np.ceil(0.01 * m)), 1) - 1]
            hot = np.flatnonzero(q >= top)
            rows.append(dict(step=step, iterate=i_iter, m=m, q_max=int(q.max()), q_mean=float(q.mean()),
                             argmax_position=float(int(np.argmax(q)) / m), top1pct_q=int(top), top1pct_count=int(len(hot)),
                             top1pct_share_in_first_quarter=float((hot < (m + 3) // 4).mean())))
        dp.shift()
    dp.close()
    return dict(order=bool(order), iterates=rows,
                argmax_position_mean=float(np.mean([r["argmax_position"] for r in rows])),
                top1pct_share_in_first_quarter_mean=float(np.mean([r["top1pct_share_in_first_quarter"] for r in rows])))


def order_main(a):
    """--order: five legs in one process at --scenarios scenarios over --steps MPC steps from step 8:
    (a) overtaking_fleet(seed 0) unordered -- the yardstick, the launches of a plan without the order --
    (b) the same fleet ordered, (c) the shared plan unordered, (d) the shared plan ordered, (e) a fleet
    whose rows all equal the shared configuration, unordered."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    common = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1)
    specs, par = obca.overtaking_fleet(n, seed=0)
    fleet_kw = dict(common, specs=specs, **par)
    same_kw = dict(common, ref_traj=np.ascontiguousarray(np.stack([np.stack(obca.ref_traj_gen())] * n)))
    legs, traces = {}, {}
    for name, kw, order in (("a_fleet", fleet_kw, False), ("b_fleet_ordered", fleet_kw, True),
                            ("c_shared", common, False), ("d_shared_ordered", common, True),
                            ("e_fleet_of_shared_rows", same_kw, False)):
        legs[name], traces[name] = order_leg(b, n, kw, order, K, a.repeats)

    def equal(x, y):
        return all(np.array_equal(getattr(traces[x], f), getattr(traces[y], f))
                   for f in ("states", "clearance", "iters", "status_mask", "primal", "dual", "min_clearance", "min_row",
                             "min_clearance_tight", "iters_sum"))

    res = dict(scenarios=n, steps=K, repeats=a.repeats, max_admm_iter=a.iterates - 1, legs=legs,
               ordered_over_plain_fleet=legs["b_fleet_ordered"]["step_ms"] / legs["a_fleet"]["step_ms"],
               fleet_spread_max_over_min=legs["a_fleet"]["spread_max_over_min"],
               ordered_over_plain_shared=legs["d_shared_ordered"]["step_ms"] / legs["c_shared"]["step_ms"],
               shared_spread_max_over_min=legs["c_shared"]["spread_max_over_min"],
               fleet_over_shared=legs["a_fleet"]["step_ms"] / legs["c_shared"]["step_ms"],
               fleet_of_shared_rows_over_shared=legs["e_fleet_of_shared_rows"]["step_ms"] / legs["c_shared"]["step_ms"],
               records_equal_fleet=equal("a_fleet", "b_fleet_ordered"),
               records_equal_shared=equal("c_shared", "d_shared_ordered"),
               records_equal_shared_rows=equal("c_shared", "e_fleet_of_shared_rows"),
               predictor=dict(ordered=order_predictor(b, n, fleet_kw, True, K),
                              unordered=order_predictor(b, n, fleet_kw, False, K)))
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["order"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(order=res)))


def clock_main(a):
    """--clock: (a) the plain fleet, (b) the same fleet with clock_init = NULL, (c) the fleet staggered
    over the manoeuvre; --steps MPC steps from step 8 through run_traced, the repeats alternating."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    specs, par = obca.overtaking_fleet(n, seed=0)
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1, specs=specs, **par)
    n_ref = 51
    c0 = np.random.default_rng(0).integers(0, n_ref - 8 + 1, n)
    stagger = np.ascontiguousarray(np.stack((c0, np.full(n, n_ref)), axis=1), np.int32)
    clocks = dict(a_fleet=None, b_fleet_null_clock=True, c_fleet_staggered=stagger)
    states, ms, traces, planners = {}, {k: [] for k in clocks}, {}, {}
    for name, clock in clocks.items():
        warm = obca.OBCADevicePlanner(b, n, clock=clock, **kw)
        assert warm.n_ref == n_ref
        states[name] = warm.get("STATE")              # the seeded state, so the later plans skip the host seeding
        warm.step()
        warm.close()
    for _ in range(a.repeats):
        for name, clock in clocks.items():
            dp = obca.OBCADevicePlanner(b, n, clock=clock, state=states[name], **kw)
            t0 = time.perf_counter()
            traces[name] = dp.run_traced(K, keep_lambda=False)
            ms[name].append((time.perf_counter() - t0) * 1e3)
            planners[name] = dp
            dp.close()
    legs = {}
    for name in clocks:
        tr = traces[name]
        n_it, best = int(tr.iters.max(axis=1).sum()), min(ms[name])
        legs[name] = dict(steps_run=int(tr.iters.shape[0]), admm_iterates=n_it, step_ms=best / max(tr.iters.shape[0], 1),
                          iterate_ms=best / max(n_it, 1), total_ms_runs=ms[name], spread_max_over_min=max(ms[name]) / best,
                          scenario_steps_run=int((tr.iters > 0).sum()),
                          stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist())
    alive_end = planners["c_fleet_staggered"].alive()
    legs["c_fleet_staggered"].update(alive_per_step=(traces["c_fleet_staggered"].iters > 0).sum(axis=1).tolist(),
                                     alive_at_end=int(alive_end.sum()))
    same = all(np.array_equal(getattr(traces["a_fleet"], f), getattr(traces["b_fleet_null_clock"], f))
               for f in ("states", "clearance", "iters", "status_mask", "primal", "dual", "min_clearance", "min_row",
                         "min_clearance_tight", "iters_sum"))
    ratio = min(ms["b_fleet_null_clock"]) / min(ms["a_fleet"])
    res = dict(scenarios=n, steps=K, repeats=a.repeats, max_admm_iter=a.iterates - 1, legs=legs,
               null_clock_over_plain=ratio, plain_spread_max_over_min=legs["a_fleet"]["spread_max_over_min"],
               ratio_exceeds_plain_spread=bool(ratio > legs["a_fleet"]["spread_max_over_min"]),
               records_equal_null_clock=same,
               staggered_ms_per_scenario_step=min(ms["c_fleet_staggered"]) / max(legs["c_fleet_staggered"]["scenario_steps_run"], 1),
               plain_ms_per_scenario_step=min(ms["a_fleet"]) / max(legs["a_fleet"]["scenario_steps_run"], 1))
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["clock"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(clock=res)))


def migrate_main(a):
    """--migrate: every tenant of a clocked fleet from one plan into another, through export + import and
    through plan_get + clock_admit, the legs alternating; then one MPC step of the destination against
    the first step of a plan that never saw an import."""
    import ctypes

    from piadmm import _lib
    n = a.scenarios
    specs, par = obca.overtaking_fleet(n, seed=0)
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1, specs=specs, clock=True, **par)
    ha, hb, hc = (obca.OBCABatch(0) for _ in range(3))
    lib = ha._lib
    src = obca.OBCADevicePlanner(ha, n, **kw)
    seeds = src.get("STATE")                           # the seeded state, so the later plans skip the host seeding
    dst = obca.OBCADevicePlanner(hb, n, state=seeds, **kw)
    slots = np.arange(n, dtype=np.int32)
    size = ctypes.c_int64()
    src._check(lib.piadmm_obca_tenant_export_bytes(ha._h, n, ctypes.byref(size)))
    blob = np.zeros(size.value, np.uint8)
    clock2 = np.ascontiguousarray(src.clock()[:, :2])
    iters = {k: np.zeros(n, np.int32) for k in ("import", "admit", "fresh")}

    def step_ms(pl, key):
        t0 = time.perf_counter()
        pl._check(lib.piadmm_obca_plan_step(pl.batch._h, _lib.iptr(iters[key])))
        return (time.perf_counter() - t0) * 1e3

    def leg_export_import():
        t0 = time.perf_counter()
        src._check(lib.piadmm_obca_tenant_export(ha._h, n, _lib.iptr(slots), blob.ctypes.data, blob.nbytes))
        t1 = time.perf_counter()
        dst._check(lib.piadmm_obca_tenant_import(hb._h, n, _lib.iptr(slots), blob.ctypes.data, blob.nbytes))
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    def leg_get_admit():
        t0 = time.perf_counter()
        got = {k: src.get(k) for k in ("STATE", "REF", "PAR", "PROB", "PRIMAL_THRES", "DUAL_THRES")}
        t1 = time.perf_counter()
        dst._check(lib.piadmm_obca_clock_admit(hb._h, n, _lib.iptr(slots), _lib.iptr(clock2), _lib.dptr(got["STATE"]),
                                               _lib.dptr(got["REF"]), _lib.dptr(got["PAR"]), _lib.iptr(got["PROB"]),
                                               _lib.dptr(got["PRIMAL_THRES"]), _lib.dptr(got["DUAL_THRES"])))
        t2 = time.perf_counter()
        return (t1 - t0) * 1e3, (t2 - t1) * 1e3

    ms = {k: [] for k in ("export", "import", "export_import", "get", "admit", "get_admit", "step_after_import",
                          "step_after_admit", "step_fresh")}
    same_iters = True
    for rep in range(a.repeats + 1):                    # repeat 0 is the warm-up
        e, i = leg_export_import()
        s_imp = step_ms(dst, "import")
        g, ad = leg_get_admit()
        s_adm = step_ms(dst, "admit")
        fresh = obca.OBCADevicePlanner(hc, n, state=seeds, **kw)
        s_fresh = step_ms(fresh, "fresh")
        fresh.close()
        same_iters = same_iters and np.array_equal(iters["import"], iters["fresh"]) and np.array_equal(iters["admit"], iters["fresh"])
        if rep == 0:
            continue
        for k, v in (("export", e), ("import", i), ("export_import", e + i), ("get", g), ("admit", ad), ("get_admit", g + ad),
                     ("step_after_import", s_imp), ("step_after_admit", s_adm), ("step_fresh", s_fresh)):
            ms[k].append(v)
    legs = {k: dict(best_ms=min(v), runs_ms=v, spread_max_over_min=max(v) / min(v)) for k, v in ms.items()}
    res = dict(scenarios=n, repeats=a.repeats, max_admm_iter=a.iterates - 1, blob_bytes=int(size.value),
               record_bytes=(int(size.value) - obca.TENANT_HEADER) // n, legs=legs,
               get_admit_over_export_import=legs["get_admit"]["best_ms"] / legs["export_import"]["best_ms"],
               step_after_import_over_fresh=legs["step_after_import"]["best_ms"] / legs["step_fresh"]["best_ms"],
               step_after_admit_over_fresh=legs["step_after_admit"]["best_ms"] / legs["step_fresh"]["best_ms"],
               fresh_step_spread_max_over_min=legs["step_fresh"]["spread_max_over_min"],
               stop_iterates_equal=bool(same_iters),
               note="the admission leg does less (it does not carry the running state): upload mechanics only")
    src.close()
    dst.close()
    for h in (ha, hb, hc):
        h.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["migrate"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(migrate=res)))


def feedback_main(a):
    """--feedback: (a) the plain fleet, (b) the same fleet with the nominal plant and a zero tape, the
    repeats alternating; (c) the fleet under one Gaussian tape with prob = 0 and with prob = 1."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    specs, par = obca.overtaking_fleet(n, seed=0)
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1, specs=specs, **par)
    zero = dict(par=None, tape=np.zeros((n, K, 2, obca.NX)))
    legs_fb = dict(a_fleet=None, b_fleet_nominal_plant_zero_tape=zero)
    states, ms, traces = {}, {k: [] for k in legs_fb}, {}
    for name, fb in legs_fb.items():
        warm = obca.OBCADevicePlanner(b, n, feedback=fb, **kw)
        states[name] = warm.get("STATE")              # the seeded state, so the later plans skip the host seeding
        warm.step()
        warm.close()
    for _ in range(a.repeats):
        for name, fb in legs_fb.items():
            dp = obca.OBCADevicePlanner(b, n, feedback=fb, state=states[name], **kw)
            t0 = time.perf_counter()
            traces[name] = dp.run_traced(K, keep_lambda=False)
            ms[name].append((time.perf_counter() - t0) * 1e3)
            dp.close()
    legs = {}
    for name in legs_fb:
        tr = traces[name]
        n_it, best = int(tr.iters.max(axis=1).sum()), min(ms[name])
        legs[name] = dict(steps_run=int(tr.iters.shape[0]), admm_iterates=n_it, step_ms=best / max(tr.iters.shape[0], 1),
                          iterate_ms=best / max(n_it, 1), total_ms_runs=ms[name], spread_max_over_min=max(ms[name]) / best,
                          stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist())
    ratio = min(ms["b_fleet_nominal_plant_zero_tape"]) / min(ms["a_fleet"])
    # the nominal plant with a zero tape closes a step at st + DT f(st, u0): the NLP's own constraint, met to
    # the solver's tolerance only, so the two records agree to that tolerance and not bit for bit
    dev = float(np.abs(traces["a_fleet"].states - traces["b_fleet_nominal_plant_zero_tape"].states).max())
    # (c) the disturbed fleet, with and without the delay tightening
    v_ref = np.array([[sp.v0, sp.v1] for sp in specs])
    tape = np.zeros((n, K, 2, obca.NX))
    tape[..., :2] = np.random.default_rng(0).standard_normal((n, K, 2, 2)) * (obca.VAR_DELAY * v_ref)[:, None, :, None]
    min_dis = np.broadcast_to(np.asarray(par.get("min_dis", 0.1), np.float64), (n,))
    disturbed = {}
    for prob in (0, 1):
        dp = obca.OBCADevicePlanner(b, n, feedback=dict(par=None, tape=tape), **dict(kw, prob=[prob] * n))
        tr = dp.run_traced(K, keep_lambda=False)
        dp.close()
        below = tr.min_clearance < min_dis
        disturbed[f"prob_{prob}"] = dict(
            share_below_min_dis=float(below.mean()), scenarios_below_min_dis=int(below.sum()),
            share_touching=float((tr.min_clearance == 0.0).mean()), min_clearance_smallest=float(tr.min_clearance.min()),
            min_clearance_median=float(np.median(tr.min_clearance)),
            min_clearance_tight_median=float(np.median(tr.min_clearance_tight)),
            stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist(),
            local_status_mask_or=int(np.bitwise_or.reduce(tr.status_mask[:, :, 0].ravel())),
            edge_status_mask_or=int(np.bitwise_or.reduce(tr.status_mask[:, :, 1].ravel())))
    res = dict(scenarios=n, steps=K, repeats=a.repeats, max_admm_iter=a.iterates - 1, legs=legs,
               nominal_plant_over_plain=ratio, plain_spread_max_over_min=legs["a_fleet"]["spread_max_over_min"],
               ratio_exceeds_plain_spread=bool(ratio > legs["a_fleet"]["spread_max_over_min"]),
               nominal_plant_max_state_deviation=dev,
               disturbed=dict(tape="Gaussian on x, y: sigma = VAR_DELAY * reference speed, seed 0",
                              sigma_m=dict(min=float((obca.VAR_DELAY * v_ref).min()), max=float((obca.VAR_DELAY * v_ref).max())),
                              **disturbed))
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["feedback"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(feedback=res)))


def stats_main(a):
    """--stats: on one traced, disturbed fleet run, (a) trace_get of everything + fleet_stats_host against
    (b) trace_stats + trace_gather of the 16 worst."""
    b = obca.OBCABatch(0)
    n, K, worst, B = a.scenarios, a.steps, min(16, a.scenarios), 32
    specs, par = obca.overtaking_fleet(n, seed=0)
    v_ref = np.array([[sp.v0, sp.v1] for sp in specs])
    tape = np.zeros((n, K, 2, obca.NX))
    tape[..., :2] = np.random.default_rng(0).standard_normal((n, K, 2, 2)) * (obca.VAR_DELAY * v_ref)[:, None, :, None]
    dp = obca.OBCADevicePlanner(b, n, feedback=dict(par=None, tape=tape), prob=[k % 2 for k in range(n)], t_step0=8,
                                max_admm_iter=a.iterates - 1, specs=specs, **par)
    dp.trace_begin(K, keep_lambda=True)
    R = dp.trace_run(K)
    names = ("STATES", "CLEARANCE", "ITERS", "STATUS_MASK", "PRIMAL", "DUAL", "LAMBDA", "SUMMARY")
    edges = np.linspace(0.0, 8.0, B)

    def leg_host():
        items = {k: dp.trace_get(k) for k in names}
        st = obca.fleet_stats_host(items["CLEARANCE"], items["SUMMARY"], items["ITERS"], items["STATUS_MASK"], edges, worst)
        w = st.worst
        return st, {k: (v[w] if k == "SUMMARY" else v[:, w]) for k, v in items.items()}, sum(v.nbytes for v in items.values())

    def leg_device():
        st = dp.trace_stats(edges, worst=worst)
        rec = dp.trace_gather(st.worst)
        # piadmm_obca_stats_t, hist, row_min, row_arg, row_below, worst; then the gathered record
        back = 72 + 2 * (B + 1) * 8 + (R + 1) * 2 * (8 + 4 + 4 * B) + 4 * worst
        return st, rec, back + obca.trace_gather_layout(R, worst, True)[1]
    leg_host(), leg_device()                              # warm-up
    ms, out = dict(a=[], b=[]), {}
    for _ in range(a.repeats):
        for key, leg in (("a", leg_host), ("b", leg_device)):
            t0 = time.perf_counter()
            out[key] = leg()
            ms[key].append((time.perf_counter() - t0) * 1e3)
    (sa, ra, bytes_a), (sb, rb, bytes_b) = out["a"], out["b"]
    same = all(np.array_equal(np.asarray(getattr(sa, f)), np.asarray(getattr(sb, f)), equal_nan=True)
               for f in ("hist", "nonfinite", "fleet_min", "fleet_arg", "iter_sum", "iter_max", "mask_or", "flagged",
                         "row_min", "row_arg", "row_below", "worst"))
    same = same and all(ra[k].tobytes() == rb[k].tobytes() for k in names)
    dp.close()
    b.close()
    res = dict(scenarios=n, steps=R, repeats=a.repeats, max_admm_iter=a.iterates - 1, edges=B, worst=worst,
               a_trace_get_all_then_host=dict(ms=min(ms["a"]), ms_runs=ms["a"], bytes_to_host=int(bytes_a)),
               b_trace_stats_then_gather=dict(ms=min(ms["b"]), ms_runs=ms["b"], bytes_to_host=int(bytes_b)),
               b_over_a_ms=min(ms["b"]) / min(ms["a"]), a_over_b_bytes=bytes_a / bytes_b, legs_equal=bool(same),
               scenarios_below_first_edges=[int(v) for v in sb.hist[0][:4]], worst_scenarios=[int(v) for v in sb.worst],
               worst_min_clearance=float(ra["SUMMARY"][0, 0]), flagged=int(sb.flagged), iter_sum=int(sb.iter_sum))
    out_json = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out_json = json.load(f)
    out_json["stats"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out_json, f, indent=1)
    print(json.dumps(dict(stats=res)))


def noise_main(a):
    """--noise: setup and steps of (a) a NumPy tape through feedback_plan and (b) noise_plan; the extra
    launch alone, (p) zero tape against (z) zero tape + zero noise; the stand-alone tape call."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    specs, par = obca.overtaking_fleet(n, seed=0)
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1, specs=specs, **par)
    sigma = (0.05, 0.05, 0.02, 0.002, 0.001)
    row = obca.noise_row(sigma=sigma)
    zero_tape = np.zeros((n, K, 2, obca.NX))

    def attach_a(dp):
        t0 = time.perf_counter()
        tape = np.random.default_rng(0).normal(0.0, sigma, (n, K, 2, obca.NX))
        t1 = time.perf_counter()
        dp.set_feedback(tape=tape)
        return dict(generate_ms=(t1 - t0) * 1e3, attach_ms=(time.perf_counter() - t1) * 1e3)

    def attach_b(dp):
        dp.set_feedback()
        t0 = time.perf_counter()
        dp.set_noise(par=row, seed=0)
        return dict(generate_ms=0.0, attach_ms=(time.perf_counter() - t0) * 1e3)

    def attach_p(dp):
        dp.set_feedback(tape=zero_tape)
        return {}

    def attach_z(dp):
        dp.set_feedback(tape=zero_tape)
        dp.set_noise(par=obca.noise_row(), seed=0)
        return {}
    legs_at = dict(a_numpy_tape=attach_a, b_noise_plan=attach_b, p_zero_tape=attach_p, z_zero_tape_zero_noise=attach_z)
    warm = obca.OBCADevicePlanner(b, n, **kw)
    state = warm.get("STATE")                          # the seeded state, so the later plans skip the host seeding
    for at in legs_at.values():
        at(warm)
        warm.step()
    warm.close()
    ms, setup, traces = {k: [] for k in legs_at}, {k: [] for k in legs_at}, {}
    for _ in range(a.repeats):
        for name, at in legs_at.items():
            dp = obca.OBCADevicePlanner(b, n, state=state, **kw)
            setup[name].append(at(dp))
            t0 = time.perf_counter()
            traces[name] = dp.run_traced(K, keep_lambda=False)
            ms[name].append((time.perf_counter() - t0) * 1e3)
            dp.close()
    legs = {}
    for name in legs_at:
        tr = traces[name]
        n_it, best = int(tr.iters.max(axis=1).sum()), min(ms[name])
        legs[name] = dict(steps_run=int(tr.iters.shape[0]), admm_iterates=n_it, step_ms=best / max(tr.iters.shape[0], 1),
                          total_ms_runs=ms[name], spread_max_over_min=max(ms[name]) / best,
                          stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist())
        if setup[name][0]:
            legs[name].update(generate_ms=min(s["generate_ms"] for s in setup[name]),
                              attach_ms=min(s["attach_ms"] for s in setup[name]),
                              attach_ms_runs=[s["attach_ms"] for s in setup[name]])
    legs["a_numpy_tape"]["bytes_uploaded"] = int(n * K * 2 * obca.NX * 8)
    legs["b_noise_plan"]["bytes_uploaded"] = int(obca.NOISE_PAR * 8 + n * 8)
    ratio = min(ms["z_zero_tape_zero_noise"]) / min(ms["p_zero_tape"])
    same = bool(np.array_equal(traces["p_zero_tape"].states, traces["z_zero_tape_zero_noise"].states)
                and np.array_equal(traces["p_zero_tape"].iters, traces["z_zero_tape_zero_noise"].iters))
    # the stand-alone tape at the size of a whole study
    n_big, cap = 65536, 42
    unit = obca.noise_row(sigma=1.0)
    b.noise_tape(1024, 2, unit)                         # warm-up
    alone = dict(device=[], numpy_statement=[], rng_normal=[])
    for _ in range(3):
        t0 = time.perf_counter()
        dev = b.noise_tape(n_big, cap, unit, seed=0)
        alone["device"].append((time.perf_counter() - t0) * 1e3)
        t0 = time.perf_counter()
        np.random.default_rng(0).normal(0.0, 1.0, (n_big, cap, 2, obca.NX))
        alone["rng_normal"].append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter()
    host = obca.noise_tape(n_big, cap, unit, seed=0)
    alone["numpy_statement"].append((time.perf_counter() - t0) * 1e3)
    res = dict(scenarios=n, steps=K, repeats=a.repeats, max_admm_iter=a.iterates - 1, sigma=list(sigma), legs=legs,
               zero_noise_over_zero_tape=ratio, zero_tape_spread_max_over_min=legs["p_zero_tape"]["spread_max_over_min"],
               ratio_exceeds_zero_tape_spread=bool(ratio > legs["p_zero_tape"]["spread_max_over_min"]),
               zero_noise_run_equals_zero_tape_run=same,
               extra_launch_ms_per_step=(min(ms["z_zero_tape_zero_noise"]) - min(ms["p_zero_tape"])) / K,
               stand_alone=dict(n=n_big, cap=cap, bytes=int(dev.nbytes), device_ms=min(alone["device"]),
                                device_ms_runs=alone["device"], numpy_statement_ms=alone["numpy_statement"][0],
                                rng_normal_ms=min(alone["rng_normal"]), rng_normal_ms_runs=alone["rng_normal"],
                                max_abs_deviation_from_statement=float(np.abs(dev - host).max()),
                                max_abs_z=float(np.abs(host).max()), mean=float(dev.mean()), variance=float(dev.var())))
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["noise"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(noise=res)))


def delay_main(a):
    """--delay: (p) zero tape against (d) zero tape + a delay row that draws tau = 0; the fleet under
    tau ~ N(AVG_DELAY, VAR_DELAY) with prob = 0 and prob = 1 next to the runs without delay; the
    stand-alone latencies."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    specs, par = obca.overtaking_fleet(n, seed=0)
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1, specs=specs, **par)
    zero_tape = np.zeros((n, K, 2, obca.NX))

    def attach_p(dp):
        dp.set_feedback(tape=zero_tape)

    def attach_d(dp):
        dp.set_feedback(tape=zero_tape)
        dp.set_delay(par=obca.delay_row(), seed=0)
    legs_at = dict(p_zero_tape=attach_p, d_zero_tape_zero_delay=attach_d)
    warm = obca.OBCADevicePlanner(b, n, **kw)
    state = warm.get("STATE")                          # the seeded state, so the later plans skip the host seeding
    for at in legs_at.values():
        at(warm)
        warm.step()
    warm.close()
    ms, traces = {k: [] for k in legs_at}, {}
    for _ in range(a.repeats):
        for name, at in legs_at.items():
            dp = obca.OBCADevicePlanner(b, n, state=state, **kw)
            at(dp)
            t0 = time.perf_counter()
            traces[name] = dp.run_traced(K, keep_lambda=False)
            ms[name].append((time.perf_counter() - t0) * 1e3)
            dp.close()
    legs = {}
    for name in legs_at:
        tr = traces[name]
        n_it, best = int(tr.iters.max(axis=1).sum()), min(ms[name])
        legs[name] = dict(steps_run=int(tr.iters.shape[0]), admm_iterates=n_it, step_ms=best / max(tr.iters.shape[0], 1),
                          total_ms_runs=ms[name], spread_max_over_min=max(ms[name]) / best,
                          stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist())
    tp, td = traces["p_zero_tape"], traces["d_zero_tape_zero_delay"]
    same = bool(all(np.array_equal(getattr(tp, f), getattr(td, f))
                    for f in ("states", "clearance", "iters", "status_mask", "primal", "dual")))
    ratio = min(ms["d_zero_tape_zero_delay"]) / min(ms["p_zero_tape"])
    before = None
    if os.path.exists(a.out):
        with open(a.out) as f:
            before = json.load(f).get("noise", {}).get("legs", {}).get("p_zero_tape", {}).get("step_ms")
    # the study: stale messages, with and without the delay tightening
    min_dis = np.broadcast_to(np.asarray(par.get("min_dis", 0.1), np.float64), (n,))
    row = obca.delay_row(avg=obca.AVG_DELAY, std=obca.VAR_DELAY)
    study = {}
    for prob in (0, 1):
        seeded = None                                   # the seeded state of this prob, from the first plan
        for delayed in (False, True):
            dp = obca.OBCADevicePlanner(b, n, state=seeded, feedback=dict(par=None),
                                        delay=dict(par=row, seed=0) if delayed else None, **dict(kw, prob=[prob] * n))
            seeded = dp.get("STATE")
            tr = dp.run_traced(K, keep_lambda=False)
            dp.close()
            below = tr.min_clearance < min_dis
            study[f"{'delay' if delayed else 'no_delay'}_prob_{prob}"] = dict(
                share_below_min_dis=float(below.mean()), scenarios_below_min_dis=int(below.sum()),
                share_touching=float((tr.min_clearance == 0.0).mean()), min_clearance_smallest=float(tr.min_clearance.min()),
                min_clearance_median=float(np.median(tr.min_clearance)),
                min_clearance_tight_median=float(np.median(tr.min_clearance_tight)),
                stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist(),
                local_status_mask_or=int(np.bitwise_or.reduce(tr.status_mask[:, :, 0].ravel())),
                edge_status_mask_or=int(np.bitwise_or.reduce(tr.status_mask[:, :, 1].ravel())))
    # the stand-alone latencies at the size of a whole study, once
    n_big, cap = 65536, 42
    b.delay_tau(1024, 2, row)                           # warm-up
    t0 = time.perf_counter()
    dev = b.delay_tau(n_big, cap, row, seed=0)
    dev_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    host = obca.delay_tau(n_big, cap, row, seed=0)
    host_ms = (time.perf_counter() - t0) * 1e3
    res = dict(scenarios=n, steps=K, repeats=a.repeats, max_admm_iter=a.iterates - 1, legs=legs,
               zero_delay_over_zero_tape=ratio, zero_tape_spread_max_over_min=legs["p_zero_tape"]["spread_max_over_min"],
               ratio_exceeds_zero_tape_spread=bool(ratio > legs["p_zero_tape"]["spread_max_over_min"]),
               zero_delay_run_equals_zero_tape_run=same,
               extra_ms_per_step=(min(ms["d_zero_tape_zero_delay"]) - min(ms["p_zero_tape"])) / K,
               zero_tape_step_ms_under_key_noise_before=before,
               study=dict(latency="tau ~ N(AVG_DELAY, VAR_DELAY) clipped to [0, DT], one per vehicle and step, seed 0; "
                                  "nominal plant, no position noise", **study),
               stand_alone=dict(n=n_big, cap=cap, bytes=int(dev.nbytes), device_ms=dev_ms, numpy_statement_ms=host_ms,
                                max_abs_deviation_from_statement=float(np.abs(dev - host).max()),
                                share_at_0=float((dev == 0.0).mean()), share_at_dt=float((dev == obca.DT).mean()),
                                mean=float(dev.mean())))
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["delay"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(delay=res)))


def loop_main(a):
    """--loop: (c) the clocked fleet against (l) the same with the loop under rows that draw zero."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    specs, par = obca.overtaking_fleet(n, seed=0)
    kw = dict(prob=[k % 2 for k in range(n)], t_step0=8, max_admm_iter=a.iterates - 1, specs=specs, clock=True, **par)
    zero = dict(plant=None, noise=obca.noise_row(), delay=obca.delay_row(tau_max=0.0), seed=0, k0=0)
    legs_at = dict(c_clocked=None, p_clocked_plant_only=dict(plant=None), l_clocked_zero_loop=zero)
    warm = obca.OBCADevicePlanner(b, n, **kw)
    state = warm.get("STATE")                          # the seeded state, so the later plans skip the host seeding
    warm.close()
    for loop in legs_at.values():
        warm = obca.OBCADevicePlanner(b, n, state=state, loop=loop, **kw)
        warm.step()
        warm.close()
    ms, traces, tau_any = {k: [] for k in legs_at}, {}, None
    for _ in range(a.repeats):
        for name, loop in legs_at.items():
            dp = obca.OBCADevicePlanner(b, n, state=state, loop=loop, **kw)
            t0 = time.perf_counter()
            traces[name] = dp.run_traced(K, keep_lambda=False)
            ms[name].append((time.perf_counter() - t0) * 1e3)
            if loop is not None:
                tau_any = bool(dp.loop_tau().any())
            dp.close()
    legs = {}
    for name in legs_at:
        tr = traces[name]
        n_it, best = int(tr.iters.max(axis=1).sum()), min(ms[name])
        legs[name] = dict(steps_run=int(tr.iters.shape[0]), admm_iterates=n_it, step_ms=best / max(tr.iters.shape[0], 1),
                          total_ms_runs=ms[name], spread_max_over_min=max(ms[name]) / best,
                          stop_iterate_histogram=np.bincount(tr.iters.ravel()).tolist())
    tc, tp, tl = traces["c_clocked"], traces["p_clocked_plant_only"], traces["l_clocked_zero_loop"]
    fields = ("states", "clearance", "iters", "status_mask", "primal", "dual")
    same = {f: bool(np.array_equal(getattr(tc, f), getattr(tl, f))) for f in fields}
    same_p = {f: bool(np.array_equal(getattr(tp, f), getattr(tl, f))) for f in fields}
    ratio = min(ms["l_clocked_zero_loop"]) / min(ms["c_clocked"])
    ratio_p = min(ms["l_clocked_zero_loop"]) / min(ms["p_clocked_plant_only"])
    # the older attachments' lines of the same file, as they stand
    quoted = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            old = json.load(f)
        for key, leg, over in (("noise", "z_zero_tape_zero_noise", "zero_noise_over_zero_tape"),
                               ("delay", "d_zero_tape_zero_delay", "zero_delay_over_zero_tape")):
            got = old.get(key, {})
            quoted[key] = {over: got.get(over), "p_zero_tape_step_ms": got.get("legs", {}).get("p_zero_tape", {}).get("step_ms"),
                           leg + "_step_ms": got.get("legs", {}).get(leg, {}).get("step_ms")}
    res = dict(scenarios=n, steps=K, repeats=a.repeats, max_admm_iter=a.iterates - 1, legs=legs,
               zero_loop_over_clocked=ratio, clocked_spread_max_over_min=legs["c_clocked"]["spread_max_over_min"],
               ratio_exceeds_clocked_spread=bool(ratio > legs["c_clocked"]["spread_max_over_min"]),
               extra_ms_per_step=(min(ms["l_clocked_zero_loop"]) - min(ms["c_clocked"])) / K,
               records_equal=same, max_abs_state_difference=float(np.abs(tc.states - tl.states).max()),
               zero_loop_over_plant_only=ratio_p, plant_only_spread_max_over_min=legs["p_clocked_plant_only"]["spread_max_over_min"],
               ratio_exceeds_plant_only_spread=bool(ratio_p > legs["p_clocked_plant_only"]["spread_max_over_min"]),
               extra_ms_per_step_over_plant_only=(min(ms["l_clocked_zero_loop"]) - min(ms["p_clocked_plant_only"])) / K,
               records_equal_plant_only=same_p,
               zero_loop_latencies_nonzero=tau_any, unclocked_attachments_quoted=quoted)
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["loop"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(loop=res)))


def ledger_main(a):
    """--ledger: the --loop fleet (a) without a ledger, (b) with one, (c) with a STATE download per step."""
    b = obca.OBCABatch(0)
    n, K = a.scenarios, a.steps
    specs, par = obca.overtaking_fleet(n, seed=0)
    prob = [k % 2 for k in range(n)]
    kw = dict(prob=prob, t_step0=8, max_admm_iter=a.iterates - 1, specs=specs, **par)
    zero = dict(plant=None, noise=obca.noise_row(), delay=obca.delay_row(tau_max=0.0), seed=0, k0=0)
    warm = obca.OBCADevicePlanner(b, n, clock=True, **kw)
    n_ref = warm.n_ref
    state = warm.get("STATE")                          # the seeded state, so the later plans skip the host seeding
    warm.close()
    # the service's clocks: everyone at step 8 over the whole reference; and, for the append, everyone
    # at step 8 on a reference that ends with the K-th step, so that all n retire at the last shift
    live = np.array([[8, n_ref]] * n, np.int32)
    last = np.array([[8, 8 + 8 + K - 1]] * n, np.int32)
    legs_at = dict(a_no_ledger=(live, False, False), b_ledger=(live, True, False), c_state_download=(live, False, True),
                   ar_no_ledger_all_retire=(last, False, False), br_ledger_all_retire=(last, True, False))

    def run(clock, ledger, download, steps):
        """One leg: `steps` MPC steps through piadmm_obca_plan_step, timed without the attachment."""
        dp = obca.OBCADevicePlanner(b, n, state=state, clock=clock, loop=zero, **kw)
        begin_ms, mins, per_step = 0.0, None, []
        if ledger:
            t0 = time.perf_counter()
            dp.ledger_begin(n)
            begin_ms = (time.perf_counter() - t0) * 1e3
        if download:
            st = dp.get("STATE")[:, 546:].reshape(n, 2, 5)
            mins = np.array([obca.clearance(st[s], prob[s]) for s in range(n)])
        t_all = time.perf_counter()
        for _ in range(steps):
            t0 = time.perf_counter()
            dp._check(dp._lib.piadmm_obca_plan_step(b._h, None))
            if download:
                # what a user does today: the states to the host, the clearances and the minima there
                st = dp.get("STATE")[:, 546:].reshape(n, 2, 5)
                mins = np.minimum(mins, np.array([obca.clearance(st[s], prob[s]) for s in range(n)]))
            per_step.append((time.perf_counter() - t0) * 1e3)
        total = (time.perf_counter() - t_all) * 1e3
        out = dict(total_ms=total, per_step_ms=per_step, begin_ms=begin_ms, mins=mins, STATE=dp.get("STATE"),
                   LAMBDA=dp.get("LAMBDA"))
        if ledger:
            out.update(count=dp.ledger_count(), running=dp.ledger_running(), records=dp.ledger_records())
        dp.close()
        return out

    for clock, ledger, download in legs_at.values():
        run(clock, ledger, download, 1)
    ms, last_ms, got = {k: [] for k in legs_at}, {k: [] for k in legs_at}, {}
    for _ in range(a.repeats):
        for name, (clock, ledger, download) in legs_at.items():
            got[name] = run(clock, ledger, download, K)
            ms[name].append(got[name]["total_ms"])
            last_ms[name].append(got[name]["per_step_ms"][-1])
    # the ledger changes nothing of the plan: asserted, on the fleet that is measured
    for x, y in (("a_no_ledger", "b_ledger"), ("ar_no_ledger_all_retire", "br_ledger_all_retire")):
        for item in ("STATE", "LAMBDA"):
            assert got[x][item].tobytes() == got[y][item].tobytes(), f"{item} of {y} differs from {x}"
    assert got["b_ledger"]["count"] == 0 and (got["b_ledger"]["running"]["steps"] == K).all()
    assert got["br_ledger_all_retire"]["count"] == n
    assert got["br_ledger_all_retire"]["records"]["slot"].tolist() == list(range(n))
    # bytes brought to the host per MPC step: the 4-byte active count of every iterate, which every leg
    # reads; (c) adds the states; the ledger adds nothing per step (its records come once, at the end)
    iterates = a.iterates
    host_bytes = dict(a_no_ledger=4 * iterates, b_ledger=4 * iterates, c_state_download=4 * iterates + n * 556 * 8,
                      ar_no_ledger_all_retire=4 * iterates, br_ledger_all_retire=4 * iterates)
    legs = {}
    for name in legs_at:
        best = min(ms[name])
        legs[name] = dict(step_ms=best / K, total_ms_runs=ms[name], spread_max_over_min=max(ms[name]) / best,
                          last_step_ms=min(last_ms[name]), host_bytes_per_step_at_most=host_bytes[name],
                          ledger_begin_ms=got[name]["begin_ms"])
    run_b = got["b_ledger"]["running"]
    dev = np.stack((run_b["min_clearance"], run_b["min_clearance_tight"]), axis=1)
    res = dict(scenarios=n, steps=K, repeats=a.repeats, max_admm_iter=a.iterates - 1, legs=legs,
               ledger_over_no_ledger=min(ms["b_ledger"]) / min(ms["a_no_ledger"]),
               no_ledger_spread_max_over_min=legs["a_no_ledger"]["spread_max_over_min"],
               ratio_exceeds_no_ledger_spread=bool(min(ms["b_ledger"]) / min(ms["a_no_ledger"])
                                                   > legs["a_no_ledger"]["spread_max_over_min"]),
               extra_ms_per_step=(min(ms["b_ledger"]) - min(ms["a_no_ledger"])) / K,
               download_over_no_ledger=min(ms["c_state_download"]) / min(ms["a_no_ledger"]),
               all_retire_ledger_over_no_ledger=min(ms["br_ledger_all_retire"]) / min(ms["ar_no_ledger_all_retire"]),
               all_retire_last_step_extra_ms=min(last_ms["br_ledger_all_retire"]) - min(last_ms["ar_no_ledger_all_retire"]),
               all_retire_no_ledger_spread_max_over_min=legs["ar_no_ledger_all_retire"]["spread_max_over_min"],
               state_and_lambda_equal_with_and_without_ledger=True,
               ledger_bytes_at_the_end=int(n * 176),
               ledger_minima_max_abs_deviation_from_host_minima=float(np.abs(dev - got["c_state_download"]["mins"]).max()))
    b.close()
    out = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            out = json.load(f)
    out["ledger"] = res
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(dict(ledger=res)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--ledger", action="store_true")
    ap.add_argument("--loop", action="store_true")
    ap.add_argument("--delay", action="store_true")
    ap.add_argument("--noise", action="store_true")
    ap.add_argument("--stats", action="store_true")
    ap.add_argument("--feedback", action="store_true")
    ap.add_argument("--migrate", action="store_true")
    ap.add_argument("--clock", action="store_true")
    ap.add_argument("--order", action="store_true")
    ap.add_argument("--dual-pi", action="store_true")
    ap.add_argument("--fleet", action="store_true")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--scenarios", type=int, default=2048)
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--iterates", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "obca_admm_bench.json"))
    a = ap.parse_args()
    if a.ledger:
        return ledger_main(a)
    if a.loop:
        return loop_main(a)
    if a.delay:
        return delay_main(a)
    if a.noise:
        return noise_main(a)
    if a.stats:
        return stats_main(a)
    if a.feedback:
        return feedback_main(a)
    if a.migrate:
        return migrate_main(a)
    if a.clock:
        return clock_main(a)
    if a.order:
        return order_main(a)
    if a.dual_pi:
        return dual_pi_main(a)
    if a.fleet:
        return fleet_main(a)
    if a.trace:
        return trace_main(a)
    b = obca.OBCABatch(0)
    recs = edge_batch(a.pairs)
    b.time_edge(recs, 1)                                   # warm-up
    edge_ms = [b.time_edge(recs, a.repeats) for _ in range(3)]
    res = b.solve_edge(recs)
    # the local launch at the same scenario count (pairs x 2 problems), for the share
    lrecs = obca.scenario_batch(2 * a.pairs)
    b.upload(lrecs)
    b.time(1)
    local_ms = [b.time(max(1, a.repeats // 2)) for _ in range(2)]
    # full iterates
    stamps = []
    t_last = [time.perf_counter()]

    def on_stage(name, inp, outp):
        now = time.perf_counter()
        stamps.append((name, (now - t_last[0]) * 1e3))
        t_last[0] = now

    pl = obca.OBCAPlanner(b, a.scenarios, prob=[k % 2 for k in range(a.scenarios)], t_step0=8,
                          max_admm_iter=a.iterates - 1, on_stage=on_stage)
    t0 = time.perf_counter()
    t_last[0] = t0
    pl.step()
    total = (time.perf_counter() - t0) * 1e3
    n_it = sum(1 for s in stamps if s[0] == "local")
    by = {}
    for name, ms in stamps:
        by[name] = by.get(name, 0.0) + ms
    # the same scenarios with the loop on the device (OBCADevicePlanner: one piadmm_obca_plan_step per
    # MPC step): a warm-up step on its own plan, then the timed first step of a fresh plan, so both
    # planners time the same MPC step from the same seeded state
    kw = dict(prob=[k % 2 for k in range(a.scenarios)], t_step0=8, max_admm_iter=a.iterates - 1)
    dp = obca.OBCADevicePlanner(b, a.scenarios, **kw)
    dp.step()
    dp.close()
    dp = obca.OBCADevicePlanner(b, a.scenarios, **kw)
    t0 = time.perf_counter()
    dp.step()
    dev_total = (time.perf_counter() - t0) * 1e3
    dev_it = int(np.asarray(dp.record.iter_num_record[0]).max())
    dev_iters_equal = bool(np.array_equal(dp.record.iter_num_record[0], pl.record.iter_num_record[0]))
    dp.close()
    out = dict(
        pairs=a.pairs, slot_problems=a.pairs * obca.NT, repeats=a.repeats,
        edge_ms_per_launch=min(edge_ms), edge_ms_runs=edge_ms,
        edge_status_counts=np.bincount(res.status.ravel(), minlength=5).tolist(),
        edge_sqp_iters_mean=float(res.iters.mean()),
        local_problems=len(lrecs), local_ms_per_launch=min(local_ms),
        scenarios=a.scenarios, admm_iterates=n_it, iterate_ms=total / max(n_it, 1),
        stage_ms_per_iterate={k: v / max(n_it, 1) for k, v in by.items()},
        device_admm_iterates=dev_it, device_step_ms=dev_total, device_iterate_ms=dev_total / max(dev_it, 1),
        device_over_host_iterate=(dev_total / max(dev_it, 1)) / (total / max(n_it, 1)),
        host_over_device_iterate=(total / max(n_it, 1)) / (dev_total / max(dev_it, 1)),
        device_stop_iterates_equal_host=dev_iters_equal,
        baseline=None, note="no CPU baseline exists for the edge step",
    )
    b.close()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
