// piadmm_steps.cpp -- the launches of MPC steps and how they end (C-ABI of libpiadmm, piadmm_ctx.h):
// per-component, fixed-iteration, in-kernel, device-decided and host-decided termination, the X / Z
// phases of sharded and split graphs, the job's all-reduce and its communicator, host stepping.
#include <array>

#include "piadmm_ctx.h"

namespace {

// A stop / distance decision the host takes within tie_tol of its threshold (the device kernels
// log their own, pd::scalar_tie).
void host_tie(piadmm_ctx* h, int t, int it, int kind, int id, int idx, double v, double thr) {
  if (!(h->tie_tol > 0.0) || !(std::fabs(v - thr) <= h->tie_tol * std::fabs(thr))) return;
  ++h->host_tie_cnt[kind];
  piadmm_near_tie_t ev{};
  ev.step = t;
  ev.iter = it;
  ev.kind = kind;
  ev.id = id;
  ev.index = idx;
  ev.margin = (v - thr) / thr;
  if (h->host_ties.size() < PIADMM_TIE_CAP) h->host_ties.push_back(ev);
}

// Sum over the job's ranks of n doubles at send into recv (may alias), on the handle's stream:
// ncclAllReduce over the RCCL communicator, else the host transport callback (through pinned
// memory; the callback returns when every rank has contributed), else one rank: a copy.
int allreduce(piadmm_ctx* h, const double* send, double* recv, size_t n) {
  if (n == 0) return 0;
  if (h->comm) {
    ncclResult_t r = ncclAllReduce(send, recv, n, ncclDouble, ncclSum, h->comm, h->stream);
    if (r != ncclSuccess) return fail(h, PIADMM_E_HIP, std::string("ncclAllReduce: ") + ncclGetErrorString(r));
    return 0;
  }
  if (h->xfn) {
    if (n > h->h_x_n) {
      h->h_x_n = 0;
      HIPCHK(h, h->h_x.make(n));
      h->h_x_n = n;
    }
    HIPCHK(h, hipMemcpyAsync(h->h_x, send, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (int rc = h->xfn(h->xctx, h->h_x, (int64_t)n))
      return fail(h, PIADMM_E_STATE, "all-reduce callback failed with " + std::to_string(rc));
    HIPCHK(h, hipMemcpyAsync(recv, h->h_x, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
    return 0;
  }
  if (send != recv && pd::launch_copy(recv, send, n, h->stream) != 0)
    return fail(h, PIADMM_E_HIP, std::string("copy kernel: ") + hipGetErrorString(pd::g_launch_err));
  return 0;
}

// One launch of the step kernel of the scenario's mode (fused components / general graph).
int launch_step(const pd::DevArgs& a, int t, int n, int it0, int it1, int flags, hipStream_t s) {
  return a.graph ? pd::launch_graph_step(a, t, n, it0, it1, flags, s) : pd::launch_mpc_step(a, t, n, it0, it1, flags, s);
}

// The launches of ONE outer iteration `it` of MPC step tk under the global scope (term_global,
// the stop decided outside the kernel): one launch; or -- a sharded graph with pairs across ranks
// (SURVEY.md 8e), or a connected component split over workgroups -- an X launch (the x-steps;
// boundary agents write px | py | u to their exchange slot), ONE all-reduce of the exchange buffer
// (sharded: the ranks' slots are disjoint and zero elsewhere, so the sum is an all-gather), and a Z
// launch (ghost agents read their owner's values; every local pair -- a cross-rank pair on both of
// its ranks, bit-identically -- runs its collision test, pair QP, dual update and residual terms).
// A split component's blocks reset their pairs in a step-init launch before any block's first
// x-step reads them (casadi/main.py:52-63).
int32_t iteration_launches(piadmm_handle_t h, int32_t tk, int it, int extra) {
  hipStream_t s = h->stream;
  int f = (it == 0 ? pd::F_FIRST : 0) | pd::F_GLOBAL | extra;
  if (h->xchg || h->split) {
    if (it == 0 && h->split) {
      LAUNCH(h, launch_step(h->a, tk, 1, 0, 0, pd::F_FIRST | pd::F_GLOBAL | pd::F_INITONLY, s));
      f &= ~pd::F_FIRST;
    }
    LAUNCH(h, launch_step(h->a, tk, 1, it, it + 1, f | pd::F_XONLY, s));
    const size_t nx = h->xchg ? (size_t)h->n_slots * 3 * (h->cfg.H + 1) : 0;
    if (int rc = allreduce(h, h->a.xbuf, h->d_xrecv, nx)) return rc;
    LAUNCH(h, launch_step(h->a, tk, 1, it, it + 1, pd::F_GLOBAL | pd::F_ZONLY | extra, s));
  } else {
    LAUNCH(h, launch_step(h->a, tk, 1, it, it + 1, f, s));
  }
  return PIADMM_OK;
}

// One MPC step under device-decided global termination (term_global with natural termination
// across ranks -- RCCL or the host transport --, a split component, or PIADMM_NO_COOP on one rank).
// Chunks of outer iterations are enqueued ahead: per iteration its launches (iteration_launches),
// the termination partials, their all-reduce and k_decide, which applies the reference's stop rules
// (casadi/main.py:115-118,174-178) on the device and sets the stop flag; launches after the stop
// return at once.  The host reads the stop state once per chunk (chunk = the previous step's
// iteration count, doubled while the step runs on), instead of one host round trip per outer
// iteration; the LAST launch takes the iteration count and the NANLAST case from the device.
int32_t devstop_step(piadmm_handle_t h, int32_t tk, bool sync_outputs) {
  const piadmm_config_t& c = h->cfg;
  hipStream_t s = h->stream;
  const int M = c.max_outer;
  HIPCHK(h, hipMemsetAsync(h->a.gctl, 0, 4 * sizeof(int), s));
  if (!h->a.graph) LAUNCH(h, pd::launch_pair_deff(h->a, s));
  int it = 0, K = std::max(1, std::min(h->chunk_guess, M));
  while (true) {
    const int n = std::min(K, M - it);
    for (int j = 0; j < n; ++j, ++it) {
      if (int rc = iteration_launches(h, tk, it, pd::F_DEVSTOP)) return rc;
      double* part = h->d_part + (size_t)5 * it;
      LAUNCH(h, h->a.graph ? pd::launch_graph_partials(h->a, part, s, 1) : pd::launch_term_partials(h->a, it, part, s, 1));
      if (int rc = allreduce(h, part, part, 5)) return rc;
      LAUNCH(h, pd::launch_decide(h->a, tk, it, part, s));
    }
    HIPCHK(h, hipMemcpyAsync(h->h_ctl, h->a.gctl, 4 * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    if (h->h_ctl[0] || it >= M) break;
    K *= 2;
  }
  const int nit = h->h_ctl[2], nanlast = h->h_ctl[1];
  h->chunk_guess = std::max(1, nit);
  h->giters = nit;
  LAUNCH(h, launch_step(h->a, tk, 1, nit, nit, pd::F_LAST | pd::F_GLOBAL | pd::F_DEVSTOP, s));
  if (sync_outputs) {
    const int nrec = nanlast ? nit - 1 : nit;
    h->ghist.assign((size_t)2 * M, NAN);
    if (nrec > 0) {
      HIPCHK(h, hipMemcpyAsync(h->h_part, h->a.ghist, (size_t)2 * nrec * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      std::copy(h->h_part.get(), h->h_part + 2 * nrec, h->ghist.begin());
    }
  }
  return PIADMM_OK;
}

// One outer iteration `it` of MPC step t under host-decided global termination (term_global
// without the in-kernel stop test: PIADMM_HOST_DECIDE, or host stepping): the iteration's launches,
// the job's termination partials (all-reduced), and the reference's stop rules over all agents
// (casadi/main.py:115-118,174-178; MATLAB :191-210).  flag / nanlast carry the step's state;
// *stop = 1 when the step ends at this iteration.
int32_t global_iteration(piadmm_handle_t h, int32_t tk, int it, int& flag, int& nanlast, int* stop) {
  const piadmm_config_t& c = h->cfg;
  hipStream_t s = h->stream;
  *stop = 0;
  if (int rc = iteration_launches(h, tk, it, 0)) return rc;
  double* part = h->d_part + (size_t)5 * it;
  LAUNCH(h, h->a.graph ? pd::launch_graph_partials(h->a, part, s) : pd::launch_term_partials(h->a, it, part, s));
  if (int rc = allreduce(h, part, part, 5)) return rc;
  HIPCHK(h, hipMemcpyAsync(h->h_part, part, 5 * sizeof(double), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  const double rk = h->h_part[0], sk = h->h_part[1], n_act = h->h_part[2];
  const double n_seen = h->h_part[3], n_bad = h->h_part[4];
  if (n_act == 0.0 && flag == 0 && !c.fixed_iters) {   // no pair collides anywhere: stop (casadi/main.py:115-116)
    nanlast = 1;
    *stop = 1;
    return PIADMM_OK;
  }
  flag = 1;
  h->ghist[2 * it + 0] = rk;
  h->ghist[2 * it + 1] = sk;
  if (c.fixed_iters) return PIADMM_OK;   // throughput mode: the history only, never a stop
  host_tie(h, tk, it, PIADMM_TIE_STOP, -1, 0, rk, c.eps_pri);
  host_tie(h, tk, it, PIADMM_TIE_STOP, -1, 1, sk, c.eps_dual);
  const bool dist_ok = n_seen > 0.0 && n_bad == 0.0;
  if (rk <= c.eps_pri && sk <= c.eps_dual && (!c.term_dist_check || dist_ok)) *stop = 1;
  return PIADMM_OK;
}

// MPC steps of a job whose iterations are split into X and Z launches (a sharded graph with pairs
// across ranks, or a component split over workgroups), one step at a time.  Fixed iterations: the
// steps' residual histories are all-reduced ONCE for the n steps (n x 2 x max_outer doubles), the
// same collective as run_steps' persistent launch, so ranks of one job that take different paths
// (a split component on one rank only) still issue matching collectives.
int32_t run_steps_phases(piadmm_handle_t h, int32_t t, int32_t n, bool sync_outputs) {
  const piadmm_config_t& c = h->cfg;
  hipStream_t s = h->stream;
  const int M = c.max_outer;
  for (int k = 0; k < n; ++k) {
    const int tk = t + k;
    if (!c.fixed_iters && !h->host_decide) {
      if (int rc = devstop_step(h, tk, sync_outputs && k == n - 1)) return rc;
      continue;
    }
    h->ghist.assign((size_t)2 * M, NAN);
    int flag = 0, nit = 0, nanlast = 0;
    if (c.fixed_iters && h->xchg && !h->split && M > 1 && !knob_no_zx()) {
      // a sharded job's fixed iterations, one launch between two exchanges: X(0), then per
      // iteration it the Z phase of it and the X phase of it+1 in ONE launch (a component is one
      // workgroup: its x-steps read only its own pairs' hat / lam), then Z(M-1) -- M + 1 launches
      // and M all-reduces per step instead of 2M launches
      const size_t nx = (size_t)h->n_slots * 3 * (c.H + 1);
      LAUNCH(h, launch_step(h->a, tk, 1, 0, 1, pd::F_FIRST | pd::F_GLOBAL | pd::F_XONLY, s));
      if (int rc = allreduce(h, h->a.xbuf, h->d_xrecv, nx)) return rc;
      for (int it = 0; it + 1 < M; ++it) {
        LAUNCH(h, launch_step(h->a, tk, 1, it, it + 2, pd::F_GLOBAL | pd::F_ZONLY | pd::F_XONLY, s));
        if (int rc = allreduce(h, h->a.xbuf, h->d_xrecv, nx)) return rc;
      }
      LAUNCH(h, launch_step(h->a, tk, 1, M - 1, M, pd::F_GLOBAL | pd::F_ZONLY, s));
      nit = M;
    } else
    for (int it = 0; it < M; ++it) {
      nit = it + 1;
      if (c.fixed_iters) {
        if (int rc = iteration_launches(h, tk, it, 0)) return rc;
        // the iteration's (rk, sk): a split component's sums in the reference's pair order
        // (k_graph_partials), a sharded graph's the blocks' partials -- the history of the step
        if (h->split) LAUNCH(h, pd::launch_graph_partials(h->a, h->d_part + (size_t)k * 2 * M + 2 * it, s, 0, 2));
        continue;
      }
      int stop = 0;
      if (int rc = global_iteration(h, tk, it, flag, nanlast, &stop)) return rc;
      if (stop) break;
    }
    h->giters = nit;
    LAUNCH(h, launch_step(h->a, tk, 1, nit, nit, pd::F_LAST | pd::F_GLOBAL | (nanlast ? pd::F_NANLAST : 0), s));
    if (c.fixed_iters && !h->split) LAUNCH(h, pd::launch_resid_history(h->a, 1, h->d_part + (size_t)k * 2 * M, s));
  }
  if (c.fixed_iters) {
    if (int rc = allreduce(h, h->d_part, h->d_part, (size_t)n * 2 * M)) return rc;
    h->giters = M;
    if (sync_outputs) {
      HIPCHK(h, hipMemcpyAsync(h->h_part, h->d_part + (size_t)(n - 1) * 2 * M, (size_t)2 * M * sizeof(double),
                               hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      h->ghist.assign(h->h_part.get(), h->h_part + 2 * M);
    }
  }
  return PIADMM_OK;
}

// MPC steps t .. t+n-1 (n <= step_cap).  Per-component termination, or fixed iterations under
// term_global: ONE persistent launch for all n steps (each workgroup runs its component's steps
// back to back), plus, under term_global, the component-summed residual history of every step,
// all-reduced once (n x 2 x max_outer doubles).  Natural global termination: in-kernel behind a
// grid barrier (one rank, cooperative launch), else one step at a time with the stop decided on
// the device (devstop_step) or, PIADMM_HOST_DECIDE=1, on the host after every outer iteration.
int32_t run_steps(piadmm_handle_t h, int32_t t, int32_t n, bool sync_outputs) {
  const piadmm_config_t& c = h->cfg;
  hipStream_t s = h->stream;
  const int M = c.max_outer;
  if (h->xchg || h->split) return run_steps_phases(h, t, n, sync_outputs);
  if (!c.term_global) {
    LAUNCH(h, launch_step(h->a, t, n, 0, M, pd::F_FIRST | pd::F_LAST, s));
    return PIADMM_OK;
  }
  if (c.fixed_iters) {
    LAUNCH(h, launch_step(h->a, t, n, 0, M, pd::F_FIRST | pd::F_LAST | pd::F_GLOBAL, s));
    LAUNCH(h, pd::launch_resid_history(h->a, n, h->d_part, s));
    if (int rc = allreduce(h, h->d_part, h->d_part, (size_t)n * 2 * M)) return rc;
    h->giters = M;
    if (sync_outputs) {
      const double* last = h->d_part + (size_t)(n - 1) * 2 * M;
      HIPCHK(h, hipMemcpyAsync(h->h_part, last, (size_t)2 * M * sizeof(double), hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      h->ghist.assign(h->h_part.get(), h->h_part + 2 * M);
    }
    return PIADMM_OK;
  }
  if (h->coop && !h->comm && !h->xfn &&
      launch_step(h->a, t, n, 0, M, pd::F_FIRST | pd::F_LAST | pd::F_GLOBAL | pd::F_COOP, s) != 0) {
    (void)hipGetLastError();       // the cooperative launch was refused: host-decided path from now on
    h->coop = false;
  }
  if (h->coop && !h->comm && !h->xfn) {
    if (sync_outputs) {
      int gi = 0;
      HIPCHK(h, hipMemcpyAsync(h->h_part, h->a.ghist + (size_t)(n - 1) * 2 * M, (size_t)2 * M * sizeof(double),
                               hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipMemcpyAsync(&gi, h->a.giters + (n - 1), sizeof(int), hipMemcpyDeviceToHost, s));
      HIPCHK(h, hipStreamSynchronize(s));
      h->ghist.assign(h->h_part.get(), h->h_part + 2 * M);
      h->giters = gi;
    }
    return PIADMM_OK;
  }
  for (int k = 0; k < n; ++k) {
    const int tk = t + k;
    if (!h->host_decide) {
      if (int rc = devstop_step(h, tk, sync_outputs && k == n - 1)) return rc;
      continue;
    }
    LAUNCH(h, pd::launch_pair_deff(h->a, s));
    h->ghist.assign((size_t)2 * M, NAN);
    int flag = 0, nit = 0, nanlast = 0;
    for (int it = 0; it < M; ++it) {
      int stop = 0;
      if (int rc = global_iteration(h, tk, it, flag, nanlast, &stop)) return rc;
      nit = it + 1;
      if (stop) break;
    }
    h->giters = nit;
    LAUNCH(h, launch_step(h->a, tk, 1, nit, nit, pd::F_LAST | pd::F_GLOBAL | (nanlast ? pd::F_NANLAST : 0), s));
  }
  return PIADMM_OK;
}

// The job's ranks agree on the MPC steps per launch (the smallest): the fixed-iteration residual
// history is all-reduced once per launch, so every rank must cut a run into the same launches
// (step_cap depends on the rank's component count).  An all-gather through the sum: slot k of a
// 33-double buffer counts the ranks whose cap is k.
int32_t sync_step_cap(piadmm_handle_t h) {
  double v[33] = {};
  v[std::min(32, std::max(1, h->step_cap))] = 1.0;
  hipStream_t s = h->stream;
  HIPCHK(h, hipMemcpyAsync(h->d_part, v, sizeof(v), hipMemcpyHostToDevice, s));   // (d_part: >= 33 doubles)
  if (int rc = allreduce(h, h->d_part, h->d_part, 33)) return rc;
  HIPCHK(h, hipMemcpyAsync(v, h->d_part, sizeof(v), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  int cap = h->step_cap;
  for (int k = 1; k <= 32; ++k)
    if (v[k] > 0.0) {
      cap = std::min(cap, k);
      break;
    }
  h->step_cap = cap;
  h->cap_synced = true;
  return PIADMM_OK;
}

// A step at t0 that does not continue the receding-horizon sequence forgets the pairs' stored
// active sets (codes, step index, the snapshot's validity: pd_qp.h gi_solve / gi_snap_restore).
// t_next: -1 = no step yet (nothing stored), -2 = the last run failed part-way (whatever is stored
// may belong to any step: always forget it), else the step the last completed run leads to.
int32_t continue_sequence(piadmm_handle_t h, int32_t t0) {
  if (h->t_next != -1 && t0 != h->t_next && h->E)
    HIPCHK(h, hipMemsetAsync(h->a.gi_ws, 0, (size_t)h->E * (2 + pd::WAVE) * sizeof(int), h->stream));
  return PIADMM_OK;
}

int32_t enqueue_steps(piadmm_handle_t h, int32_t t0, int32_t n) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  if (h->step_open) return fail(h, PIADMM_E_STATE, "a host-stepped MPC step is open: piadmm_step_finish first");
  if (n < 0 || t0 < 0 || t0 + (n > 0 ? n - 1 : 0) + h->cfg.H + 1 > h->T)
    return fail(h, PIADMM_E_ARG, "time index out of the reference trajectory");
  if (n == 0) return PIADMM_OK;    // nothing runs: the stored active sets and t_next stay as they are
  HIPCHK(h, hipSetDevice(h->cfg.device));
  if (int rc = continue_sequence(h, t0)) return rc;
  if ((h->comm || h->xfn) && !h->cap_synced)
    if (int rc = sync_step_cap(h)) return rc;
  for (int i = 0; i < n;) {
    const int k = std::min(h->step_cap, n - i);
    if (int rc = run_steps(h, t0 + i, k, i + k == n)) {
      h->t_next = -2;              // part of the sequence may have run: the next step forgets the sets
      return rc;
    }
    i += k;
  }
  h->t_next = t0 + n;              // only a sequence enqueued in full continues at t0 + n
  return PIADMM_OK;
}

}  // namespace

extern "C" {

int32_t piadmm_set_allreduce(piadmm_handle_t h, piadmm_allreduce_fn fn, void* ctx) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (h->comm && fn) return fail(h, PIADMM_E_STATE, "the handle already has an RCCL communicator");
  h->xfn = fn;
  h->xctx = ctx;
  h->cap_synced = false;
  return PIADMM_OK;
}

int32_t piadmm_mpc_steps_async(piadmm_handle_t h, int32_t t0, int32_t n_steps) {
  return enqueue_steps(h, t0, n_steps);
}

int32_t piadmm_sync(piadmm_handle_t h) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIADMM_OK;
}

// Host stepping of one MPC step, one outer iteration per call (SURVEY.md 8b piadmm_outer_iter):
// the state of casadi/main.py:78-181 after each iteration (pos_old, hat, lam and the PI
// accumulators S, D of ADMM_CVX_..._PI_antiwindup.m:160-188) is read with piadmm_get_state.
int32_t piadmm_outer_iter(piadmm_handle_t h, int32_t t, int32_t it, int32_t* stop_out) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  const piadmm_config_t& c = h->cfg;
  if (it < 0 || it >= c.max_outer) return fail(h, PIADMM_E_ARG, "it must be in [0, max_outer)");
  if (t < 0 || t + c.H + 1 > h->T) return fail(h, PIADMM_E_ARG, "time index out of the reference trajectory");
  if (it == 0) {
    HIPCHK(h, hipSetDevice(c.device));
    if (int rc = continue_sequence(h, t)) return rc;
    h->t_next = t + 1;
    h->step_open = true;
    h->step_t = t;
    h->step_flag = h->step_nanlast = h->step_stop = 0;
    h->ghist.assign((size_t)2 * c.max_outer, NAN);
  } else if (!h->step_open || t != h->step_t || it != h->step_it) {
    return fail(h, PIADMM_E_STATE, "outer_iter out of order: iterations of a step run 0, 1, 2, ...");
  } else if (h->step_stop) {
    return fail(h, PIADMM_E_STATE, "the step's stop rule already fired: piadmm_step_finish");
  }
  HIPCHK(h, hipSetDevice(c.device));
  hipStream_t s = h->stream;
  int stop = 0;
  if (c.term_global) {
    if (it == 0 && !h->a.graph) LAUNCH(h, pd::launch_pair_deff(h->a, s));
    if (int rc = global_iteration(h, t, it, h->step_flag, h->step_nanlast, &stop)) return rc;
    h->giters = it + 1;
  } else {
    // per-component stop: a component whose stop rule fired keeps its state (the kernels skip it)
    LAUNCH(h, launch_step(h->a, t, 1, it, it + 1, it == 0 ? pd::F_FIRST : 0, s));
    std::vector<int> cst((size_t)h->C * 4);
    HIPCHK(h, hipMemcpyAsync(cst.data(), h->a.cst, cst.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
    stop = 1;
    for (int ci = 0; ci < h->C; ++ci) stop &= cst[(size_t)ci * 4 + 3] != 0;
  }
  h->step_it = it + 1;
  h->step_stop = stop;
  if (stop_out) *stop_out = stop;
  return PIADMM_OK;
}

int32_t piadmm_step_finish(piadmm_handle_t h, double* xt_out, double* u_out) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->step_open) return fail(h, PIADMM_E_STATE, "no host-stepped MPC step is open");
  const piadmm_config_t& c = h->cfg;
  HIPCHK(h, hipSetDevice(c.device));
  hipStream_t s = h->stream;
  const int nit = h->step_it;
  int flags = pd::F_LAST;
  if (c.term_global) flags |= pd::F_GLOBAL | (h->step_nanlast ? pd::F_NANLAST : 0);
  LAUNCH(h, launch_step(h->a, h->step_t, 1, nit, nit, flags, s));
  h->step_open = false;
  const int N = h->N, H = c.H;
  if (int rc = download(h, xt_out, h->a.xt, (size_t)N * 3)) return rc;
  if (int rc = download(h, u_out, h->a.u, (size_t)N * H)) return rc;
  HIPCHK(h, hipStreamSynchronize(s));
  return PIADMM_OK;
}

int32_t piadmm_mpc_step(piadmm_handle_t h, int32_t t, double* xt_out, double* u_out, double* resid_out,
                        int32_t* iters_out, int32_t* status_out) {
  if (int rc = enqueue_steps(h, t, 1)) return rc;
  hipStream_t s = h->stream;
  const int N = h->N, E = h->E, C = h->C, H = h->cfg.H;
  int rc = 0;
  if ((rc = download(h, xt_out, h->a.xt, (size_t)N * 3)) || (rc = download(h, u_out, h->a.u, (size_t)N * H)) ||
      (rc = download(h, resid_out, h->a.resid, (size_t)C * h->cfg.max_outer * 2)) ||
      (rc = download(h, iters_out, h->a.iters, (size_t)C)) ||
      (rc = download(h, status_out, h->a.status, (size_t)N + E)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(s));
  return PIADMM_OK;
}

int32_t piadmm_time_steps(piadmm_handle_t h, int32_t t0, int32_t n_steps, float* ms_out) {
  if (!h || !ms_out) return fail(h, PIADMM_E_ARG, "null argument");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipEventRecord(h->ev0, h->stream));
  if (int rc = enqueue_steps(h, t0, n_steps)) return rc;
  HIPCHK(h, hipEventRecord(h->ev1, h->stream));
  HIPCHK(h, hipEventSynchronize(h->ev1));
  HIPCHK(h, hipEventElapsedTime(ms_out, h->ev0, h->ev1));
  return PIADMM_OK;
}

int32_t piadmm_comm_unique_id(uint8_t* id_out) {
  if (!id_out) return fail(nullptr, PIADMM_E_ARG, "null argument");
  ncclUniqueId id;
  ncclResult_t r = ncclGetUniqueId(&id);
  if (r != ncclSuccess) return fail(nullptr, PIADMM_E_HIP, std::string("ncclGetUniqueId: ") + ncclGetErrorString(r));
  std::memcpy(id_out, id.internal, NCCL_UNIQUE_ID_BYTES);
  return PIADMM_OK;
}

int32_t piadmm_comm_init(piadmm_handle_t h, const uint8_t* id_in, int32_t nranks, int32_t rank) {
  if (!h || !id_in) return fail(h, PIADMM_E_ARG, "null argument");
  if (nranks < 1 || rank < 0 || rank >= nranks) return fail(h, PIADMM_E_ARG, "bad rank / nranks");
  if (h->comm) return fail(h, PIADMM_E_STATE, "communicator already initialised");
  if (h->xfn) return fail(h, PIADMM_E_STATE, "the handle already has a host all-reduce transport");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  ncclUniqueId id;
  std::memcpy(id.internal, id_in, NCCL_UNIQUE_ID_BYTES);
  NCCLCHK(h, ncclCommInitRank(&h->comm, nranks, id, rank));
  h->nranks = nranks;
  h->rank = rank;
  h->cap_synced = false;
  return PIADMM_OK;
}

int32_t piadmm_global_resid(piadmm_handle_t h, double* resid_out, int32_t* iters_out) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->cfg.term_global) return fail(h, PIADMM_E_STATE, "term_global is off: residuals are per component");
  const int M = h->cfg.max_outer;
  if (resid_out) {
    for (int i = 0; i < 2 * M; ++i) resid_out[i] = NAN;
    for (int i = 0; i < 2 * h->giters && i < (int)h->ghist.size(); ++i) resid_out[i] = h->ghist[i];
  }
  if (iters_out) *iters_out = h->giters;
  return PIADMM_OK;
}

}  // extern "C"
