// piadmm_scenario.cpp -- set_scenario (C-ABI of libpiadmm, piadmm_ctx.h): the arguments are checked,
// the candidate graph is partitioned (pd_partition.h), the scenario's device arrays are allocated in
// the handle's arena and the host's arrays are uploaded.
#include "pd_partition.h"
#include "piadmm_ctx.h"

namespace {

// the arguments of one set_scenario call (shard arrays null: not a sharded job)
struct scn_args {
  const double *spd, *xt0, *ref;
  int32_t T;
  const int32_t* edges;
  int32_t n_edges;
  const uint8_t* owned;
  const int32_t* slot;
  int32_t n_slots;
  const uint8_t* counted;
};

// the scenario's read-only device arrays while they are filled (DevArgs holds them as const)
struct scn_dev {
  double *spd, *ref;
  int *cp, *ce, *ed, *nb;
  int *scp = nullptr, *sel = nullptr;                    // split
  int* g[7] = {};                                        // graph: aptr, alist, eptr, elist, nptr, nedge, ndir
  unsigned char *owned = nullptr, *counted = nullptr;    // sharded
  int* xslot = nullptr;
};

// Stage 1: what is refused before the handle is touched (the old scenario stays usable).
int check_args(piadmm_ctx* h, const scn_args& s) {
  if (!s.spd || !s.xt0 || !s.ref || (s.n_edges > 0 && !s.edges)) return fail(h, PIADMM_E_ARG, "null array");
  if (s.T < h->cfg.H + 1) return fail(h, PIADMM_E_ARG, "reference too short: T < H+1");
  if (s.n_edges < 0) return fail(h, PIADMM_E_ARG, "n_edges < 0");
  if (const char* why = pd::check_graph_args(h->cfg.n_agents, s.edges, s.n_edges, s.owned, s.slot, s.n_slots,
                                             s.counted, h->cfg.term_global != 0, s.spd, s.xt0))
    return fail(h, PIADMM_E_ARG, why);
  return 0;
}

// One zero-filled array of the scenario's arena, of the pointer's own element type.
template <typename T>
void take(piadmm_ctx* h, T*& p, size_t n) {
  p = h->scn.take<T>(n, true);
}

// Stage 3a: the arrays every scenario has.  The takes are sticky: h->scn.rc is asked once, by the caller.
void allocate_common(piadmm_ctx* h, const scenario_knobs& k, scn_dev& d) {
  pd::DevArgs& A = h->a;
  const int N = h->N, H = h->cfg.H, T = h->T;
  const size_t H1 = H + 1, E = h->E, C = h->C;
  take(h, d.spd, N);
  take(h, d.ref, (size_t)N * 2 * T);
  take(h, d.cp, C + 1);
  take(h, d.ce, C);
  take(h, d.ed, 2 * E);
  take(h, d.nb, N);
  take(h, A.xt, (size_t)N * 3);
  take(h, A.u, (size_t)N * H);
  take(h, A.pos_old, (size_t)N * 2 * H1);
  take(h, A.hat, E * 4 * H1);
  take(h, A.lam, E * 4 * H1);
  take(h, A.edge_active, E);
  take(h, A.iters, C);
  // one residual-history slot per step of a persistent multi-step launch (<= 32 steps,
  // <= 64 MB of history per launch)
  {
    const size_t per_step = (size_t)C * std::max(h->cfg.max_outer, 1) * 2 * sizeof(double);
    h->step_cap = (int)std::max<size_t>(1, std::min<size_t>(32, ((size_t)64 << 20) / per_step));
  }
  take(h, A.resid, (size_t)h->step_cap * C * h->cfg.max_outer * 2);
  take(h, A.status, (size_t)N + E);
  take(h, A.Pinv_x, (size_t)N * H * H);
  take(h, A.sc_x, (size_t)N * 4 * pd::HCAP);
  take(h, A.lab_x, (size_t)N * 2 * pd::HCAP);
  const bool big = H > pd::HMAX || A.graph;   // graph mode: the big-mode HBM layout at every H
  take(h, A.Gx_g, big ? (size_t)N * (H * H + H) : 1);
  take(h, A.XT_g, big ? (size_t)N * H1 * pd::XLDG : 1);
  A.ke_stride = A.graph ? std::max(4 * H * H, 2 * H * pd::WAVE) : 4 * H * H;
  take(h, A.Ke_g, big ? E * A.ke_stride : 1);
  take(h, A.Yx_g, big ? (size_t)N * pd::WAVE * H : 1);
  if (h->cfg.precision == 2 && big) take(h, A.T32_g, (size_t)N * (H * H + H * pd::XLDG));
  take(h, A.tab_e, E * 8 * H * H);
  take(h, A.warm_ok, (size_t)N);
  take(h, A.Sacc, E * 4 * H1);
  take(h, A.Dacc, E * 4 * H1);
  take(h, A.last, E * 4 * H1);
  take(h, A.dischk, E);
  take(h, A.deff, E);
  take(h, A.qs_x, (size_t)N * 5 * pd::WAVE);
  take(h, A.ql_x, (size_t)N * 2 * pd::WAVE);
  take(h, A.qs_e, E * 12 * pd::WAVE);
  take(h, A.ql_e, E * 5 * pd::WAVE);
  take(h, A.cst, C * 4);
  take(h, h->d_part, std::max<size_t>(33, (size_t)h->cfg.max_outer * std::max(5, 2 * h->step_cap)));
  take(h, A.counters, C * 8);
  take(h, A.rho_x, (size_t)N);
  take(h, A.rho_e, E);
  take(h, A.Kx_cache, (size_t)N * H * H);
  take(h, A.xcache_rho, (size_t)N);
  take(h, A.ecache, E);
  take(h, A.gi_ws, E * (2 + pd::WAVE));
  // the wide dual active set's scratch (pair working sets beyond 63 rows, H >= 32): one region
  // per wave that solves pair QPs -- the graph kernel's GW waves, the fused kernel's pair wave
  A.gi_wide_stride = pd::giw_stride(H);
  // (over 8 GB -- hundreds of thousands of components at H >= 32 -- the wide path is off: such
  // saturated pair QPs are then reported PIADMM_QP_INEXACT, as before it existed)
  if (E > 0 && A.pair_gi && 2 * H > pd::WAVE - 1) {
    const size_t wide_n = C * (A.graph ? pd::GW : 1) * A.gi_wide_stride;
    if (wide_n * sizeof(double) <= ((size_t)8 << 30)) take(h, A.gi_wide, wide_n);
  }
  // graph mode: each pair's last dual active set (S^-1 and Y columns) for its next solve in the
  // same MPC step (pd_qp.h gi_snap_restore); PIADMM_PAIR_SNAP=0 appends the rows again instead
  {
    const size_t snap_n = E * ((size_t)pd::WAVE * pd::WAVE + (size_t)pd::WAVE * 2 * H + pd::WAVE);
    if (A.graph && E > 0 && A.pair_gi && k.pair_snap && snap_n * sizeof(double) <= ((size_t)8 << 30))
      take(h, A.gi_snap, snap_n);
  }
  take(h, A.gpart, (size_t)2 * C * 5);
  take(h, A.gbar, (size_t)C);
  take(h, A.ghist, (size_t)h->step_cap * std::max(h->cfg.max_outer, 1) * 2);
  take(h, A.giters, (size_t)h->step_cap);
  take(h, A.gctl, 4);
  take(h, A.tie_cnt, PIADMM_TIE_KINDS);
  take(h, A.tie_n, 1);
  take(h, A.tie_ev, (size_t)PIADMM_TIE_CAP * 6);
  take(h, A.tie_mg, (size_t)PIADMM_TIE_CAP);
  A.tie_cap = PIADMM_TIE_CAP;
  A.tie_tol = h->tie_tol;
  A.tie_on = h->tie_tol > 0.0 ? 1 : 0;
}

// Stage 3b: the arrays of a split component, of graph mode and of a sharded job.
void allocate_modes(piadmm_ctx* h, const pd::Partition& P, bool sharded, scn_dev& d) {
  pd::DevArgs& A = h->a;
  const int N = h->N;
  const size_t H1 = h->cfg.H + 1, E = h->E, C = h->C;
  if (h->split) {
    take(h, A.eterm, E * 2);
    take(h, d.scp, P.sum_cptr.size());
    take(h, d.sel, E);
  }
  if (A.graph) {
    const size_t n7[7] = {C + 1, (size_t)N, C + 1, E, (size_t)N + 1, 2 * E, 2 * E};
    for (int j = 0; j < 7; ++j) take(h, d.g[j], n7[j]);
    take(h, A.seed_g, (size_t)N * 2);
    take(h, A.eres, E * 2);
    take(h, A.cpart, C * 5);
    take(h, A.csig_x, (size_t)N * pd::WAVE);
    take(h, A.xflags, (size_t)N);
    take(h, A.eflags, E);
    if (h->cfg.dual_mode == PIADMM_DUAL_PI_GLOBAL) {
      take(h, A.rho_pi, E);
      take(h, A.xcache_coef, (size_t)N);
      take(h, A.ecache_rho, E);
    }
  }
  if (sharded) {
    take(h, d.owned, (size_t)N);
    take(h, d.counted, E);
    take(h, d.xslot, (size_t)N);
  }
  if (h->xchg) {
    take(h, A.xbuf, (size_t)h->n_slots * 3 * H1);
    take(h, h->d_xrecv, (size_t)h->n_slots * 3 * H1);
  }
#ifdef PIADMM_STAMPS
  take(h, A.stamps, C * 64 * 4);     // per component and wave (pd_common.h STAMP_WAVES)
#endif
}

// n elements of the host's src to device array dst on the handle's stream (src outlives the copy)
template <typename T>
int upload_n(piadmm_ctx* h, T* dst, const T* src, size_t n) {
  if (n) HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyHostToDevice, h->stream));
  return 0;
}

// Stage 4: the host's arrays to the device, and DevArgs' pointers to them.
int upload(piadmm_ctx* h, const scn_args& s, pd::Partition& P, const scn_dev& d) {
  pd::DevArgs& A = h->a;
  const size_t N = h->N, E = h->E, C = h->C;
  int rc = 0;
  if ((rc = upload_n(h, d.spd, s.spd, N)) || (rc = upload_n(h, d.ref, s.ref, N * 2 * h->T)) ||
      (rc = upload_n(h, d.cp, h->comp_ptr.data(), C + 1)) || (rc = upload_n(h, d.ce, h->comp_edge.data(), C)) ||
      (rc = upload_n(h, d.ed, s.edges, 2 * E)) || (rc = upload_n(h, d.nb, P.nbr.data(), N)) ||
      (rc = upload_n(h, A.xt, s.xt0, N * 3)))
    return rc;
  h->graph_host.clear();
  if (A.graph) {
    h->graph_host = {std::move(P.aptr), std::move(P.alist), std::move(P.eptr), std::move(P.elist),
                     std::move(P.nptr), std::move(P.nedge), std::move(P.ndir)};   // outlive the copies
    for (int j = 0; j < 7; ++j)
      if ((rc = upload_n(h, d.g[j], h->graph_host[j].data(), h->graph_host[j].size()))) return rc;
    A.comp_aptr = d.g[0];
    A.comp_alist = d.g[1];
    A.comp_eptr = d.g[2];
    A.comp_elist = d.g[3];
    A.nbr_ptr = d.g[4];
    A.nbr_edge = d.g[5];
    A.nbr_dir = d.g[6];
  }
  if (h->split) {
    h->graph_host.push_back(std::move(P.sum_cptr));
    h->graph_host.push_back(std::move(P.sum_pos));
    const auto& hc = h->graph_host[h->graph_host.size() - 2];
    const auto& he = h->graph_host.back();
    if ((rc = upload_n(h, d.scp, hc.data(), hc.size())) || (rc = upload_n(h, d.sel, he.data(), he.size()))) return rc;
    A.sum_cptr = d.scp;
    A.sum_pos = d.sel;
    A.sum_C = (int)hc.size() - 1;
  }
  if (s.owned) {
    h->shard_host.assign(s.owned, s.owned + N);
    h->shard_host.insert(h->shard_host.end(), s.counted, s.counted + E);
    h->graph_host.push_back(std::vector<int>(s.slot, s.slot + N));
    if ((rc = upload_n(h, d.owned, h->shard_host.data(), N)) ||
        (rc = upload_n(h, d.counted, h->shard_host.data() + N, E)) ||
        (rc = upload_n(h, d.xslot, h->graph_host.back().data(), N)))
      return rc;
    A.owned = d.owned;
    A.counted = d.counted;
    A.xslot = d.xslot;
    A.xrecv = h->d_xrecv;
    A.n_slots = h->n_slots;
  }
  if ((rc = reset_penalties(h))) return rc;
  HIPCHK(h, hipMemsetAsync(A.xcache_rho, 0xff, N * sizeof(double), h->stream));   // NaN: no cache
  if (A.xcache_coef) HIPCHK(h, hipMemsetAsync(A.xcache_coef, 0xff, N * sizeof(double), h->stream));
  if (A.ecache_rho && E) HIPCHK(h, hipMemsetAsync(A.ecache_rho, 0xff, E * sizeof(double), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  A.spd = d.spd;
  A.ref = d.ref;
  A.comp_ptr = d.cp;
  A.comp_edge = d.ce;
  A.edges = d.ed;
  A.nbr_cnt = d.nb;
  return 0;
}

// check -> partition -> allocate -> upload.  The old scenario's arrays go before the new ones are
// allocated (peak memory); a device failure after that leaves the handle without a scenario.
int32_t set_scenario_impl(piadmm_ctx* h, const scn_args& s) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (int rc = check_args(h, s)) return rc;
  const piadmm_config_t& c = h->cfg;
  const scenario_knobs k = read_scenario_knobs();
  const bool sharded = s.owned != nullptr;
  pd::Partition P = pd::partition(c.n_agents, s.edges, s.n_edges, sharded, sharded && s.n_slots > 0,
                                  c.dual_mode == PIADMM_DUAL_PI_GLOBAL, c.no_collision_gate != 0,
                                  c.dual_init != 0.0, c.term_global != 0, k.force_graph, k.block);
  HIPCHK(h, hipSetDevice(c.device));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  h->release_scenario();
  h->step_open = false;
  h->cap_synced = false;
  h->split = P.split;
  h->comp_ptr = std::move(P.comp_ptr);
  h->comp_edge = std::move(P.comp_edge);
  h->N = c.n_agents;
  h->E = s.n_edges;
  h->C = P.C;
  h->T = s.T;
  h->xchg = sharded && s.n_slots > 0;
  h->n_slots = h->xchg ? s.n_slots : 0;
  pd::DevArgs& A = h->a;
  A = pd::DevArgs{};
  A.cfg = c;
  A.pair_gi = k.pair_gi;
  A.pair_warm = k.pair_warm;
  A.x_gi = k.x_gi;
  A.no_spec = k.no_spec;
  A.N = h->N;
  A.E = h->E;
  A.C = h->C;
  A.T = h->T;
  A.graph = P.simple ? 0 : 1;
  scn_dev d;
  allocate_common(h, k, d);
  allocate_modes(h, P, sharded, d);
  if (h->scn.rc) return h->scn.rc;
  if (int rc = upload(h, s, P, d)) return rc;
  // natural global termination without a communicator (one rank): the stop test in-kernel
  // behind a grid barrier, when every workgroup can be resident (cooperative launch);
  // PIADMM_NO_COOP=1 keeps the host-decided path (one launch per outer iteration, the path
  // every rank of a sharded job takes, with the RCCL all-reduce) for tests and comparisons
  h->coop = c.term_global && !c.fixed_iters && !k.no_coop && !h->xchg && !h->split &&
            (A.graph ? pd::graph_coop_fits(A, c.device) : pd::coop_fits(A, c.device));
  (void)hipGetLastError();   // a refused query must not surface as the next launch's error
  h->have_scn = true;
  h->t_next = -1;
  return PIADMM_OK;
}

}  // namespace

extern "C" {

int32_t piadmm_set_scenario(piadmm_handle_t h, const double* spd, const double* xt0, const double* ref,
                            int32_t T, const int32_t* edges, int32_t n_edges) {
  return set_scenario_impl(h, {spd, xt0, ref, T, edges, n_edges, nullptr, nullptr, 0, nullptr});
}

int32_t piadmm_set_scenario_shard(piadmm_handle_t h, const double* spd, const double* xt0, const double* ref,
                                  int32_t T, const int32_t* edges, int32_t n_edges, const uint8_t* owned,
                                  const int32_t* slot, int32_t n_slots, const uint8_t* counted) {
  if (!owned) return fail(h, PIADMM_E_ARG, "shard: null owned");
  return set_scenario_impl(h, {spd, xt0, ref, T, edges, n_edges, owned, slot, n_slots, counted});
}

}  // extern "C"
