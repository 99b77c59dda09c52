// piadmm_capi.cpp -- C-ABI of libpiadmm (include/piadmm.h): the handle, its configuration, state up
// and down, counters and the near-tie log.  piadmm_ctx.h lists the other units.
//
// Replaces the reference's per-call CasADi/OSQP instantiation
// (casadi/main.py:96,146) and its Python loop state (casadi/main.py:52-72).
#include <cstdio>
#include <memory>

#include "piadmm_ctx.h"

namespace pd {
thread_local hipError_t g_launch_err = hipSuccess;
}

namespace {
thread_local std::string g_err;

int check_cfg(piadmm_ctx* h, const piadmm_config_t& c) {
  if (c.n_agents <= 0) return fail(h, PIADMM_E_ARG, "n_agents must be > 0");
  if (c.H < 3 || c.H > pd::HBIG) return fail(h, PIADMM_E_ARG, "H must be in [3, 63] in this version");
  if (c.max_outer <= 0) return fail(h, PIADMM_E_ARG, "max_outer must be > 0");
  if (c.dual_mode != PIADMM_DUAL_PLAIN && c.dual_mode != PIADMM_DUAL_PI && c.dual_mode != PIADMM_DUAL_PI_GLOBAL)
    return fail(h, PIADMM_E_ARG, "dual_mode must be 0 (plain), 1 (PI) or 2 (global PI)");
  if (c.dual_mode == PIADMM_DUAL_PI_GLOBAL && !(c.rho_min > 0 && c.rho_max >= c.rho_min && c.rho_num > 0))
    return fail(h, PIADMM_E_ARG, "global PI needs 0 < rho_min <= rho_max and rho_num > 0");
  if ((c.pi_trad != 0 && c.pi_trad != 1) || (c.ki_adapt != 0 && c.ki_adapt != 1))
    return fail(h, PIADMM_E_ARG, "pi_trad and ki_adapt must be 0 or 1");
  if ((c.pi_trad || c.ki_adapt) && c.dual_mode != PIADMM_DUAL_PI_GLOBAL)
    return fail(h, PIADMM_E_ARG, "pi_trad / ki_adapt select variants of the global PI law (dual_mode 2)");
  if (!std::isfinite(c.d_gain) || !std::isfinite(c.dual_init))
    return fail(h, PIADMM_E_ARG, "d_gain and dual_init must be finite");
  // ABI 7 made the back-calculation gain of the global PI law a field: a zero-initialised config
  // would silently drop the term of casadi_old_PI_ADMM/main.py:142 (d_gain 2) and of the adaptive
  // script (1), so 0 is refused rather than taken as a variant
  if (c.dual_mode == PIADMM_DUAL_PI_GLOBAL && c.d_gain == 0.0)
    return fail(h, PIADMM_E_ARG, "global PI needs d_gain != 0 (2.0: casadi_old_PI_ADMM, 1.0: the adaptive-gain script)");
  // warm_duals carries the previous step's shifted duals; dual_init sets every step's start
  // values -- the reference's scripts never combine the two (the first step would be ambiguous)
  if (c.warm_duals && c.dual_init != 0.0)
    return fail(h, PIADMM_E_ARG, "warm_duals and a nonzero dual_init are exclusive");
  if (!(c.dt > 0) || !(c.L > 0) || !(c.rho > 0) || !(c.Pcost > 0) || c.Pnorm < 0 || c.beta < 0)
    return fail(h, PIADMM_E_ARG, "dt, L, rho, Pcost must be > 0; Pnorm, beta >= 0");
  // !(x > 0) also refuses NaN; a non-finite bound, distance or tolerance has no valid solve (an
  // empty or unbounded box, a stop test that never or always fires)
  if (!(c.u_max > 0) || !(c.du_max > 0) || !(c.dis_thres > 0) || !std::isfinite(c.u_max) ||
      !std::isfinite(c.du_max) || !std::isfinite(c.dis_thres))
    return fail(h, PIADMM_E_ARG, "u_max, du_max, dis_thres must be > 0 and finite");
  if (!std::isfinite(c.eps_pri) || !std::isfinite(c.eps_dual))
    return fail(h, PIADMM_E_ARG, "eps_pri, eps_dual must be finite");
  if (c.windup && !(c.windup_sat > 0))
    return fail(h, PIADMM_E_ARG, "windup needs windup_sat > 0 (the saturation +-windup_sat)");
  if (c.max_inner <= 0 || c.polish_every <= 0) return fail(h, PIADMM_E_ARG, "max_inner, polish_every must be > 0");
  if (c.round_decimals < -1 || c.round_decimals > 12)
    return fail(h, PIADMM_E_ARG, "round_decimals must be in [-1, 12] (-1: no rounding)");
  if (c.tighten && !(c.tight_p > 0 && c.tight_p < 1)) return fail(h, PIADMM_E_ARG, "tight_p must be in (0, 1)");
  if (c.precision < 0 || c.precision > 2)
    return fail(h, PIADMM_E_ARG, "precision must be 0 (fp64), 1 (fp32 ADMM matrices) or 2 (fp32 x-step tables)");
  if (pd::lds_bytes(c.H, c.precision) + pd::STATIC_LDS > pd::MAX_LDS)
    return fail(h, PIADMM_E_ARG, "the workgroup's LDS exceeds 160 KB (precision 1 keeps the pair's fp32 "
                                  "K_s^-1 in LDS: H <= 55 in big mode)");
  return 0;
}
}  // namespace

int fail(piadmm_ctx* h, int code, const std::string& msg) {
  if (h) h->err = msg;
  g_err = msg;
  return code;
}

// Initial ADMM penalties (x-step: adapted by the OSQP rule and carried across steps; pair QPs
// keep this penalty: no adaptation, and on the GPU smaller fixed penalties cost more ADMM
// iterations on the bench's pair QPs -- 0.5x: +0%, 0.2x: +39%, 0.1x: +114% time).
int reset_penalties(piadmm_ctx* h) {
  const size_t N = h->N, E = h->E;
  h->rho_init.assign(std::max<size_t>(N, E) + 1, h->cfg.admm_rho);
  h->rho_pi_init.assign(E + 1, h->cfg.rho);
  HIPCHK(h, hipMemcpyAsync(h->a.rho_x, h->rho_init.data(), N * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (E) HIPCHK(h, hipMemcpyAsync(h->a.rho_e, h->rho_init.data(), E * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // global PI: every pair starts from the configured penalty (PI_ADMM_class.py:26, rho = 1)
  if (E && h->a.rho_pi)
    HIPCHK(h, hipMemcpyAsync(h->a.rho_pi, h->rho_pi_init.data(), E * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return 0;
}

extern "C" {

int32_t piadmm_abi_version(void) { return PIADMM_ABI_VERSION; }

const char* piadmm_build_info(void) {
  static char buf[160];
  std::snprintf(buf, sizeof(buf), "libpiadmm abi=%d arch=gfx950 hip=%d.%d waves/wg=%d hmax=%d (lds layout <= %d)",
                PIADMM_ABI_VERSION, HIP_VERSION_MAJOR, HIP_VERSION_MINOR, pd::NW, pd::HBIG, pd::HMAX);
  return buf;
}

int32_t piadmm_config_size(void) { return (int32_t)sizeof(piadmm_config_t); }

int32_t piadmm_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

const char* piadmm_last_error(piadmm_handle_t h) { return h ? h->err.c_str() : g_err.c_str(); }

int32_t piadmm_create(const piadmm_config_t* cfg, piadmm_handle_t* out) {
  if (!cfg || !out) return fail(nullptr, PIADMM_E_ARG, "null argument");
  *out = nullptr;
  // (owned until it is handed out: every refusal and failure below releases what was made)
  std::unique_ptr<piadmm_ctx> h(new piadmm_ctx());
  h->cfg = *cfg;
  if (h->cfg.admm_rho <= 0) h->cfg.admm_rho = 0.05;
  if (h->cfg.admm_sigma <= 0) h->cfg.admm_sigma = 1e-6;
  if (h->cfg.admm_alpha <= 0 || h->cfg.admm_alpha >= 2) h->cfg.admm_alpha = 1.6;
  if (h->cfg.qp_tol <= 0) h->cfg.qp_tol = 1e-9;
  // the configuration is judged before any device call: a refusal needs no GPU
  if (int rc = check_cfg(h.get(), h->cfg)) return rc;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd == 0) return fail(nullptr, PIADMM_E_NODEV, "no HIP device");
  if (cfg->device < 0 || cfg->device >= nd) return fail(nullptr, PIADMM_E_ARG, "device ordinal out of range");
  hipError_t e = hipSetDevice(cfg->device);
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&h->ev0);
  if (e == hipSuccess) e = hipEventCreate(&h->ev1);
  if (e == hipSuccess) e = h->h_part.make((size_t)std::max(cfg->max_outer, 1) * 5);
  if (e == hipSuccess) e = h->h_ctl.make(4);
  h->host_decide = knob_host_decide();
  if (e != hipSuccess) return fail(nullptr, PIADMM_E_HIP, std::string("HIP init: ") + hipGetErrorString(e));
  *out = h.release();
  return PIADMM_OK;
}

int32_t piadmm_destroy(piadmm_handle_t h) {
  if (!h) return PIADMM_OK;
  (void)hipSetDevice(h->cfg.device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  delete h;
  return PIADMM_OK;
}

int32_t piadmm_set_xt(piadmm_handle_t h, const double* xt) {
  if (!h || !xt) return fail(h, PIADMM_E_ARG, "null argument");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  h->step_open = false;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipMemcpyAsync(h->a.xt, xt, (size_t)h->N * 3 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  // a new state breaks the receding-horizon sequence: no label warm start for the next step
  HIPCHK(h, hipMemsetAsync(h->a.warm_ok, 0, (size_t)h->N * sizeof(int), h->stream));
  if (h->E) HIPCHK(h, hipMemsetAsync(h->a.gi_ws, 0, (size_t)h->E * (2 + pd::WAVE) * sizeof(int), h->stream));
  h->t_next = -1;
  // and no carried ADMM penalties: a run from a new state starts from the configured penalty
  // (the per-scenario caches stay: they are keyed by the penalty they were built for)
  if (int rc = reset_penalties(h)) return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIADMM_OK;
}

int32_t piadmm_get_state(piadmm_handle_t h, double* xt, double* u, double* pos_old, double* hat, double* lam,
                         double* S, double* D, uint8_t* edge_active, int32_t* iters) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  const int N = h->N, E = h->E, C = h->C, H = h->cfg.H, H1 = H + 1;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  const size_t pair_n = (size_t)E * 4 * H1;
  int rc = 0;
  if ((rc = download(h, xt, h->a.xt, (size_t)N * 3)) || (rc = download(h, u, h->a.u, (size_t)N * H)) ||
      (rc = download(h, pos_old, h->a.pos_old, (size_t)N * 2 * H1)) || (rc = download(h, hat, h->a.hat, pair_n)) ||
      (rc = download(h, lam, h->a.lam, pair_n)) || (rc = download(h, S, h->a.Sacc, pair_n)) ||
      (rc = download(h, D, h->a.Dacc, pair_n)) || (rc = download(h, edge_active, h->a.edge_active, (size_t)E)) ||
      (rc = download(h, iters, h->a.iters, (size_t)C)))
    return rc;
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIADMM_OK;
}

int32_t piadmm_n_components(piadmm_handle_t h) { return h && h->have_scn ? h->C : 0; }

int32_t piadmm_steps_per_launch(piadmm_handle_t h) {
  if (!h || !h->have_scn) return 0;
  if (h->xchg || h->split) return 1;
  if (h->cfg.term_global && !h->cfg.fixed_iters) return (h->coop && !h->comm && !h->xfn) ? h->step_cap : 1;
  return h->step_cap;
}

int32_t piadmm_get_counters(piadmm_handle_t h, uint64_t* out) {
  if (!h || !out) return fail(h, PIADMM_E_ARG, "null argument");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  std::vector<unsigned long long> buf((size_t)h->C * 8);
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipMemcpyAsync(buf.data(), h->a.counters, buf.size() * sizeof(buf[0]), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < 8; ++k) out[k] = 0;
  for (int c = 0; c < h->C; ++c)
    for (int k = 0; k < 8; ++k) out[k] += buf[(size_t)c * 8 + k];
  return PIADMM_OK;
}

int32_t piadmm_get_component_counters(piadmm_handle_t h, uint64_t* out, int32_t n) {
  if (!h || !out) return fail(h, PIADMM_E_ARG, "null argument");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  if (n < h->C * 8) return fail(h, PIADMM_E_ARG, "buffer too small");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipMemcpyAsync(out, h->a.counters, (size_t)h->C * 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIADMM_OK;
}

// Diagnostic builds only: per-component phase cycle sums, reset with the counters: C x 64 summed
// over the workgroup's waves, or (n >= C x 256) C x 4 x 64 per wave.
int32_t piadmm_debug_stamps(piadmm_handle_t h, uint64_t* out, int32_t n) {
  if (!h || !out) return fail(h, PIADMM_E_ARG, "null argument");
  if (!h->a.stamps) return fail(h, PIADMM_E_STATE, "library built without PIADMM_STAMPS");
  if (n < h->C * 64) return fail(h, PIADMM_E_ARG, "buffer too small");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  std::vector<uint64_t> raw((size_t)h->C * 64 * 4);
  HIPCHK(h, hipMemcpyAsync(raw.data(), h->a.stamps, raw.size() * sizeof(uint64_t), hipMemcpyDeviceToHost, h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  if (n >= h->C * 64 * 4) {
    std::copy(raw.begin(), raw.end(), out);
  } else {
    for (int ci = 0; ci < h->C; ++ci)
      for (int k = 0; k < 64; ++k) {
        uint64_t v = 0;
        for (int w = 0; w < 4; ++w) v += raw[((size_t)ci * 4 + w) * 64 + k];
        out[(size_t)ci * 64 + k] = v;
      }
  }
  return PIADMM_OK;
}

int32_t piadmm_set_tie_tolerance(piadmm_handle_t h, double tol) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!(tol >= 0.0) || !std::isfinite(tol)) return fail(h, PIADMM_E_ARG, "tie tolerance must be finite and >= 0");
  h->tie_tol = tol;
  h->a.tie_tol = tol;          // (the kernels take DevArgs by value: from the next launch on)
  h->a.tie_on = tol > 0.0 ? 1 : 0;
  return PIADMM_OK;
}

int32_t piadmm_get_near_ties(piadmm_handle_t h, uint64_t* counts, piadmm_near_tie_t* events, int32_t max_events,
                             int32_t* n_events) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  if (max_events < 0 || (max_events > 0 && !events)) return fail(h, PIADMM_E_ARG, "bad events / max_events");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  unsigned long long cnt[PIADMM_TIE_KINDS];
  unsigned long long nd = 0;
  HIPCHK(h, hipMemcpyAsync(cnt, h->a.tie_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipMemcpyAsync(&nd, h->a.tie_n, sizeof(nd), hipMemcpyDeviceToHost, s));
  HIPCHK(h, hipStreamSynchronize(s));
  const int kept = (int)std::min<unsigned long long>(nd, (unsigned long long)PIADMM_TIE_CAP);
  std::vector<int> ev((size_t)kept * 6);
  std::vector<double> mg((size_t)kept);
  if (kept > 0) {
    HIPCHK(h, hipMemcpyAsync(ev.data(), h->a.tie_ev, ev.size() * sizeof(int), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipMemcpyAsync(mg.data(), h->a.tie_mg, mg.size() * sizeof(double), hipMemcpyDeviceToHost, s));
    HIPCHK(h, hipStreamSynchronize(s));
  }
  if (counts)
    for (int k = 0; k < PIADMM_TIE_KINDS; ++k) counts[k] = cnt[k] + h->host_tie_cnt[k];
  int w = 0;
  for (int i = 0; i < kept && w < max_events; ++i, ++w) {
    piadmm_near_tie_t& o = events[w];
    o.step = ev[6 * i];
    o.iter = ev[6 * i + 1];
    o.kind = ev[6 * i + 2];
    o.id = ev[6 * i + 3];
    o.index = ev[6 * i + 4];
    o.reserved = 0;
    o.margin = mg[i];
  }
  for (size_t i = 0; i < h->host_ties.size() && w < max_events; ++i, ++w) events[w] = h->host_ties[i];
  if (n_events) *n_events = w;   // events written; the totals are the per-kind counts
  return PIADMM_OK;
}

int32_t piadmm_get_step_state(piadmm_handle_t h, double* xt, double* hat, double* lam, double* S, double* D,
                              double* last_hat, double* rho_pi) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  if (h->step_open) return fail(h, PIADMM_E_STATE, "a host-stepped MPC step is open: piadmm_step_finish first");
  const size_t N = h->N, E = h->E, H1 = h->cfg.H + 1;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  if (int rc = download(h, xt, h->a.xt, N * 3)) return rc;
  double* src[5] = {h->a.hat, h->a.lam, h->a.Sacc, h->a.Dacc, h->a.last};
  double* dst[5] = {hat, lam, S, D, last_hat};
  for (int k = 0; k < 5; ++k)
    if (int rc = download(h, dst[k], src[k], E * 4 * H1)) return rc;
  if (rho_pi && E) {
    if (h->a.rho_pi) {
      if (int rc = download(h, rho_pi, h->a.rho_pi, E)) return rc;
    } else
      for (size_t e = 0; e < E; ++e) rho_pi[e] = h->cfg.rho;
  }
  HIPCHK(h, hipStreamSynchronize(s));
  return PIADMM_OK;
}

int32_t piadmm_set_state(piadmm_handle_t h, const double* xt, const double* hat, const double* lam, const double* S,
                         const double* D, const double* last_hat, const double* rho_pi) {
  if (!h || !xt) return fail(h, PIADMM_E_ARG, "null argument (xt is required)");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  const size_t N = h->N, E = h->E, H1 = h->cfg.H + 1;
  for (size_t i = 0; i < 3 * N; ++i)
    if (!std::isfinite(xt[i])) return fail(h, PIADMM_E_ARG, "non-finite state");
  if (rho_pi)
    for (size_t e = 0; e < E; ++e)
      if (!(rho_pi[e] > 0.0) || !std::isfinite(rho_pi[e])) return fail(h, PIADMM_E_ARG, "rho_pi must be finite and > 0");
  {
    const double* pst[5] = {hat, lam, S, D, last_hat};
    for (int k = 0; k < 5; ++k)
      if (pst[k])
        for (size_t i = 0; i < E * 4 * H1; ++i)
          if (!std::isfinite(pst[k][i])) return fail(h, PIADMM_E_ARG, "non-finite pair state");
  }
  // xt, and a fresh receding-horizon sequence (labels, warm active sets, ADMM penalties)
  if (int rc = piadmm_set_xt(h, xt)) return rc;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  double* dst[5] = {h->a.hat, h->a.lam, h->a.Sacc, h->a.Dacc, h->a.last};
  const double* src[5] = {hat, lam, S, D, last_hat};
  for (int k = 0; k < 5 && E; ++k) {
    if (src[k]) HIPCHK(h, hipMemcpyAsync(dst[k], src[k], E * 4 * H1 * sizeof(double), hipMemcpyHostToDevice, s));
    else HIPCHK(h, hipMemsetAsync(dst[k], 0, E * 4 * H1 * sizeof(double), s));
  }
  if (h->a.rho_pi && E) {
    std::vector<double> r(rho_pi ? rho_pi : h->rho_pi_init.data(), (rho_pi ? rho_pi : h->rho_pi_init.data()) + E);
    HIPCHK(h, hipMemcpyAsync(h->a.rho_pi, r.data(), E * sizeof(double), hipMemcpyHostToDevice, s));
    HIPCHK(h, hipStreamSynchronize(s));
  }
  HIPCHK(h, hipStreamSynchronize(s));
  return PIADMM_OK;
}

int32_t piadmm_reset_counters(piadmm_handle_t h) {
  if (!h) return fail(nullptr, PIADMM_E_ARG, "null handle");
  if (!h->have_scn) return fail(h, PIADMM_E_STATE, "set_scenario first");
  HIPCHK(h, hipSetDevice(h->cfg.device));
  HIPCHK(h, hipMemsetAsync(h->a.counters, 0, (size_t)h->C * 8 * sizeof(uint64_t), h->stream));
  HIPCHK(h, hipMemsetAsync(h->a.tie_cnt, 0, PIADMM_TIE_KINDS * sizeof(unsigned long long), h->stream));
  HIPCHK(h, hipMemsetAsync(h->a.tie_n, 0, sizeof(unsigned long long), h->stream));
  h->host_ties.clear();
  for (auto& v : h->host_tie_cnt) v = 0;
  if (h->a.stamps) HIPCHK(h, hipMemsetAsync(h->a.stamps, 0, (size_t)h->C * 64 * 4 * sizeof(uint64_t), h->stream));
  HIPCHK(h, hipStreamSynchronize(h->stream));
  return PIADMM_OK;
}

}  // extern "C"
