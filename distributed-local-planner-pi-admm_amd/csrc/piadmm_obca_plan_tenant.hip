// piadmm_obca_plan_tenant.hip -- export and import of running tenants of the device-resident
// OBCA-ADMM plan (gfx950): k_plan_export and k_plan_import, launched by piadmm_obca_tenant_export /
// _import alone.  Pure copies; the launch sequence of the plan is in csrc/piadmm_obca_plan.hip.

#include "piadmm_obca_plan.h"

namespace obca_plan {

// ---------------------------------------------------------------------------------------------
// Export and import of running tenants (piadmm_obca_tenant_export / _import): a record per tenant
// that holds every per-scenario array of the plan (the layout: include/piadmm.h).  Pure copies;
// neither kernel is launched by any other entry point.
// ---------------------------------------------------------------------------------------------
// the fp64 section (doubles) up to the reference; WINDOW and, with a law, the integrator follow it
constexpr int TR_STATE = 0, TR_STATE_PREV = 556, TR_CTRL = 1112, TR_CTRL_PREV = 1140, TR_X = 1168, TR_LAMBDA = 1248,
              TR_PRIMAL = 1374, TR_PAR = 1378, TR_REF = 1394;
constexpr int TR_INTS = PIADMM_OBCA_TENANT_INTS;
// the int32 section
constexpr int TI_ITERS = 0, TI_STOP = 1, TI_CONV = 2, TI_PROB = 3, TI_MASK = 4, TI_WORK = 6, TI_CLOCK = 8;
static_assert(TR_STATE_PREV == STATE && TR_CTRL == 2 * STATE && TR_X == TR_CTRL + 2 * NCTRL && TR_LAMBDA == TR_X + NX &&
              TR_PRIMAL == TR_LAMBDA + 126 && TR_PAR == TR_PRIMAL + 4 && TR_REF == TR_PAR + TAB &&
              TR_REF + WIN == PIADMM_OBCA_TENANT_F64 && 4 * 126 + DPAR == PIADMM_OBCA_TENANT_F64_LAW &&
              TI_CLOCK + 3 <= TR_INTS && (TR_INTS * 4) % 16 == 0, "tenant record layout");
// the loop section (doubles), behind the law's: the three rows, the open step's latencies, the stream id
constexpr int TL_PLANT = 0, TL_NOISE = 16, TL_DELAY = 38, TL_TAU = 46, TL_STREAM = 48, TL_WORDS = PIADMM_OBCA_TENANT_F64_LOOP;
static_assert(TL_NOISE == FPAR && TL_DELAY == TL_NOISE + ZPAR && TL_TAU == TL_DELAY + YPAR && TL_STREAM == TL_TAU + 2 &&
              TL_STREAM + 2 == TL_WORDS && TL_WORDS % 2 == 0, "tenant record layout: the loop section");

// the plan's per-scenario arrays, by value.  S .. gains: only with a law (`law`); win, work, clk:
// nullptr without the clock / the order.  The strides are 0 where the plan shares one row.  l_*: only
// with the loop (`loop`, its flags); l_noise / l_delay nullptr where the kind is absent (export) or
// the plan shares one row (import, as l_plant and gains).
struct tenant_arrays {
  double *l_plant, *l_noise, *l_delay, *l_tau;
  long long* l_streams;
  int l_plant_s, l_noise_s, l_delay_s, loop;
  double *bar, *barp, *ctrl, *ctrlp, *X, *lamb, *primal, *dual, *pth, *dth, *tab, *ref, *win, *S, *D, *Sp, *Dp, *gains;
  int *iters, *stop, *conv, *prob, *mask, *work, *clk;
  int tab_stride, ref_stride, g_stride, n_ref, t_step, law, f64_words;
};

// One wave per tenant: record k of `blob` = scenario list[k] of the plan.  Nothing of the plan is
// written.
__global__ void __launch_bounds__(64 * PW) k_plan_export(const int* __restrict__ list, int m, tenant_arrays a,
                                                         double* __restrict__ blob) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= m) return;
  const size_t s = (size_t)__builtin_amdgcn_readfirstlane(list[k]);
  const int R = 10 * a.n_ref;
  double* rec = blob + (size_t)k * ((size_t)a.f64_words + TR_INTS / 2);
  copy_seg(rec + TR_STATE, a.bar + s * STATE, STATE, lane);
  copy_seg(rec + TR_STATE_PREV, a.barp + s * STATE, STATE, lane);
  copy_seg(rec + TR_CTRL, a.ctrl + s * NCTRL, NCTRL, lane);
  copy_seg(rec + TR_CTRL_PREV, a.ctrlp + s * NCTRL, NCTRL, lane);
  copy_seg(rec + TR_X, a.X + s * NX, NX, lane);
  copy_seg(rec + TR_LAMBDA, a.lamb + s * 126, 126, lane);
  if (lane < 4) {
    const double* one = lane == 0 ? a.primal : lane == 1 ? a.dual : lane == 2 ? a.pth : a.dth;
    rec[TR_PRIMAL + lane] = one[s];
  }
  copy_seg(rec + TR_PAR, a.tab + s * a.tab_stride, TAB, lane);
  const double* rf = a.ref + s * a.ref_stride;
  copy_seg(rec + TR_REF, rf, R, lane);
  double* W = rec + TR_REF + R;
  if (a.win) {
    copy_seg(W, a.win + s * WIN, WIN, lane);
  } else {
    // the window a clock attached now would build: the 8 rows at the plan's step
    const bool ok = a.t_step >= 0 && a.t_step + 8 <= a.n_ref;
    for (int i = lane; i < WIN; i += 64) W[i] = ok ? rf[((size_t)(i / 40) * a.n_ref + a.t_step) * 5 + i % 40] : 0.0;
  }
  if (a.law) {
    double* L = W + WIN;
    copy_seg(L, a.S + s * 126, 126, lane);
    copy_seg(L + 126, a.D + s * 126, 126, lane);
    copy_seg(L + 252, a.Sp + s * 126, 126, lane);
    copy_seg(L + 378, a.Dp + s * 126, 126, lane);
    copy_seg(L + 504, a.gains + s * a.g_stride, DPAR, lane);
  }
  if (a.loop) {
    double* Q = W + WIN + (a.law ? PIADMM_OBCA_TENANT_F64_LAW : 0);
    copy_seg(Q + TL_PLANT, a.l_plant + s * a.l_plant_s, FPAR, lane);
    if (a.l_noise) copy_seg(Q + TL_NOISE, a.l_noise + s * a.l_noise_s, ZPAR, lane);
    else if (lane < ZPAR) Q[TL_NOISE + lane] = 0.0;
    if (a.l_delay) copy_seg(Q + TL_DELAY, a.l_delay + s * a.l_delay_s, YPAR, lane);
    else if (lane < YPAR) Q[TL_DELAY + lane] = 0.0;
    copy_seg(Q + TL_TAU, a.l_tau + s * 2, 2, lane);
    if (lane < 2) Q[TL_STREAM + lane] = lane == 0 ? __longlong_as_double(a.l_streams[s]) : 0.0;
  }
  if (lane < TR_INTS) {
    int v = 0;
    if (lane == TI_ITERS) v = a.iters[s];
    else if (lane == TI_STOP) v = a.stop[s];
    else if (lane == TI_CONV) v = a.conv[s];
    else if (lane == TI_PROB) v = a.prob[s];
    else if (lane < TI_WORK) v = a.mask[2 * s + (lane - TI_MASK)];
    else if (lane < TI_CLOCK) v = a.work ? a.work[2 * s + (lane - TI_WORK)] : 0;
    else if (lane < TI_CLOCK + 3)
      v = a.clk ? a.clk[3 * s + (lane - TI_CLOCK)] : lane == TI_CLOCK ? a.t_step : lane == TI_CLOCK + 1 ? a.n_ref : 1;
    reinterpret_cast<int*>(rec + a.f64_words)[lane] = v;
  }
}

// One wave per tenant: scenario list[k] of the plan = record k of `blob`.  The host has checked the
// blob and that the plan has a row of everything per scenario; a.gains is nullptr where the plan
// shares one gains row (the record's was compared with it).  alive = (c + 8 <= len) is recomputed;
// k_plan_clock then rebuilds the flags, and the windows of the alive, over all n.
__global__ void __launch_bounds__(64 * PW) k_plan_import(const int* __restrict__ list, int m, tenant_arrays a,
                                                         const double* __restrict__ blob) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= m) return;
  const size_t s = (size_t)__builtin_amdgcn_readfirstlane(list[k]);
  const int R = 10 * a.n_ref;
  const double* rec = blob + (size_t)k * ((size_t)a.f64_words + TR_INTS / 2);
  copy_seg(a.bar + s * STATE, rec + TR_STATE, STATE, lane);
  copy_seg(a.barp + s * STATE, rec + TR_STATE_PREV, STATE, lane);
  copy_seg(a.ctrl + s * NCTRL, rec + TR_CTRL, NCTRL, lane);
  copy_seg(a.ctrlp + s * NCTRL, rec + TR_CTRL_PREV, NCTRL, lane);
  copy_seg(a.X + s * NX, rec + TR_X, NX, lane);
  copy_seg(a.lamb + s * 126, rec + TR_LAMBDA, 126, lane);
  if (lane < 4) {
    double* one = lane == 0 ? a.primal : lane == 1 ? a.dual : lane == 2 ? a.pth : a.dth;
    one[s] = rec[TR_PRIMAL + lane];
  }
  copy_seg(a.tab + s * a.tab_stride, rec + TR_PAR, TAB, lane);
  copy_seg(a.ref + s * a.ref_stride, rec + TR_REF, R, lane);
  const double* W = rec + TR_REF + R;
  copy_seg(a.win + s * WIN, W, WIN, lane);
  if (a.law) {
    const double* L = W + WIN;
    copy_seg(a.S + s * 126, L, 126, lane);
    copy_seg(a.D + s * 126, L + 126, 126, lane);
    copy_seg(a.Sp + s * 126, L + 252, 126, lane);
    copy_seg(a.Dp + s * 126, L + 378, 126, lane);
    if (a.gains) copy_seg(a.gains + s * a.g_stride, L + 504, DPAR, lane);
  }
  if (a.loop) {
    const double* Q = W + WIN + (a.law ? PIADMM_OBCA_TENANT_F64_LAW : 0);
    if (a.l_plant) copy_seg(a.l_plant + s * FPAR, Q + TL_PLANT, FPAR, lane);
    if (a.l_noise) copy_seg(a.l_noise + s * ZPAR, Q + TL_NOISE, ZPAR, lane);
    if (a.l_delay) copy_seg(a.l_delay + s * YPAR, Q + TL_DELAY, YPAR, lane);
    copy_seg(a.l_tau + s * 2, Q + TL_TAU, 2, lane);
    if (lane == 0) a.l_streams[s] = __double_as_longlong(Q[TL_STREAM]);
  }
  if (lane < TR_INTS) {
    const int* ri = reinterpret_cast<const int*>(rec + a.f64_words);
    const int v = ri[lane];
    if (lane == TI_ITERS) a.iters[s] = v;
    else if (lane == TI_STOP) a.stop[s] = v;
    else if (lane == TI_CONV) a.conv[s] = v;
    else if (lane == TI_PROB) a.prob[s] = v;
    else if (lane < TI_WORK) a.mask[2 * s + (lane - TI_MASK)] = v;
    else if (lane < TI_CLOCK) { if (a.work) a.work[2 * s + (lane - TI_WORK)] = v; }
    else if (lane < TI_CLOCK + 2) a.clk[3 * s + (lane - TI_CLOCK)] = v;
    else if (lane == TI_CLOCK + 2) a.clk[3 * s + 2] = ri[TI_CLOCK] + 8 <= ri[TI_CLOCK + 1] ? 1 : 0;
  }
}

}  // namespace obca_plan

using namespace obca_plan;

namespace {
// the fp64 words of a record of a plan with references of n_ref rows, with or without a law and the loop
int64_t tenant_f64(int n_ref, bool law, bool loop) {
  return (int64_t)PIADMM_OBCA_TENANT_F64 + 10 * (int64_t)n_ref + (law ? PIADMM_OBCA_TENANT_F64_LAW : 0) +
         (loop ? PIADMM_OBCA_TENANT_F64_LOOP : 0);
}
int64_t tenant_rec_bytes(int n_ref, bool law, bool loop) {
  return 8 * tenant_f64(n_ref, law, loop) + 4 * PIADMM_OBCA_TENANT_INTS;
}

obca_plan::tenant_arrays tenant_view(const piadmm_obca_plan_s* p) {
  obca_plan::tenant_arrays a{};
  a.bar = p->bar;  a.barp = p->barp;  a.ctrl = p->ctrl;  a.ctrlp = p->ctrlp;  a.X = p->X;  a.lamb = p->lamb;
  a.primal = p->primal;  a.dual = p->dual;  a.pth = p->pth;  a.dth = p->dth;  a.tab = p->tab;  a.ref = p->ref;
  a.win = p->ck.on ? p->ck.win : nullptr;
  a.S = p->du.S;  a.D = p->du.D;  a.Sp = p->du.Sp;  a.Dp = p->du.Dp;  a.gains = p->du.par;
  a.iters = p->iters;  a.stop = p->stop;  a.conv = p->conv;  a.prob = p->prob;  a.mask = p->mask;
  a.work = p->ord.on ? p->ord.work : nullptr;
  a.clk = p->ck.on ? p->ck.clk : nullptr;
  a.tab_stride = p->tab_stride;  a.ref_stride = p->ref_stride;  a.g_stride = p->du.stride;
  a.n_ref = p->cfg.n_ref;  a.t_step = p->t_step;  a.law = p->du.on ? 1 : 0;
  a.f64_words = (int)tenant_f64(p->cfg.n_ref, p->du.on, p->lp.on);
  a.loop = p->lp.on ? p->lp.flags : 0;
  a.l_plant = p->lp.plant;  a.l_plant_s = p->lp.plant_rows > 1 ? FPAR : 0;
  a.l_noise = p->lp.noise;  a.l_noise_s = p->lp.noise_rows > 1 ? ZPAR : 0;
  a.l_delay = p->lp.delay;  a.l_delay_s = p->lp.delay_rows > 1 ? YPAR : 0;
  a.l_tau = p->lp.tau;  a.l_streams = p->lp.streams;
  return a;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_tenant_export_bytes(piadmm_obca_t h, int32_t m, int64_t* bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_tenant_export_bytes")) return rc;
  if (m < 1 || m > p->n) return fail(h, PIADMM_E_ARG, "obca_tenant_export_bytes: 1 <= m <= n_scenarios");
  if (!bytes) return fail(h, PIADMM_E_ARG, "obca_tenant_export_bytes: null argument");
  *bytes = PIADMM_OBCA_TENANT_HEADER + (int64_t)m * tenant_rec_bytes(p->cfg.n_ref, p->du.on, p->lp.on);
  return 0;
}

int32_t piadmm_obca_tenant_export(piadmm_obca_t h, int32_t m, const int32_t* slots, void* blob, int64_t bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_tenant_export")) return rc;
  if (int rc = tenant_slots_check(h, p, m, slots, blob, "obca_tenant_export")) return rc;
  const int64_t rec_bytes = tenant_rec_bytes(p->cfg.n_ref, p->du.on, p->lp.on), body = (int64_t)m * rec_bytes;
  if (bytes != PIADMM_OBCA_TENANT_HEADER + body)
    return fail(h, PIADMM_E_ARG, "obca_tenant_export: the blob is " + std::to_string(PIADMM_OBCA_TENANT_HEADER + body) +
                " bytes, not " + std::to_string(bytes));
  if (p->fb.on) return fail(h, PIADMM_E_STATE, "obca_tenant_export: feedback is attached (the tenant record has no room for the tape)");
  if (p->dl.on) return fail(h, PIADMM_E_STATE, "obca_tenant_export: the delay is attached (the tenant record has no room for it)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_tenant_export: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  if (int rc = stage_ensure(h, p, (size_t)body, m)) return rc;
  int* d_list = reinterpret_cast<int*>(p->stg.buf + body);
  char* out = static_cast<char*>(blob);
  OWN_HIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_export, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, (const int*)d_list, m,
                     tenant_view(p), reinterpret_cast<double*>(p->stg.buf.get()));
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(out + PIADMM_OBCA_TENANT_HEADER, p->stg.buf, (size_t)body, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  const int32_t hdr[PIADMM_OBCA_TENANT_HEADER / 4] = {
      PIADMM_OBCA_TENANT_MAGIC, PIADMM_ABI_VERSION, m, p->cfg.n_ref, p->cfg.update_lamb_ij, p->du.on ? 1 : 0,
      p->ord.on ? 1 : 0, (int32_t)tenant_f64(p->cfg.n_ref, p->du.on, p->lp.on), PIADMM_OBCA_TENANT_INTS,
      (int32_t)rec_bytes, PIADMM_OBCA_TENANT_HEADER,
      // the loop: its flags, the seed (low, high) and k0; zeros without it
      p->lp.on ? p->lp.flags : 0, p->lp.on ? (int32_t)(uint32_t)p->lp.seed : 0,
      p->lp.on ? (int32_t)(uint32_t)(p->lp.seed >> 32) : 0, p->lp.on ? p->lp.k0 : 0, 0};
  std::memcpy(out, hdr, sizeof(hdr));
  return 0;
}

int32_t piadmm_obca_tenant_import(piadmm_obca_t h, int32_t m, const int32_t* slots, const void* blob, int64_t bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_tenant_import")) return rc;
  if (int rc = tenant_slots_check(h, p, m, slots, blob, "obca_tenant_import")) return rc;
  const int n = p->n, n_ref = p->cfg.n_ref;
  const char* in = static_cast<const char*>(blob);
  // the header against itself, then against the plan
  if (bytes < PIADMM_OBCA_TENANT_HEADER) return fail(h, PIADMM_E_ARG, "obca_tenant_import: the blob is shorter than its header");
  int32_t hdr[PIADMM_OBCA_TENANT_HEADER / 4];
  std::memcpy(hdr, in, sizeof(hdr));
  if (hdr[0] != PIADMM_OBCA_TENANT_MAGIC) return fail(h, PIADMM_E_ARG, "obca_tenant_import: bad magic (not a tenant blob)");
  if (hdr[1] != PIADMM_ABI_VERSION)
    return fail(h, PIADMM_E_ARG, "obca_tenant_import: the blob is of ABI " + std::to_string(hdr[1]));
  if (hdr[2] != m) return fail(h, PIADMM_E_ARG, "obca_tenant_import: the blob holds " + std::to_string(hdr[2]) + " tenants, not m");
  const bool law = hdr[5] == 1, order = hdr[6] == 1, loop = hdr[11] != 0;
  const bool loop_ok = hdr[15] == 0 && (loop ? (hdr[11] & 1) && !(hdr[11] & ~7) && hdr[14] >= 0
                                              : hdr[12] == 0 && hdr[13] == 0 && hdr[14] == 0);
  if (!loop_ok || hdr[3] < 8 || hdr[3] > (1 << 20) || (hdr[4] != 0 && hdr[4] != 1) || (hdr[5] != 0 && hdr[5] != 1) ||
      (hdr[6] != 0 && hdr[6] != 1) || hdr[10] != PIADMM_OBCA_TENANT_HEADER || hdr[8] != PIADMM_OBCA_TENANT_INTS ||
      (int64_t)hdr[7] != tenant_f64(hdr[3], law, loop) || (int64_t)hdr[9] != tenant_rec_bytes(hdr[3], law, loop))
    return fail(h, PIADMM_E_ARG, "obca_tenant_import: bad header (flags or section sizes)");
  const int64_t rec_bytes = hdr[9], body = (int64_t)m * rec_bytes;
  if (bytes != PIADMM_OBCA_TENANT_HEADER + body)
    return fail(h, PIADMM_E_ARG, "obca_tenant_import: the blob is " + std::to_string(PIADMM_OBCA_TENANT_HEADER + body) +
                " bytes, not " + std::to_string(bytes));
  if (hdr[3] != n_ref)
    return fail(h, PIADMM_E_ARG, "obca_tenant_import: n_ref mismatch (the blob " + std::to_string(hdr[3]) + ", the plan " +
                std::to_string(n_ref) + ")");
  if (hdr[4] != p->cfg.update_lamb_ij) return fail(h, PIADMM_E_ARG, "obca_tenant_import: update_lamb_ij mismatch");
  const uint64_t blob_seed = (uint64_t)(uint32_t)hdr[12] | ((uint64_t)(uint32_t)hdr[13] << 32);
  if (loop && p->lp.on) {
    if (hdr[11] != p->lp.flags)
      return fail(h, PIADMM_E_ARG, "obca_tenant_import: the loop's row kinds differ (the blob " + std::to_string(hdr[11]) +
                  ", the plan " + std::to_string(p->lp.flags) + ")");
    if (blob_seed != p->lp.seed || hdr[14] != p->lp.k0)
      return fail(h, PIADMM_E_ARG, "obca_tenant_import: the loop's seed or k0 differ from the plan's");
  }
  // the records: what the kernels rely on (the rows, prob, the clocks)
  const size_t F = (size_t)hdr[7];
  const size_t law_at = (size_t)PIADMM_OBCA_TENANT_F64 + 10 * (size_t)n_ref;
  const size_t loop_at = law_at + (law ? PIADMM_OBCA_TENANT_F64_LAW : 0);
  auto rec_f64 = [&](int k, size_t word, double* dst, int count) {
    std::memcpy(dst, in + PIADMM_OBCA_TENANT_HEADER + (size_t)k * rec_bytes + 8 * word, sizeof(double) * (size_t)count);
  };
  std::vector<int32_t> ints((size_t)m * TR_INTS);
  std::vector<int> admm((size_t)m);
  for (int k = 0; k < m; ++k) {
    const std::string row = "obca_tenant_import: row " + std::to_string(k) + ": ";
    double par[TAB];
    rec_f64(k, TR_PAR, par, TAB);
    if (const char* why = row_check(par)) return fail(h, PIADMM_E_ARG, row + why);
    admm[(size_t)k] = (int)par[T_ADMM];
    int32_t* ri = ints.data() + (size_t)k * TR_INTS;
    std::memcpy(ri, in + PIADMM_OBCA_TENANT_HEADER + (size_t)k * rec_bytes + 8 * F, sizeof(int32_t) * TR_INTS);
    if (ri[TI_PROB] != 0 && ri[TI_PROB] != 1) return fail(h, PIADMM_E_ARG, row + "prob must be 0 or 1");
    if (ri[TI_CLOCK] < 0) return fail(h, PIADMM_E_ARG, row + "c >= 0");
    if (ri[TI_CLOCK + 1] < 8 || ri[TI_CLOCK + 1] > n_ref) return fail(h, PIADMM_E_ARG, row + "8 <= len <= n_ref");
    if (law) {
      double g[DPAR];
      rec_f64(k, law_at + 504, g, DPAR);
      if (const char* why = dual_row_check(g)) return fail(h, PIADMM_E_ARG, row + "gains: " + why);
    }
    if (loop) {
      double q[TL_WORDS];
      rec_f64(k, loop_at, q, TL_WORDS);
      if (const char* why = feedback_row_check(q + TL_PLANT)) return fail(h, PIADMM_E_ARG, row + "plant: " + why);
      if (const char* why = noise_row_check(q + TL_NOISE)) return fail(h, PIADMM_E_ARG, row + "noise: " + why);
      if (const char* why = delay_row_check(q + TL_DELAY)) return fail(h, PIADMM_E_ARG, row + "delay: " + why);
      for (int v = 0; v < 2; ++v)
        if (!(q[TL_TAU + v] >= 0.0 && q[TL_TAU + v] <= PLANT_DT)) return fail(h, PIADMM_E_ARG, row + "tau must be in [0, DT]");
      int64_t stream;
      std::memcpy(&stream, q + TL_STREAM, sizeof(stream));
      if (stream < 0) return fail(h, PIADMM_E_ARG, row + "the stream id must be >= 0");
      if ((int64_t)hdr[14] + ri[TI_CLOCK] >= ((int64_t)1 << 31) && ri[TI_CLOCK] + 8 <= ri[TI_CLOCK + 1])
        return fail(h, PIADMM_E_ARG, row + "loop step index exhausted");
    }
  }
  // the destination
  if (p->fb.on) return fail(h, PIADMM_E_STATE, "obca_tenant_import: feedback is attached (the tenant record has no room for the tape)");
  if (p->dl.on) return fail(h, PIADMM_E_STATE, "obca_tenant_import: the delay is attached (the tenant record has no room for it)");
  if (!p->ck.on) return fail(h, PIADMM_E_STATE, "obca_tenant_import: no clock attached (obca_clock_plan)");
  if (p->tr.on) return fail(h, PIADMM_E_STATE, "obca_tenant_import: a trace is attached (its minima would mix two tenants)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_tenant_import: only at a step boundary (an MPC step is open)");
  if (p->ref_rows != n || p->tab_rows != n)
    return fail(h, PIADMM_E_STATE, "obca_tenant_import: needs a plan with a reference and a parameter row per scenario (obca_fleet_begin)");
  if (law != p->du.on)
    return fail(h, PIADMM_E_STATE, law ? "obca_tenant_import: the blob carries a dual law, the plan has none attached"
                                        : "obca_tenant_import: the plan has a dual law attached, the blob carries none");
  if (loop != p->lp.on)
    return fail(h, PIADMM_E_STATE, loop ? "obca_tenant_import: the blob carries the loop, the plan has none attached"
                                         : "obca_tenant_import: the plan has the loop attached, the blob carries none");
  if (order != p->ord.on)
    return fail(h, PIADMM_E_STATE, order ? "obca_tenant_import: the blob carries the order's record, the plan has no order attached"
                                          : "obca_tenant_import: the plan has the order attached, the blob carries no record");
  if (const char* why = ledger_replace_refusal(p, m, slots, false))
    return fail(h, PIADMM_E_STATE, std::string("obca_tenant_import: ") + why);
  OWN_HIP(h, hipSetDevice(h->device));
  const bool gains_travel = law && p->du.rows == n;
  if (law && !gains_travel) {
    // one shared gains row: a read of 8 doubles, nothing is written
    double shared[DPAR], g[DPAR];
    OWN_HIP(h, hipMemcpyAsync(shared, p->du.par, sizeof(shared), hipMemcpyDeviceToHost, h->stream));
    OWN_HIP(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < m; ++k) {
      rec_f64(k, law_at + 504, g, DPAR);
      if (std::memcmp(g, shared, sizeof(g)) != 0)
        return fail(h, PIADMM_E_ARG, "obca_tenant_import: row " + std::to_string(k) +
                    ": the gains row differs from the plan's shared one");
    }
  }
  if (loop) {
    // a shared row of a kind: a read of that one row, nothing is written
    const struct { const double* dev; int rows, at, width; const char* kind; } kinds[3] = {
        {p->lp.plant, p->lp.plant_rows, TL_PLANT, FPAR, "plant"},
        {p->lp.noise, (p->lp.flags & 2) ? p->lp.noise_rows : n, TL_NOISE, ZPAR, "noise"},
        {p->lp.delay, (p->lp.flags & 4) ? p->lp.delay_rows : n, TL_DELAY, YPAR, "delay"}};
    for (const auto& kd : kinds) {
      if (kd.rows == n) continue;
      double shared[ZPAR], g[ZPAR];
      OWN_HIP(h, hipMemcpyAsync(shared, kd.dev, sizeof(double) * (size_t)kd.width, hipMemcpyDeviceToHost, h->stream));
      OWN_HIP(h, hipStreamSynchronize(h->stream));
      for (int k = 0; k < m; ++k) {
        rec_f64(k, loop_at + (size_t)kd.at, g, kd.width);
        if (std::memcmp(g, shared, sizeof(double) * (size_t)kd.width) != 0)
          return fail(h, PIADMM_E_ARG, "obca_tenant_import: row " + std::to_string(k) + ": the " + kd.kind +
                      " row differs from the plan's shared one");
      }
    }
  }
  if (int rc = stage_ensure(h, p, (size_t)body, m)) return rc;
  if (p->lg.on) {
    // the tenants that leave: their records, before k_plan_import overwrites their slots
    if (int rc = ledger_close(h, p, m, slots, 3, false)) return rc;
  }
  int* d_list = reinterpret_cast<int*>(p->stg.buf + body);
  OWN_HIP(h, hipMemcpyAsync(p->stg.buf, in + PIADMM_OBCA_TENANT_HEADER, (size_t)body, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  tenant_arrays a = tenant_view(p);
  if (!gains_travel) a.gains = nullptr;
  if (p->lp.plant_rows != n) a.l_plant = nullptr;
  if (!(p->lp.flags & 2) || p->lp.noise_rows != n) a.l_noise = nullptr;
  if (!(p->lp.flags & 4) || p->lp.delay_rows != n) a.l_delay = nullptr;
  hipLaunchKernelGGL(k_plan_import, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, (const int*)d_list, m, a,
                     reinterpret_cast<const double*>(p->stg.buf.get()));
  OWN_HIP(h, hipGetLastError());
  // what an admission does next: the rows' largest max_admm_iter, the mirror, the windows, flags and list
  for (int k = 0; k < m; ++k) {
    const size_t s = (size_t)slots[k];
    const int32_t* ri = ints.data() + (size_t)k * TR_INTS;
    p->admm_rows[s] = admm[(size_t)k];
    int* k3 = p->ck.host.data() + 3 * s;
    k3[0] = ri[TI_CLOCK];
    k3[1] = ri[TI_CLOCK + 1];
    k3[2] = k3[0] <= k3[1] - 8 ? 1 : 0;
  }
  if (int rc = clock_relist(h, p)) return rc;
  if (p->lp.on) {
    // as after an admission: an alive tenant's latency is the draw at its clock, whatever the record
    // held; a retired tenant keeps the record's
    if (int rc = loop_open(h, p, p->ck.n_list)) {
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    OWN_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (p->lg.on) {
    // an imported tenant starts a fresh record (the blob carries none); a retired one holds no tenant
    if (int rc = ledger_open(h, p, m, slots)) return rc;
  }
  return 0;
}

}  // extern "C"
