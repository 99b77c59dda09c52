// piadmm_obca_plan_attach.hip -- the attachments of the device-resident OBCA-ADMM plan that change
// what an iterate or a shift launches: the PI anti-windup dual law, the longest-first order and the
// per-scenario clocks (gfx950).  csrc/piadmm_obca_plan.hip describes the launch sequence; of it:
// With a dual law attached (piadmm_obca_dual_plan) k_plan_dual_pi runs between k_obca_edge and
// k_plan_residual and k_plan_dual_shift after k_plan_shift; without one neither is launched.
// With the longest-first order attached (piadmm_obca_order_plan) k_plan_work runs after k_obca_edge
// and k_plan_order after k_plan_compact and after k_plan_shift: the record order of a launch is then
// the scenarios by the work of their last solves, a pure function of that record, the same on
// every run; without it neither is launched.
// With per-scenario clocks attached (piadmm_obca_clock_plan) k_plan_pack_local reads each scenario's
// own 8 reference rows from a window, piadmm_obca_plan_shift runs k_plan_shift_list /
// k_plan_dual_shift_list on the scenarios the step ran and then k_plan_clock (their tick, the alive
// flags, the windows) and k_plan_compact on the flags (the next list: the alive scenarios); without
// them none of the three is launched and the plan issues the launches it issued before.

#include "piadmm_obca_plan.h"

namespace obca_plan {

// ---------------------------------------------------------------------------------------------
// The PI anti-windup dual law (piadmm_obca_dual_plan): the per-edge PI of
// ADMM_CVX_two_veh_intesection_PI_antiwindup.m:156-188 with a constant proportional gain, on the
// consensus error of the plan.  Opt-in: without a law neither kernel is launched.
// ---------------------------------------------------------------------------------------------
// One wave per active scenario, between k_obca_edge and k_plan_residual: the edge output's
// lamb_bar_new and its 7 dres partials are overwritten in place with the law's, so k_plan_residual
// takes them into the state, the residual and the stop rule as it takes the fused update's.  Entry
// i = lane + 64 j of [vehicle 2][slot 7][9] (two passes); of a slot whose edge solve wrote an answer
//   e = w - Zb;  S' = S + kI e + d_gain D;  raw = S' + kP e;
//   lam' = windup ? min(sat, max(raw, -sat)) : raw;  D' = windup ? lam' - raw : 0
// with w = [local_x, lamb_ij] of the edge record and Zb the rounded Z of the edge output; every
// other slot keeps lamb_bar, S and D and adds 0 to the residual.  S and D are first copied to
// S_prev and D_prev: a scenario is only submitted while it has not stopped, so at its stopping
// iterate the copies are the integrator of the frozen previous state (B16).  The scenario index is
// wave-uniform, so the gains row and the 7 statuses are uniform loads.  Products and sums are kept
// apart (no contraction): piadmm.obca.lambda_update_pi is the same statements on the host.
__global__ void __launch_bounds__(64 * PW) k_plan_dual_pi(const int* __restrict__ active, int n_act,
                                                          const double* __restrict__ erecs,
                                                          double* __restrict__ eout, const int* __restrict__ eist,
                                                          const double* __restrict__ gains, int g_stride,
                                                          double* __restrict__ S, double* __restrict__ D,
                                                          double* __restrict__ Sp, double* __restrict__ Dp) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= n_act) return;
  const int s = __builtin_amdgcn_readfirstlane(active[k]);
  const double* G = gains + (size_t)s * g_stride;
  const double kP = G[G_KP], kI = G[G_KI], sat = G[G_SAT], d_gain = G[G_DGAIN];
  const bool windup = G[G_WINDUP] != 0.0;
  const double* E = erecs + (size_t)k * EREC;
  double* eo = eout + (size_t)k * EOUT;
  const int* st = eist + (size_t)k * NT * 3;
  // the slots whose solve wrote an answer, as bits (the `wrote` rule of the edge kernel)
  unsigned wrote = 0;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    const int c = st[t * 3];
    if (c == PIADMM_OBCA_CONVERGED || c == PIADMM_OBCA_MAX_ITER || c == PIADMM_OBCA_LINESEARCH_FAIL) wrote |= 1u << t;
  }
  double dr0 = 0.0, dr1 = 0.0;
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    double dr = 0.0;
    if (i < 126) {
      const int vt = i / 9, li = i % 9, t = vt % NT;
      const double w = li < 5 ? E[E_LX + vt * 5 + li] : E[E_LIJ + vt * 4 + (li - 5)];
      const double zb = eo[EO_ZB + i], lam = E[E_LB + i];
      const size_t q = (size_t)s * 126 + i;
      const double S0 = S[q], D0 = D[q];
      Sp[q] = S0;
      Dp[q] = D0;
      double lam1 = lam;
      if ((wrote >> t) & 1u) {
        const double e = w - zb;
        const double S1 = S0 + kI * e + d_gain * D0;
        const double raw = S1 + kP * e;
        lam1 = windup ? fmin(sat, fmax(raw, -sat)) : raw;
        const double D1 = windup ? lam1 - raw : 0.0;
        S[q] = S1;
        D[q] = D1;
      }
      eo[EO_LBN + i] = lam1;
      dr = fabs(lam1 - lam);
    }
    if (j == 0) dr0 = dr; else dr1 = dr;
  }
  // every lane is here again.  Slot t's sum |delta lamb_bar| over its 18 entries in the edge kernel's
  // lane order (vehicle 0's 9, then vehicle 1's 9): entry i sits in pass i / 64, lane i % 64
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    double dsum = 0.0;
#pragma unroll
    for (int c = 0; c < 18; ++c) {
      const int i = (c / 9) * 63 + t * 9 + c % 9;
      dsum += __shfl(i < 64 ? dr0 : dr1, i & 63, 64);
    }
    if (lane == 0) eo[EO_DRES + t] = dsum;
  }
}

// One wave (a workgroup of its own) on scenario s: the horizon shift of the frozen integrator
// (S_prev, D_prev: one slot on, the last slot repeated) into both copies, as the state shift does to
// lamb_bar.  The body of k_plan_dual_shift and of k_plan_dual_shift_list.
__device__ __forceinline__ void dual_shift_scenario(int s, int lane, double* __restrict__ S, double* __restrict__ D,
                                                    double* __restrict__ Sp, double* __restrict__ Dp) {
  const size_t base = (size_t)s * 126;
  double vs[2], vd[2];
  // every read first, then every write: the shift reads slot t + 1 of the arrays it overwrites
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    vs[j] = vd[j] = 0.0;
    if (i < 126) {
      const int v = i / (NT * 9), t = (i % (NT * 9)) / 9, e = i % 9;
      const int tt = t + 1 < NT ? t + 1 : NT - 1;
      vs[j] = Sp[base + (v * NT + tt) * 9 + e];
      vd[j] = Dp[base + (v * NT + tt) * 9 + e];
    }
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    if (i < 126) {
      S[base + i] = vs[j];  Sp[base + i] = vs[j];
      D[base + i] = vd[j];  Dp[base + i] = vd[j];
    }
  }
}

// One wave per scenario, after k_plan_shift.
__global__ void __launch_bounds__(64) k_plan_dual_shift(int n, double* __restrict__ S, double* __restrict__ D,
                                                        double* __restrict__ Sp, double* __restrict__ Dp) {
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  if (s >= n) return;
  dual_shift_scenario(s, lane, S, D, Sp, Dp);
}

// One wave per entry of `list`, after k_plan_shift_list: the integrators of the scenarios a clocked
// step ran; a retired scenario's stay frozen.
__global__ void __launch_bounds__(64) k_plan_dual_shift_list(const int* __restrict__ list, int m,
                                                             double* __restrict__ S, double* __restrict__ D,
                                                             double* __restrict__ Sp, double* __restrict__ Dp) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= m) return;
  const int s = __builtin_amdgcn_readfirstlane(list[blockIdx.x]);
  dual_shift_scenario(s, lane, S, D, Sp, Dp);
}

// ---------------------------------------------------------------------------------------------
// Longest-first scenario order (piadmm_obca_order_plan): k_plan_work keeps what every scenario's
// solves cost when it last ran, k_plan_order sorts a list by it.  Both launches of an iterate run
// one wave per problem in list order, so the list's order is the order both solves start in.
// Opt-in: without it neither kernel is launched and every list is ascending.
// ---------------------------------------------------------------------------------------------
constexpr int ORDER_BITS = 21;                       // per key field; scenario indices stay below 2^21
constexpr int ORDER_CLAMP = (1 << ORDER_BITS) - 1;

// One wave per active scenario, after k_obca_edge (and k_plan_dual_pi, which leaves ist alone):
// work[s] = (Q, I), the largest QP step count ist[.][2] and the largest SQP iteration count
// ist[.][1] over the scenario's 2 local and 7 edge solves of this iterate.  Lanes 0-1 read the local
// triples, lanes 2-8 the edge triples; the counts are non-negative, so the idle lanes' 0 is neutral.
// A scenario that is not in the list keeps its pair.
__global__ void __launch_bounds__(64 * PW) k_plan_work(const int* __restrict__ active, int n_act,
                                                       const int* __restrict__ list, const int* __restrict__ eist,
                                                       int* __restrict__ work) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= n_act) return;
  const int s = __builtin_amdgcn_readfirstlane(active[k]);
  int q = 0, it = 0;
  if (lane < 2 + NT) {
    const int* t3 = lane < 2 ? list + (size_t)(2 * k + lane) * 3 : eist + ((size_t)k * NT + (lane - 2)) * 3;
    it = t3[1];
    q = t3[2];
  }
#pragma unroll
  for (int o = 8; o > 0; o >>= 1) {
    q = max(q, __shfl_xor(q, o, 64));
    it = max(it, __shfl_xor(it, o, 64));
  }
  if (lane == 0) {
    work[2 * (size_t)s] = q;
    work[2 * (size_t)s + 1] = it;
  }
}

// (Q, I, s) as one key: a greater key sorts earlier.  Q and I are clamped into their 21 bits and
// the scenario enters as 2^21 - 1 - s, so the keys of distinct scenarios are distinct and equal
// work is broken by the smaller index.
__device__ __forceinline__ unsigned long long order_key(const int* __restrict__ work, int s) {
  const int q = min(max(work[2 * (size_t)s], 0), ORDER_CLAMP), it = min(max(work[2 * (size_t)s + 1], 0), ORDER_CLAMP);
  return ((unsigned long long)q << (2 * ORDER_BITS)) | ((unsigned long long)it << ORDER_BITS) |
         (unsigned long long)(ORDER_CLAMP - s);
}

// list_out = the first c entries of list_in sorted by Q descending, then I descending, then
// scenario ascending; c = count[0] clamped to [0, m] (read once), or m without a count.  One wave
// per entry: its position is the number of entries with a greater key, counted by the lanes
// striding over the list (ballot and popcount, so the position is wave-uniform).  Keys are distinct,
// so the positions are a permutation of 0..c-1: every slot is written once, by one wave, whatever
// the order of list_in or of the workgroups; no atomic, no wait.  list_out must not be list_in.
__global__ void __launch_bounds__(64 * PW) k_plan_order(const int* __restrict__ list_in,
                                                        const int* __restrict__ count, int m,
                                                        const int* __restrict__ work, int* __restrict__ list_out) {
  const int lane = threadIdx.x & 63;
  const int i = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int c = count ? min(max(__builtin_amdgcn_readfirstlane(count[0]), 0), m) : m;
  if (i >= c) return;
  const int s = __builtin_amdgcn_readfirstlane(list_in[i]);
  const unsigned long long mine = order_key(work, s);
  int rank = 0;
  for (int start = 0; start < c; start += 64) {
    const int j = start + lane;
    const bool greater = j < c && order_key(work, list_in[j]) > mine;
    rank += __popcll(__ballot(greater));
  }
  if (lane == 0) list_out[rank] = s;
}

// ---------------------------------------------------------------------------------------------
// Per-scenario clocks (piadmm_obca_clock_plan): clk[s] = (c, len, alive), c the row of scenario s's
// own reference that slot 0 of its horizon reads, len the valid rows of that reference.  Opt-in:
// without a clock neither k_plan_clock nor the list-taking shifts are launched.
// ---------------------------------------------------------------------------------------------

// One wave per scenario, after the shifts of a clocked step: the tick c += ran[s] (ran: the scenarios
// the step ran; nullptr ticks nobody and only rebuilds), alive = (c + 8 <= len), and of an alive
// scenario the window copy, exact.  c and len are wave-uniform (first-lane broadcast), so the flag
// is and a retired scenario's wave leaves whole.  The flag also asks 0 <= c and len <= n_ref, so the
// copy stays inside the reference whatever the record holds.  `alive` is the flag list
// k_plan_compact makes the next active list from, and the next tick's `ran`.
__global__ void __launch_bounds__(64 * PW) k_plan_clock(int n, int* __restrict__ clk, const int* __restrict__ ran,
                                                        const double* __restrict__ ref, int ref_stride, int n_ref,
                                                        double* __restrict__ win, int* __restrict__ alive) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= n) return;
  int* K = clk + 3 * (size_t)s;
  const int tick = ran ? (__builtin_amdgcn_readfirstlane(ran[s]) != 0 ? 1 : 0) : 0;
  const int c = __builtin_amdgcn_readfirstlane(K[0]) + tick;
  const int len = __builtin_amdgcn_readfirstlane(K[1]);
  const int ok = (c >= 0 && len <= n_ref && c <= len - 8) ? 1 : 0;
  if (lane == 0) {
    K[0] = c;
    K[2] = ok;
    alive[s] = ok;
  }
  if (!ok) return;
  const double* rf = ref + (size_t)s * ref_stride;
  double* W = win + (size_t)s * WIN;
  for (int i = lane; i < WIN; i += 64) {
    const int v = i / 40, j = i % 40;
    W[i] = rf[((size_t)v * n_ref + c) * 5 + j];
  }
}

}  // namespace obca_plan

using namespace obca_plan;

namespace obca_plan {
// One gains row of the dual law: nullptr when it is good, else what is wrong with it.
const char* dual_row_check(const double* row) {
  for (int i = 0; i < DPAR; ++i)
    if (!std::isfinite(row[i])) return "every entry finite";
  if (row[G_WINDUP] != 0.0 && row[G_WINDUP] != 1.0) return "windup 0 or 1";
  if (row[G_WINDUP] == 1.0 && !(row[G_SAT] > 0.0)) return "windup_sat > 0 with windup set";
  for (int i = G_WINDUP + 1; i < DPAR; ++i)
    if (row[i] != 0.0) return "the trailing entries must be 0";
  return nullptr;
}

// Enqueues what follows a change of the clocks: the tick of the scenarios flagged in `ran` (nullptr:
// nobody, the record is only rebuilt), the alive flags into flag[dst], the windows of the alive
// scenarios, their ascending list into ck.list and the list the next iterate reads (sorted, with
// the order on).  n_alive is the mirror's count of the flags the tick writes.  No synchronisation.
int clock_lists(piadmm_obca_t h, piadmm_obca_plan_s* p, const int* ran, int dst, int n_alive) {
  auto& c = p->ck;
  hipLaunchKernelGGL(k_plan_clock, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->n, c.clk, ran, p->ref,
                     p->ref_stride, p->cfg.n_ref, c.win, c.flag[dst]);
  OWN_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_plan_compact, dim3(1), dim3(CT), 0, h->stream, c.ident, c.flag[dst], p->n, c.list, p->count);
  OWN_HIP(h, hipGetLastError());
  if (n_alive <= 0) return 0;
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(n_alive)), dim3(64 * PW), 0, h->stream, c.list,
                       (const int*)nullptr, n_alive, p->ord.work, p->act[p->cur]);
    OWN_HIP(h, hipGetLastError());
  } else {
    OWN_HIP(h, hipMemcpyAsync(p->act[p->cur], c.list, (size_t)n_alive * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  }
  return 0;
}

// What an admission and an import end with, the mirror and admm_rows being up to date: the rows'
// largest max_admm_iter, then the windows, the flags and the list again, over all n (the order, when
// attached, re-sorts it), and the counts.  Synchronises.
int clock_relist(piadmm_obca_t h, piadmm_obca_plan_s* p) {
  p->max_iter_all = std::max(0, *std::max_element(p->admm_rows.begin(), p->admm_rows.end()));
  int n_alive = 0;
  for (int s = 0; s < p->n; ++s) n_alive += p->ck.host[3 * (size_t)s + 2];
  if (int rc = clock_lists(h, p, nullptr, p->ck.cur, n_alive)) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  p->ck.n_list = n_alive;
  p->n_act = n_alive;
  return 0;
}

// piadmm_obca_plan_shift of a clocked plan: the step closes for the scenarios it ran (ck.list), their
// clocks tick, and the next step's list is the scenarios still alive.
int clock_shift(piadmm_obca_t h, piadmm_obca_plan_s* p) {
  auto& c = p->ck;
  const int m = c.n_list;
  if (p->lp.on) {
    // the plant step first: it reads the closing step's init_state, its first control and the clocks
    // before the shift and the tick overwrite them
    if (int rc = loop_close(h, p)) return rc;
  }
  hipLaunchKernelGGL(k_plan_shift_list, dim3(m), dim3(64), 0, h->stream, c.list, m, p->bar, p->barp, p->X, p->lamb,
                     p->ctrlp);
  OWN_HIP(h, hipGetLastError());
  if (p->du.on) {
    hipLaunchKernelGGL(k_plan_dual_shift_list, dim3(m), dim3(64), 0, h->stream, c.list, m, p->du.S, p->du.D, p->du.Sp,
                       p->du.Dp);
    OWN_HIP(h, hipGetLastError());
  }
  if (p->lp.on) {
    // the state each scenario reached over init_state of both copies, before the tick rebuilds the list
    if (int rc = loop_set_init(h, p)) return rc;
  }
  if (p->lg.on) {
    // the open records take the step while ck.list and the clocks are still the closing step's
    if (int rc = ledger_step(h, p)) return rc;
  }
  // the mirror: the tick is deterministic, nothing is read back for it
  std::vector<int> next = c.host;
  int n_alive = 0;
  for (int s = 0; s < p->n; ++s) {
    int* k = next.data() + 3 * (size_t)s;
    if (k[2]) k[0] += 1;
    k[2] = k[0] <= k[1] - 8 ? 1 : 0;
    n_alive += k[2];
  }
  if (int rc = clock_lists(h, p, c.flag[c.cur], 1 - c.cur, n_alive)) return rc;
  if (p->lp.on) {
    // the latencies of the step that opens, of the scenarios still alive at their new clocks
    if (int rc = loop_open(h, p, n_alive)) return rc;
  }
  if (p->tr.on) {
    if (int rc = trace_append(h, p, p->tr.rows + 1)) return rc;
  }
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (p->lg.on) ledger_stepped(p, next);
  c.host.swap(next);
  c.cur = 1 - c.cur;
  c.n_list = n_alive;
  if (p->tr.on) p->tr.rows += 1;
  p->t_step += 1;
  p->i_iter = 0;
  p->n_act = n_alive;
  p->n_last = 0;
  return 0;
}
}  // namespace obca_plan

namespace {
int dual_rows_check(piadmm_obca_t h, const double* gains, int rows, int n, const std::string& who) {
  return rows_check(h, who, "", gains, rows, n, obca_plan::DPAR, dual_row_check);
}

// One clock row (c0, len) against the plan's n_ref: nullptr when it is good, else what is wrong.
const char* clock_row_check(int c0, int len, int n_ref) {
  if (c0 < 0) return "c0 >= 0";
  if (len < 8 || len > n_ref) return "8 <= len <= n_ref";
  if (c0 > len - 8) return "c0 + 8 <= len";
  return nullptr;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_dual_plan(piadmm_obca_t h, const double* gains, int32_t rows) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_dual_plan")) return rc;
  const bool detach = !gains || rows == 0;
  if (!detach)
    if (int rc = dual_rows_check(h, gains, rows, p->n, "obca_dual_plan")) return rc;
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_dual_plan: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  // the earlier law goes before the new one is built, not after it: the plan never holds two
  // integrators (peak device memory), and a failure below leaves the plan without a law
  p->du = {};
  if (detach) return 0;
  piadmm_obca_plan_s::dual_s d;
  const size_t N = (size_t)p->n, L = 126 * sizeof(double);
  int rc = 0;
  if ((rc = d.par.alloc(h, (size_t)rows * DPAR, false)) || (rc = d.S.alloc(h, N * 126, false)) ||
      (rc = d.Sp.alloc(h, N * 126, false)) || (rc = d.D.alloc(h, N * 126, true)) ||
      (rc = d.Dp.alloc(h, N * 126, true)))
    return rc;
  // S = lamb_bar of the current state (at a step boundary also the previous one's), D = 0: with
  // kP = 0, kI = rho and no saturation the law is then the plain update
  hipError_t e = hipMemcpy(d.par, gains, (size_t)rows * DPAR * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(d.S, L, p->bar + S_LB, STATE * sizeof(double), L, N, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d.Sp, d.S, N * L, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    return fail(h, PIADMM_E_HIP, std::string("obca_dual_plan: ") + hipGetErrorString(e));
  }
  d.rows = rows;
  d.stride = rows > 1 ? DPAR : 0;
  d.on = true;
  p->du = std::move(d);
  return 0;
}

int32_t piadmm_obca_dual_pi(piadmm_obca_t h, int32_t n, const double* w, const double* zb, const double* lamb,
                            const int32_t* status, const double* gains, int32_t rows, double* S, double* D,
                            double* lamb_out, double* dres_out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_dual_pi: 1 <= n <= 2^20");
  if (!w || !zb || !lamb || !status || !gains || !S || !D || !lamb_out || !dres_out)
    return fail(h, PIADMM_E_ARG, "obca_dual_pi: null argument");
  if (int rc = dual_rows_check(h, gains, rows, n, "obca_dual_pi")) return rc;
  const size_t N = (size_t)n;
  const double* in[] = {w, zb, lamb, S, D};
  const char* names[] = {"w", "zb", "lamb", "S", "D"};
  for (int a = 0; a < 5; ++a)
    for (size_t i = 0; i < N * 126; ++i)
      if (!std::isfinite(in[a][i]))
        return fail(h, PIADMM_E_ARG, std::string("obca_dual_pi: ") + names[a] + " of scenario " +
                    std::to_string(i / 126) + " is not finite");
  // the kernel reads an edge record, an edge output and the slots' statuses: the caller's arrays in
  // those layouts, scenario k of the identity list
  std::vector<double> rec(N * EREC, 0.0), out(N * EOUT, 0.0);
  std::vector<int> ist(N * NT * 3, 0), ident = identity_list(N);
  for (size_t k = 0; k < N; ++k) {
    for (int i = 0; i < 126; ++i) {
      const int vt = i / 9, li = i % 9;
      rec[k * EREC + (li < 5 ? E_LX + vt * 5 + li : E_LIJ + vt * 4 + (li - 5))] = w[k * 126 + i];
      rec[k * EREC + E_LB + i] = lamb[k * 126 + i];
      out[k * EOUT + EO_ZB + i] = zb[k * 126 + i];
    }
    for (int t = 0; t < NT; ++t) ist[(k * NT + t) * 3] = status[k * NT + t];
  }
  OWN_HIP(h, hipSetDevice(h->device));
  scratch a(h);
  double *d_rec = a.take<double>(N * EREC, false), *d_out = a.take<double>(N * EOUT, false),
         *d_g = a.take<double>((size_t)rows * DPAR, false), *d_S = a.take<double>(N * 126, false),
         *d_D = a.take<double>(N * 126, false), *d_Sp = a.take<double>(N * 126, true),
         *d_Dp = a.take<double>(N * 126, true);
  int *d_ist = a.take<int>(N * NT * 3, false), *d_act = a.take<int>(N, false);
  if (a.rc) return a.rc;
  const size_t B = sizeof(double);
  OWN_HIP(h, hipMemcpyAsync(d_rec, rec.data(), N * EREC * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_out, out.data(), N * EOUT * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_g, gains, (size_t)rows * DPAR * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_S, S, N * 126 * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_D, D, N * 126 * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_ist, ist.data(), N * NT * 3 * sizeof(int), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_act, ident.data(), N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_dual_pi, dim3(blocks_for(n)), dim3(64 * PW), 0, h->stream, d_act, n, d_rec, d_out, d_ist,
                     d_g, rows > 1 ? DPAR : 0, d_S, d_D, d_Sp, d_Dp);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(out.data(), d_out, N * EOUT * B, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(S, d_S, N * 126 * B, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(D, d_D, N * 126 * B, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  for (size_t k = 0; k < N; ++k) {
    for (int i = 0; i < 126; ++i) lamb_out[k * 126 + i] = out[k * EOUT + EO_LBN + i];
    for (int t = 0; t < NT; ++t) dres_out[k * NT + t] = out[k * EOUT + EO_DRES + t];
  }
  return 0;
}

int32_t piadmm_obca_order_plan(piadmm_obca_t h, int32_t mode, const int32_t* work_init) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_order_plan")) return rc;
  if (mode != 0 && mode != 1) return fail(h, PIADMM_E_ARG, "obca_order_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  if (mode == 1) {
    if (n > ORDER_CLAMP) return fail(h, PIADMM_E_ARG, "obca_order_plan: n_scenarios < 2^21");
    if (work_init)
      for (int k = 0; k < n; ++k)
        if (work_init[2 * (size_t)k] < 0 || work_init[2 * (size_t)k + 1] < 0)
          return fail(h, PIADMM_E_ARG, "obca_order_plan: row " + std::to_string(k) + ": work_init >= 0");
  }
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_order_plan: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  // at a step boundary every scenario is active: the current list is all n of them
  const size_t N = (size_t)n;
  const std::vector<int> ident = identity_list(N);
  // with a clock the current list is the alive scenarios, ascending in ck.list
  const int m_cur = p->ck.on ? p->ck.n_list : n;
  if (mode == 0) {
    if (p->ord.on && p->ck.on) {
      if (m_cur > 0)
        OWN_HIP(h, hipMemcpy(p->act[p->cur], p->ck.list, (size_t)m_cur * sizeof(int), hipMemcpyDeviceToDevice));
    } else if (p->ord.on) {
      OWN_HIP(h, hipMemcpy(p->act[p->cur], ident.data(), N * sizeof(int), hipMemcpyHostToDevice));
    }
    p->ord = {};
    return 0;
  }
  piadmm_obca_plan_s::order_s no;
  hipError_t e = no.work.make(2 * N);
  if (e == hipSuccess) e = no.tmp.make(N);
  if (e == hipSuccess)
    e = work_init ? hipMemcpy(no.work, work_init, 2 * N * sizeof(int), hipMemcpyHostToDevice)
                  : hipMemset(no.work, 0, 2 * N * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(no.tmp, ident.data(), N * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess && m_cur > 0) {
    // the current list re-sorted at once (zero work: ascending, as it was)
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(m_cur)), dim3(64 * PW), 0, h->stream,
                       p->ck.on ? (const int*)p->ck.list : (const int*)no.tmp, (const int*)nullptr, m_cur, no.work,
                       p->act[p->cur]);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    return fail(h, PIADMM_E_HIP, std::string("obca_order_plan: ") + hipGetErrorString(e));
  }
  no.on = true;
  p->ord = std::move(no);
  return 0;
}

int32_t piadmm_obca_order(piadmm_obca_t h, const int32_t* list, int32_t m, const int32_t* work, int32_t n,
                          int32_t* out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > ORDER_CLAMP) return fail(h, PIADMM_E_ARG, "obca_order: 1 <= n < 2^21");
  if (m < 1 || m > n) return fail(h, PIADMM_E_ARG, "obca_order: 1 <= m <= n");
  if (!list || !work || !out) return fail(h, PIADMM_E_ARG, "obca_order: null argument");
  if (int rc = slots_check(h, "obca_order", "list", list, m, n)) return rc;
  for (int k = 0; k < n; ++k)
    if (work[2 * (size_t)k] < 0 || work[2 * (size_t)k + 1] < 0)
      return fail(h, PIADMM_E_ARG, "obca_order: row " + std::to_string(k) + ": work >= 0");
  OWN_HIP(h, hipSetDevice(h->device));
  const size_t M = (size_t)m, N = (size_t)n;
  scratch a(h);
  int *d_in = a.take<int>(M, false), *d_work = a.take<int>(2 * N, false), *d_out = a.take<int>(M, true);
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_in, list, M * sizeof(int), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_work, work, 2 * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, d_in, (const int*)nullptr, m,
                     d_work, d_out);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(out, d_out, M * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_clock_plan(piadmm_obca_t h, int32_t mode, const int32_t* clock_init) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_clock_plan")) return rc;
  if (mode != 0 && mode != 1) return fail(h, PIADMM_E_ARG, "obca_clock_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n, n_ref = p->cfg.n_ref;
  const size_t N = (size_t)n;
  std::vector<int> rec(3 * N);
  if (mode == 1) {
    for (int k = 0; k < n; ++k) {
      const int c0 = clock_init ? clock_init[2 * (size_t)k] : p->t_step;
      const int len = clock_init ? clock_init[2 * (size_t)k + 1] : n_ref;
      if (const char* why = clock_row_check(c0, len, n_ref))
        return fail(h, PIADMM_E_ARG, "obca_clock_plan: row " + std::to_string(k) + ": " + why);
      rec[3 * (size_t)k] = c0;
      rec[3 * (size_t)k + 1] = len;
      rec[3 * (size_t)k + 2] = 1;
    }
  }
  if (mode == 1 && p->fb.on)
    return fail(h, PIADMM_E_STATE, "obca_clock_plan: feedback is attached (obca_feedback_plan: the tape has no per-scenario clocks)");
  if (mode == 1 && p->dl.on)
    return fail(h, PIADMM_E_STATE, "obca_clock_plan: the delay is attached (obca_delay_plan: it counts the plan's steps, not per-scenario clocks)");
  if (p->lg.on)
    return fail(h, PIADMM_E_STATE, "obca_clock_plan: a ledger is attached (obca_ledger_begin: its records open and close by the clocks; end it first)");
  if (p->lp.on)
    return fail(h, PIADMM_E_STATE, "obca_clock_plan: the loop is attached (obca_loop_plan: its step index is the tenant's clock; detach it first)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_clock_plan: only at a step boundary (an MPC step is open)");
  if (mode == 0) {
    if (!p->ck.on) return 0;
    const std::vector<int>& k = p->ck.host;
    for (int s = 0; s < n; ++s)
      if (!k[3 * (size_t)s + 2] || k[3 * (size_t)s] != k[0] || k[3 * (size_t)s + 1] != n_ref)
        return fail(h, PIADMM_E_STATE, "obca_clock_plan: detaching needs every scenario alive, on one c and with len = n_ref (scenario " +
                    std::to_string(s) + ")");
    OWN_HIP(h, hipSetDevice(h->device));
    OWN_HIP(h, hipStreamSynchronize(h->stream));
    // every scenario is alive: the current list already holds all n, in the plan's order
    p->t_step = k[0];
    p->ck = {};
    return 0;
  }
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  piadmm_obca_plan_s::clock_s nk;
  const std::vector<int> ident = identity_list(N);
  hipError_t e = nk.clk.make(3 * N);
  if (e == hipSuccess) e = nk.flag[0].make(N);
  if (e == hipSuccess) e = nk.flag[1].make(N);
  if (e == hipSuccess) e = nk.list.make(N);
  if (e == hipSuccess) e = nk.ident.make(N);
  if (e == hipSuccess) e = nk.win.make(N * WIN);
  if (e == hipSuccess) e = hipMemcpy(nk.clk, rec.data(), 3 * N * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(nk.ident, ident.data(), N * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(nk.flag[0], 0, N * sizeof(int));
  if (e == hipSuccess) e = hipMemset(nk.flag[1], 0, N * sizeof(int));
  if (e == hipSuccess) e = hipMemset(nk.list, 0, N * sizeof(int));
  if (e == hipSuccess) e = hipMemset(nk.win, 0, N * WIN * sizeof(double));
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);      // the fills are done before the stream's kernels write (dalloc)
  if (e != hipSuccess) return fail(h, PIADMM_E_HIP, std::string("obca_clock_plan: ") + hipGetErrorString(e));
  p->ck = std::move(nk);
  p->ck.host = rec;
  p->ck.cur = 0;
  p->ck.n_list = n;
  p->ck.on = true;
  // every row is alive: the windows, the flags and the list of all n (sorted, with the order on)
  if (int rc = clock_lists(h, p, nullptr, 0, n)) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  p->n_act = n;
  return 0;
}

int32_t piadmm_obca_clock_admit(piadmm_obca_t h, int32_t m, const int32_t* slots, const int32_t* clock,
                                const double* state, const double* ref, const double* par, const int32_t* prob,
                                const double* primal_thres, const double* dual_thres) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_clock_admit")) return rc;
  const int n = p->n, n_ref = p->cfg.n_ref;
  if (m < 1 || m > n) return fail(h, PIADMM_E_ARG, "obca_clock_admit: 1 <= m <= n_scenarios");
  if (!slots || !clock) return fail(h, PIADMM_E_ARG, "obca_clock_admit: null argument (slots, clock)");
  if (int rc = slots_check(h, "obca_clock_admit", "slots", slots, m, n)) return rc;
  for (int k = 0; k < m; ++k) {
    const std::string row = "obca_clock_admit: row " + std::to_string(k) + ": ";
    if (const char* why = clock_row_check(clock[2 * (size_t)k], clock[2 * (size_t)k + 1], n_ref))
      return fail(h, PIADMM_E_ARG, row + why);
    if (par)
      if (const char* why = row_check(par + (size_t)k * TAB)) return fail(h, PIADMM_E_ARG, row + why);
    if (prob && prob[k] != 0 && prob[k] != 1) return fail(h, PIADMM_E_ARG, row + "prob must be 0 or 1");
  }
  if (!p->ck.on) return fail(h, PIADMM_E_STATE, "obca_clock_admit: no clock attached (obca_clock_plan)");
  if (p->tr.on) return fail(h, PIADMM_E_STATE, "obca_clock_admit: a trace is attached (its minima would mix two tenants)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_clock_admit: only at a step boundary (an MPC step is open)");
  if (ref && p->ref_rows != n) return fail(h, PIADMM_E_STATE, "obca_clock_admit: ref needs a plan with a reference per scenario (obca_fleet_begin)");
  if (par && p->tab_rows != n) return fail(h, PIADMM_E_STATE, "obca_clock_admit: par needs a plan with a parameter row per scenario (obca_fleet_begin)");
  if (p->lp.on)
    for (int k = 0; k < m; ++k)
      if ((int64_t)p->lp.k0 + clock[2 * (size_t)k] >= ((int64_t)1 << 31))
        return fail(h, PIADMM_E_STATE, "obca_clock_admit: row " + std::to_string(k) + ": loop step index exhausted");
  if (const char* why = ledger_replace_refusal(p, m, slots, false))
    return fail(h, PIADMM_E_STATE, std::string("obca_clock_admit: ") + why);
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (p->lg.on) {
    // the tenants that leave: their records, before anything of their slots is overwritten
    if (int rc = ledger_close(h, p, m, slots, 2, false)) return rc;
  }
  const size_t D = sizeof(double), ref_one = (size_t)2 * n_ref * 5;
  for (int k = 0; k < m; ++k) {
    const size_t s = (size_t)slots[k], K = (size_t)k;
    if (state) {
      OWN_HIP(h, hipMemcpy(p->bar + s * STATE, state + K * STATE, STATE * D, hipMemcpyHostToDevice));
      OWN_HIP(h, hipMemcpy(p->barp + s * STATE, state + K * STATE, STATE * D, hipMemcpyHostToDevice));
    }
    if (ref) OWN_HIP(h, hipMemcpy(p->ref + s * ref_one, ref + K * ref_one, ref_one * D, hipMemcpyHostToDevice));
    if (par) {
      OWN_HIP(h, hipMemcpy(p->tab + s * TAB, par + K * TAB, TAB * D, hipMemcpyHostToDevice));
      p->admm_rows[s] = (int)par[K * TAB + T_ADMM];
    }
    if (prob) OWN_HIP(h, hipMemcpy(p->prob + s, prob + K, sizeof(int), hipMemcpyHostToDevice));
    if (primal_thres) OWN_HIP(h, hipMemcpy(p->pth + s, primal_thres + K, D, hipMemcpyHostToDevice));
    if (dual_thres) OWN_HIP(h, hipMemcpy(p->dth + s, dual_thres + K, D, hipMemcpyHostToDevice));
    // the slot starts as a scenario of a fresh plan does
    OWN_HIP(h, hipMemset(p->ctrl + s * NCTRL, 0, NCTRL * D));
    OWN_HIP(h, hipMemset(p->ctrlp + s * NCTRL, 0, NCTRL * D));
    OWN_HIP(h, hipMemset(p->X + s * NX, 0, NX * D));
    OWN_HIP(h, hipMemset(p->lamb + s * 126, 0, 126 * D));
    OWN_HIP(h, hipMemset(p->iters + s, 0, sizeof(int)));
    OWN_HIP(h, hipMemset(p->mask + 2 * s, 0, 2 * sizeof(int)));
    if (p->du.on) {
      OWN_HIP(h, hipMemcpy(p->du.S + s * 126, p->bar + s * STATE + S_LB, 126 * D, hipMemcpyDeviceToDevice));
      OWN_HIP(h, hipMemcpy(p->du.Sp + s * 126, p->bar + s * STATE + S_LB, 126 * D, hipMemcpyDeviceToDevice));
      OWN_HIP(h, hipMemset(p->du.D + s * 126, 0, 126 * D));
      OWN_HIP(h, hipMemset(p->du.Dp + s * 126, 0, 126 * D));
    }
    if (p->ord.on) OWN_HIP(h, hipMemset(p->ord.work + 2 * s, 0, 2 * sizeof(int)));
    int* k3 = p->ck.host.data() + 3 * s;
    k3[0] = clock[2 * K];
    k3[1] = clock[2 * K + 1];
    k3[2] = 1;
    OWN_HIP(h, hipMemcpy(p->ck.clk + 3 * s, k3, 3 * sizeof(int), hipMemcpyHostToDevice));
  }
  if (int rc = clock_relist(h, p)) return rc;
  if (p->lp.on) {
    // the admitted slots keep their loop rows and stream ids; their latencies at the new clocks
    if (int rc = loop_open(h, p, p->ck.n_list)) {
      (void)hipStreamSynchronize(h->stream);
      return rc;
    }
    OWN_HIP(h, hipStreamSynchronize(h->stream));
  }
  if (p->lg.on) {
    // a fresh record for every admitted tenant, at its clock and entry state
    if (int rc = ledger_open(h, p, m, slots)) return rc;
  }
  return 0;
}

int32_t piadmm_obca_clock_tick(piadmm_obca_t h, int32_t n, const int32_t* clock_in, const int32_t* ran,
                               const double* ref, int32_t ref_rows, int32_t n_ref, int32_t* clock_out,
                               double* window_out, int32_t* list_out, int32_t* count_out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_clock_tick: 1 <= n <= 2^20");
  if (!clock_in || !ran || !ref || !clock_out || !window_out || !list_out || !count_out)
    return fail(h, PIADMM_E_ARG, "obca_clock_tick: null argument");
  if (ref_rows != 1 && ref_rows != n) return fail(h, PIADMM_E_ARG, "obca_clock_tick: ref_rows must be 1 or n");
  if (n_ref < 8 || n_ref > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_clock_tick: 8 <= n_ref <= 2^20");
  for (int k = 0; k < n; ++k) {
    const int c = clock_in[3 * (size_t)k], len = clock_in[3 * (size_t)k + 1];
    const char* why = c < 0 || c > (1 << 30) ? "0 <= c <= 2^30" : len < 8 || len > n_ref ? "8 <= len <= n_ref"
                      : ran[k] != 0 && ran[k] != 1 ? "ran 0 or 1" : nullptr;
    if (why) return fail(h, PIADMM_E_ARG, "obca_clock_tick: row " + std::to_string(k) + ": " + why);
  }
  OWN_HIP(h, hipSetDevice(h->device));
  const size_t N = (size_t)n, ref_one = (size_t)2 * n_ref * 5, R = ref_one * (size_t)ref_rows;
  const std::vector<int> ident = identity_list(N);
  scratch a(h);
  int *d_clk = a.take<int>(3 * N, false), *d_ran = a.take<int>(N, false), *d_alive = a.take<int>(N, true),
      *d_ident = a.take<int>(N, false), *d_list = a.take<int>(N, true), *d_count = a.take<int>(1, true);
  double *d_ref = a.take<double>(R, false), *d_win = a.take<double>(N * WIN, true);
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_clk, clock_in, 3 * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_ran, ran, N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_ident, ident.data(), N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_ref, ref, R * sizeof(double), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_clock, dim3(blocks_for(n)), dim3(64 * PW), 0, h->stream, n, d_clk, d_ran, d_ref,
                     ref_rows > 1 ? (int)ref_one : 0, n_ref, d_win, d_alive);
  OWN_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_plan_compact, dim3(1), dim3(CT), 0, h->stream, d_ident, d_alive, n, d_list, d_count);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(clock_out, d_clk, 3 * N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(window_out, d_win, N * WIN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(list_out, d_list, N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(count_out, d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
