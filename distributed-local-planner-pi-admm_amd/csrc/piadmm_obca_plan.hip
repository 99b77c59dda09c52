// piadmm_obca_plan.hip -- the OBCA-ADMM consensus loop, device-resident (gfx950).
//
// The loop of decentralized_overtaking_ADMM.py:31-102 (piadmm.obca.OBCAPlanner.step is the same
// statement on the host) for many scenarios at once, with the planner state kept on the device.
// One ADMM iterate is a fixed sequence of short, bounded launches on the handle's stream:
//   k_plan_pack_local   the local records of the active scenarios (pure copies of the state)
//   k_obca_sqp          the local solves (csrc/piadmm_obca.hip, identity order)
//   k_plan_exchange     bar_state_update + check_converge + the edge record
//   k_obca_edge         the edge solves with the fused lambda_update (csrc/piadmm_obca_edge.hip)
//   k_plan_residual     Z_bar / lamb_bar into the state, the residuals, the stop rule, B16's freeze
//   k_plan_compact      the next active list, in ascending scenario order (one workgroup, a scan)
// and the host reads back one int, the number of scenarios still active.  k_plan_shift closes an
// MPC step; with a trace attached (piadmm_obca_trace_begin) k_plan_trace and k_plan_clearance then
// append the step's row to the device-side run record.  With a dual law attached
// (piadmm_obca_dual_plan) k_plan_dual_pi runs between k_obca_edge and k_plan_residual and
// k_plan_dual_shift after k_plan_shift; without one neither is launched.  No kernel here waits for another workgroup, keeps a queue or orders anything with
// atomics: the record order of a launch is the ascending scenario order, the same on every run.
// With the longest-first order attached (piadmm_obca_order_plan) k_plan_work runs after k_obca_edge
// and k_plan_order after k_plan_compact and after k_plan_shift: the record order of a launch is then
// the scenarios by the work of their last solves, a pure function of that record, the same on
// every run; without it neither is launched.
// With per-scenario clocks attached (piadmm_obca_clock_plan) k_plan_pack_local reads each scenario's
// own 8 reference rows from a window, piadmm_obca_plan_shift runs k_plan_shift_list /
// k_plan_dual_shift_list on the scenarios the step ran and then k_plan_clock (their tick, the alive
// flags, the windows) and k_plan_compact on the flags (the next list: the alive scenarios); without
// them none of the three is launched and the plan issues the launches it issued before.
// With the feedback attached (piadmm_obca_feedback_plan) piadmm_obca_plan_shift runs k_plan_propagate
// before k_plan_shift (the plant step from the closing step's init_state and first control) and
// k_plan_set_init after it (the state the vehicle reached over init_state of both copies); without
// it neither is launched.  These two run one lane per vehicle, not one wave per item.
// With the noise attached on top (piadmm_obca_noise_plan) k_plan_noise runs in front of
// k_plan_propagate and writes the step's disturbance rows, which that kernel reads in the tape's
// place; without it k_plan_noise is not launched.  One lane per vehicle as well.
// With the communication delay attached (piadmm_obca_delay_plan) k_plan_exchange_stale runs in
// k_plan_exchange's place (what a vehicle sends is computed from its plan interpolated tau back) and
// piadmm_obca_plan_shift launches k_plan_delay last, one lane per vehicle: the latencies of the step
// that opens; without it neither is launched.
// With the loop attached (piadmm_obca_loop_plan; a clocked plan only) piadmm_obca_plan_shift runs
// k_loop_close before k_plan_shift_list (noise at k0 + c plus the plant step of the scenarios the
// step ran) and k_plan_set_init after it (the state each reached over init_state of both copies),
// and with delay rows k_loop_open after the tick (the latencies of the alive scenarios at their new
// clocks) and every iterate k_plan_exchange_stale in k_plan_exchange's place; without it none is
// launched.
// With a ledger attached (piadmm_obca_ledger_begin; a clocked plan only) piadmm_obca_plan_shift runs
// k_ledger_step on the scenarios the step ran, after the shift (under the loop: after k_plan_set_init)
// and before the tick: their open records take the step, and the ones the tick retires are appended;
// an admission or an import runs k_ledger_close and k_ledger_open; without it none is launched.
// The statistics of a run record (piadmm_obca_fleet_stats / _stats_trace: k_stats_fleet, k_stats_rows,
// k_stats_worst and their merges) and k_trace_gather are launched by those calls alone and write
// nothing of the plan or the trace.
//
// Layout: one wavefront per item (a local record, a scenario), PW waves per workgroup; waves
// never cooperate, and a wave past the end of its list exits whole at the top.
//
// Parameters and references are per scenario: the glue kernels read scenario s's parameter row
// at tab + s * tab_stride (PIADMM_OBCA_FLEET_PAR doubles, include/piadmm.h) and its reference at
// ref + s * ref_stride.  A plan opened by piadmm_obca_plan_begin is one row and one reference with
// both strides 0; piadmm_obca_fleet_begin uploads n of each.  The scenario index is made provably
// wave-uniform (first-lane broadcast), so what the whole wave needs of the row (conv_thres,
// min_dis, max_admm_iter) is a uniform load; the record parameters are loaded by the few lanes
// that store them.
//
// The attachments' kernels and calls are in csrc/piadmm_obca_plan_{attach,trace,tenant,feedback,delay,loop,ledger}.hip;
// the launches above that are theirs go through the declarations in csrc/piadmm_obca_plan.h.

#include "piadmm_obca_plan.h"

namespace obca_plan {

// the row entry behind parameter j of a local / an edge record, one hex digit each (prob, local 6
// and edge 2, comes from prob[])
constexpr unsigned LOCAL_PAR_ROW = 0xB0654310u;            // rho, min_dis, max_x, max_y, r, q, -, max_sqp_iter
constexpr unsigned long long EDGE_PAR_ROW = 0x987DCB010ull;  // rho, min_dis, -, max_sqp_iter, round_decimals, start,
                                                             // x_bound, mu_max, g_max

// Record 2k + v = vehicle v of scenario active[k]: what local_record (piadmm/obca.py) packs.
__global__ void __launch_bounds__(64 * PW) k_plan_pack_local(const int* __restrict__ active, int n_act,
                                                             const double* __restrict__ bar,
                                                             const int* __restrict__ prob,
                                                             const double* __restrict__ ref, int ref_stride,
                                                             int n_ref, int t_step,
                                                             const double* __restrict__ tab, int tab_stride,
                                                             double* __restrict__ recs) {
  const int lane = threadIdx.x & 63;
  const int r = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (r >= 2 * n_act) return;
  const int k = r >> 1, v = r & 1, o = 1 - v;
  const int s = __builtin_amdgcn_readfirstlane(active[k]);
  const double* B = bar + (size_t)s * STATE;
  const double* T = tab + (size_t)s * tab_stride;
  const double* rf = ref + (size_t)s * ref_stride + ((size_t)v * n_ref + t_step) * 5;
  double* rec = recs + (size_t)r * REC;
  for (int i = lane; i < REC; i += 64) {
    double val = 0.0;
    if (i < R_REF) val = B[S_INIT + v * 5 + (i - R_INIT)];
    else if (i < R_AO) val = rf[i - R_REF];
    else if (i < R_BO) val = B[S_A + o * 56 + (i - R_AO)];
    else if (i < R_LIJ) val = B[S_B + o * 28 + (i - R_BO)];
    else if (i < R_LB) val = B[S_LIJ + o * 28 + (i - R_LIJ)];
    else if (i < R_ZB) val = B[S_LB + v * 63 + (i - R_LB)];
    else if (i < R_PAR) val = B[S_ZB + v * 63 + (i - R_ZB)];
    else if (i < R_PAR + 8) {
      const int j = i - R_PAR;
      val = j == 6 ? (double)prob[s] : T[(LOCAL_PAR_ROW >> (4 * j)) & 15u];
    }
    rec[i] = val;
  }
}

// One wave per active scenario; lane < 14 owns the (vehicle, slot) item lane = v * 7 + t.  The body
// of k_plan_exchange (STALE = false: tau is not read, the statements are the plain exchange's) and of
// k_plan_exchange_stale (STALE = true: the item's state is stale_state of X[t] and X[t + 1] under the
// vehicle's latency tau[s][v]; the two latencies are loads at a wave-uniform address, X[t] 40 more
// bytes per lane next to the ones it reads anyway).
template <bool STALE>
__device__ __forceinline__ void plan_exchange(const int* __restrict__ active, int n_act,
                                              double* __restrict__ bar, const int* __restrict__ prob,
                                              const double* __restrict__ lout,
                                              const double* __restrict__ tab, int tab_stride,
                                              double sigd, int update_lamb_ij,
                                              double* __restrict__ ctrl, double* __restrict__ X,
                                              int* __restrict__ conv, double* __restrict__ erecs,
                                              const double* __restrict__ tau) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= n_act) return;
  const int s = __builtin_amdgcn_readfirstlane(active[k]);
  const int pr = prob[s];
  const double* T = tab + (size_t)s * tab_stride;
  const double conv_thres = T[T_CONV], min_dis = T[T_MIN_DIS];
  double* B = bar + (size_t)s * STATE;
  double* E = erecs + (size_t)k * EREC;
  const double* o2 = lout + (size_t)(2 * k) * OUT;           // the pair's two local outputs
  double pe0 = 0.0, pe1 = 0.0, pb = 0.0;
  if (lane < 2 * NT) {
    const int v = lane / NT, t = lane % NT, vt = lane;
    const double* ov = o2 + (size_t)v * OUT;
    const double* st = ov + O_X + (t + 1) * 5;
    double stale[5];
    if constexpr (STALE) {
      const double tau0 = tau[(size_t)2 * s], tau1 = tau[(size_t)2 * s + 1];
      stale_state(st - 5, st, v ? tau1 : tau0, stale);
      st = stale;
    }
    double A[4][2], b[4], l[4];
    halfspaces(st, pr, sigd, A, b);
#pragma unroll
    for (int i = 0; i < 4; ++i) l[i] = update_lamb_ij ? ov[O_LAM + t * 4 + i] : B[S_LIJ + vt * 4 + i];
#pragma unroll
    for (int j = 0; j < 5; ++j) { B[S_LX + vt * 5 + j] = st[j]; E[E_LX + vt * 5 + j] = st[j]; }
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      B[S_A + vt * 8 + 2 * i] = A[i][0];
      B[S_A + vt * 8 + 2 * i + 1] = A[i][1];
      B[S_B + vt * 4 + i] = b[i];
      if (update_lamb_ij) B[S_LIJ + vt * 4 + i] = l[i];
      E[E_LIJ + vt * 4 + i] = l[i];
      pe0 += A[i][0] * l[i];
      pe1 += A[i][1] * l[i];
      pb += b[i] * l[i];
    }
  }
  // the rest of the edge record: this iterate's lamb_bar, the parameters, the pad
  for (int i = lane; i < 126; i += 64) E[E_LB + i] = B[S_LB + i];
  if (lane < EREC - E_PAR) {
    const int j = lane;
    E[E_PAR + j] = j == 2 ? (double)pr : j < 9 ? T[(int)(EDGE_PAR_ROW >> (4 * j)) & 15] : 0.0;
  }
  // bar_ctrl = [U[:,0], U[:,1]] per vehicle, and X
  if (lane < NCTRL) {
    const int v = lane / 14, j = lane % 14;
    ctrl[(size_t)s * NCTRL + lane] = o2[(size_t)v * OUT + O_U + (j < NT ? 2 * j : 2 * (j - NT) + 1)];
  }
  for (int i = lane; i < NX; i += 64) X[(size_t)s * NX + i] = o2[(size_t)(i / 40) * OUT + O_X + i % 40];
  // check_converge: slot t = lanes t (vehicle 0) and t + 7 (vehicle 1)
  const double e0 = pe0 + __shfl(pe0, (lane + NT) & 63, 64);
  const double e1 = pe1 + __shfl(pe1, (lane + NT) & 63, 64);
  const double ueq = -pb - __shfl(pb, (lane + NT) & 63, 64);
  const bool ok = lane >= NT || (fabs(e0) <= conv_thres && fabs(e1) <= conv_thres && ueq >= min_dis);
  const int all_ok = __all(ok);
  if (lane == 0) conv[s] = all_ok ? 1 : 0;
}

__global__ void __launch_bounds__(64 * PW) k_plan_exchange(const int* __restrict__ active, int n_act,
                                                           double* __restrict__ bar, const int* __restrict__ prob,
                                                           const double* __restrict__ lout,
                                                           const double* __restrict__ tab, int tab_stride,
                                                           double sigd, int update_lamb_ij,
                                                           double* __restrict__ ctrl, double* __restrict__ X,
                                                           int* __restrict__ conv, double* __restrict__ erecs) {
  plan_exchange<false>(active, n_act, bar, prob, lout, tab, tab_stride, sigd, update_lamb_ij, ctrl, X, conv, erecs,
                       nullptr);
}

// The same exchange with the communication delay attached (piadmm_obca_delay_plan): what the
// vehicle sends -- local_x, A, b, and with them the edge record and check_converge -- is computed
// from the stale state; ctrl and X stay the local solution's.  Launched only while attached.
__global__ void __launch_bounds__(64 * PW) k_plan_exchange_stale(const int* __restrict__ active, int n_act,
                                                                 double* __restrict__ bar, const int* __restrict__ prob,
                                                                 const double* __restrict__ lout,
                                                                 const double* __restrict__ tab, int tab_stride,
                                                                 double sigd, int update_lamb_ij,
                                                                 double* __restrict__ ctrl, double* __restrict__ X,
                                                                 int* __restrict__ conv, double* __restrict__ erecs,
                                                                 const double* __restrict__ tau) {
  plan_exchange<true>(active, n_act, bar, prob, lout, tab, tab_stride, sigd, update_lamb_ij, ctrl, X, conv, erecs, tau);
}

// One wave per active scenario: the edge answer into the state, the residuals and the stop rule.
__global__ void __launch_bounds__(64 * PW) k_plan_residual(const int* __restrict__ active, int n_act, int i_iter,
                                                           double* __restrict__ bar, double* __restrict__ barp,
                                                           const double* __restrict__ ctrl, double* __restrict__ ctrlp,
                                                           const double* __restrict__ eout, const int* __restrict__ list,
                                                           const int* __restrict__ eist,
                                                           const double* __restrict__ pth, const double* __restrict__ dth,
                                                           const double* __restrict__ tab, int tab_stride,
                                                           double* __restrict__ primal_o, double* __restrict__ dual_o,
                                                           int* __restrict__ stop_o, int* __restrict__ iters,
                                                           int* __restrict__ mask, int* __restrict__ keep) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= n_act) return;
  const int s = __builtin_amdgcn_readfirstlane(active[k]);
  const int max_admm_iter = (int)tab[(size_t)s * tab_stride + T_ADMM];
  double* B = bar + (size_t)s * STATE;
  double* Bp = barp + (size_t)s * STATE;
  const double* eo = eout + (size_t)k * EOUT;
  // the 7 slot partials in index order, the 28 controls in index order (bit-repeatable)
  double dual = 0.0;
  for (int t = 0; t < NT; ++t) dual = dual + eo[EO_DRES + t];
  const double d = lane < NCTRL ? fabs(ctrl[(size_t)s * NCTRL + lane] - ctrlp[(size_t)s * NCTRL + lane]) : 0.0;
  double primal = 0.0;
  for (int j = 0; j < NCTRL; ++j) primal = primal + __shfl(d, j, 64);
  const bool stop = (primal <= pth[s] && dual <= dth[s]) || i_iter > max_admm_iter;
  // every status of the iterate, as bits
  int lm = lane < 2 ? 1 << (list[(size_t)(2 * k + lane) * 3] & 31) : 0;
  int em = lane < NT ? 1 << (eist[((size_t)k * NT + lane) * 3] & 31) : 0;
#pragma unroll
  for (int o = 4; o > 0; o >>= 1) { lm |= __shfl_xor(lm, o, 64); em |= __shfl_xor(em, o, 64); }
  // Z_bar and lamb_bar_new into the state; a continuing scenario's state becomes the previous
  // iterate's, a stopped one's previous state stays frozen for the shift (:87, B16)
  for (int i = lane; i < STATE; i += 64) {
    const bool zb = i < S_ZB + 126, lb = i >= S_LB && i < S_LB + 126;
    const double val = zb ? eo[EO_ZB + (i - S_ZB)] : lb ? eo[EO_LBN + (i - S_LB)] : B[i];
    if (zb || lb) B[i] = val;
    if (!stop) Bp[i] = val;
  }
  if (!stop && lane < NCTRL) ctrlp[(size_t)s * NCTRL + lane] = ctrl[(size_t)s * NCTRL + lane];
  if (lane == 0) {
    primal_o[s] = primal;
    dual_o[s] = dual;
    stop_o[s] = stop ? 1 : 0;
    if (stop) iters[s] = i_iter;
    mask[2 * s] |= lm;
    mask[2 * s + 1] |= em;
    keep[k] = stop ? 0 : 1;
  }
}

// The next active list: the kept entries of `active` in their order (ascending scenarios).  One
// workgroup scans the list tile by tile; nothing depends on the order workgroups run in.
__global__ void __launch_bounds__(CT) k_plan_compact(const int* __restrict__ active, const int* __restrict__ keep,
                                                     int n_act, int* __restrict__ next, int* __restrict__ count) {
  __shared__ int wtot[CT / 64];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  int base = 0;
  for (int start = 0; start < n_act; start += CT) {
    const int i = start + tid;
    const int f = i < n_act ? keep[i] : 0;
    const unsigned long long bal = __ballot(f);
    const int before = __popcll(bal & ((1ull << lane) - 1ull));
    if (lane == 0) wtot[wave] = __popcll(bal);
    __syncthreads();
    int off = base, tot = 0;
    for (int w = 0; w < CT / 64; ++w) {
      if (w < wave) off += wtot[w];
      tot += wtot[w];
    }
    if (f) next[off + before] = active[i];
    base += tot;
    __syncthreads();
  }
  if (tid == 0) count[0] = base;
}

// One wave (a workgroup of its own) on scenario s: iterate_next_state of the frozen previous state
// into both states, init_state = X[:, 1], the step's last lamb_bar kept for the record, the step's
// bookkeeping reset.  The body of k_plan_shift and of k_plan_shift_list.
__device__ __forceinline__ void shift_scenario(int s, int lane, double* __restrict__ bar, double* __restrict__ barp,
                                               const double* __restrict__ X, double* __restrict__ lamb,
                                               double* __restrict__ ctrlp) {
  double* B = bar + (size_t)s * STATE;
  double* Bp = barp + (size_t)s * STATE;
  constexpr int NV = (STATE + 63) / 64;
  double val[NV], lam[2];
  // every read first, then every write: the shift reads slot t + 1 of the array it overwrites
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = lane + 64 * j;
    val[j] = 0.0;
    if (i < S_INIT) {
      const int base = i < S_A ? S_ZB : i < S_B ? S_A : i < S_LB ? S_B : i < S_LIJ ? S_LB : i < S_LX ? S_LIJ : S_LX;
      const int w = i < S_A ? 9 : i < S_B ? 8 : i < S_LB ? 4 : i < S_LIJ ? 9 : i < S_LX ? 4 : 5;
      const int f = i - base, v = f / (NT * w), t = (f % (NT * w)) / w, e = f % w;
      const int tt = t + 1 < NT ? t + 1 : NT - 1;
      val[j] = Bp[base + (v * NT + tt) * w + e];
    } else if (i < STATE) {
      const int f = i - S_INIT;
      val[j] = X[(size_t)s * NX + (f / 5) * 40 + 5 + f % 5];
    }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    lam[j] = i < 126 ? B[S_LB + i] : 0.0;
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < NV; ++j) {
    const int i = lane + 64 * j;
    if (i < STATE) { B[i] = val[j]; Bp[i] = val[j]; }
  }
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int i = lane + 64 * j;
    if (i < 126) lamb[(size_t)s * 126 + i] = lam[j];
  }
  if (lane < NCTRL) ctrlp[(size_t)s * NCTRL + lane] = 0.0;
}

// One wave per scenario: every scenario is shifted and is active again.
__global__ void __launch_bounds__(64) k_plan_shift(int n, double* __restrict__ bar, double* __restrict__ barp,
                                                   const double* __restrict__ X, double* __restrict__ lamb,
                                                   double* __restrict__ ctrlp, int* __restrict__ active) {
  const int lane = threadIdx.x;
  const int s = blockIdx.x;
  if (s >= n) return;
  shift_scenario(s, lane, bar, barp, X, lamb, ctrlp);
  if (lane == 0) active[s] = s;
}

// One wave per entry of `list` (the scenarios a clocked step ran, piadmm_obca_clock_plan): the same
// shift for those alone; every other scenario stays as it is.  The next list is k_plan_clock's.
__global__ void __launch_bounds__(64) k_plan_shift_list(const int* __restrict__ list, int m,
                                                        double* __restrict__ bar, double* __restrict__ barp,
                                                        const double* __restrict__ X, double* __restrict__ lamb,
                                                        double* __restrict__ ctrlp) {
  const int lane = threadIdx.x;
  if ((int)blockIdx.x >= m) return;
  const int s = __builtin_amdgcn_readfirstlane(list[blockIdx.x]);
  shift_scenario(s, lane, bar, barp, X, lamb, ctrlp);
}

}  // namespace obca_plan

// ---------------------------------------------------------------------------------------------
// C-ABI (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
using namespace obca_plan;

namespace obca_plan {
// One parameter row: the ranges check_recs (csrc/piadmm_obca.hip) and edge_check
// (csrc/piadmm_obca_edge.hip) enforce per record, on the row those records are packed from, and the
// integers integral.  nullptr when the row is good, else what is wrong with it.
const char* row_check(const double* row) {
  auto integral = [](double v, double lo, double hi) { return v >= lo && v <= hi && v == std::floor(v); };
  if (!(row[T_RHO] > 0.0) || !(row[T_R] > 0.0) || !(row[T_Q] > 0.0) || !(row[T_MAX_X] > 0.0) ||
      !(row[T_MAX_Y] > 0.0) || !(row[T_XB] > 0.0) || !(row[T_MU] > 0.0))
    return "bad parameters (rho, r, q, max_x, max_y, x_bound, mu_max > 0)";
  if (!integral(row[T_SQP], 1.0, 1000.0)) return "1 <= max_sqp_iter <= 1000, an integer";
  if (!integral(row[T_START], 0.0, 1.0)) return "start 0 or 1";
  if (!integral(row[T_ROUND], -1.0, 15.0)) return "-1 <= round_decimals <= 15, an integer";
  if (!integral(row[T_ADMM], 0.0, 1073741824.0)) return "max_admm_iter >= 0 (at most 2^30), an integer";
  return nullptr;
}

// the staging buffer holds `bytes` of records and m slot numbers behind them
int stage_ensure(piadmm_obca_t h, piadmm_obca_plan_s* p, size_t bytes, int m) {
  const size_t need = bytes + (size_t)m * sizeof(int);
  if (p->stg.cap >= need) return 0;
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  p->stg = {};
  if (int rc = p->stg.buf.alloc(h, need, false)) return rc;
  p->stg.cap = need;
  return 0;
}
}  // namespace obca_plan

namespace {
// the parameter row of a configuration (the row a plan without a table runs every scenario on)
void row_of_cfg(const piadmm_obca_plan_cfg_t& c, double* row) {
  for (int i = 0; i < TAB; ++i) row[i] = 0.0;
  row[T_RHO] = c.rho;  row[T_MIN_DIS] = c.min_dis;  row[T_CONV] = c.conv_thres;
  row[T_MAX_X] = c.max_x;  row[T_MAX_Y] = c.max_y;  row[T_R] = c.r;  row[T_Q] = c.q;
  row[T_XB] = c.x_bound;  row[T_MU] = c.mu_max;  row[T_G] = c.g_max;
  row[T_ADMM] = (double)c.max_admm_iter;  row[T_SQP] = (double)c.max_sqp_iter;
  row[T_ROUND] = (double)c.round_decimals;  row[T_START] = (double)c.start;
}

// what every scenario of a plan shares, and prob
int shared_check(piadmm_obca_t h, const piadmm_obca_plan_cfg_t& c, const int32_t* prob, const std::string& who) {
  if (c.update_lamb_ij != 0 && c.update_lamb_ij != 1) return fail(h, PIADMM_E_ARG, who + ": update_lamb_ij 0 or 1");
  if (c.n_scenarios < 1) return fail(h, PIADMM_E_ARG, who + ": n_scenarios >= 1");
  if (c.n_scenarios > (1 << 20)) return fail(h, PIADMM_E_ARG, who + ": n_scenarios <= 2^20");
  if (c.t_step0 < 0 || c.n_ref < 8 || c.t_step0 > c.n_ref - 8)
    return fail(h, PIADMM_E_ARG, who + ": t_step0 >= 0 and t_step0 + 8 <= n_ref");
  if (c.n_ref > (1 << 20)) return fail(h, PIADMM_E_ARG, who + ": n_ref <= 2^20");
  for (int k = 0; k < c.n_scenarios; ++k)
    if (int rc = prob_check(h, who, prob, k)) return rc;
  return 0;
}

// Opens the plan both entry points share: `tab` holds tab_rows parameter rows (1: every scenario
// reads row 0, stride 0; n: one each), ref_traj ref_rows references of 2 x n_ref x 5 likewise.
// Everything was checked before; this is the first device call.
int plan_open(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob, const double* primal_thres,
              const double* dual_thres, const double* ref_traj, int ref_rows, const std::vector<double>& tab,
              int tab_rows, const double* state) {
  const int n = cfg->n_scenarios;
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (!h->plan) h->plan = new piadmm_obca_plan_s();
  piadmm_obca_plan_s* p = h->plan;
  *p = piadmm_obca_plan_s();      // everything an earlier plan owned goes; open == false until the end
  // the takeover: the resident local batch and its longest-first history end here
  h->n = 0;
  h->cost_n = 0;
  h->plan_taken = true;
  if (int rc = piadmm_obca_local_ensure(h, 2 * n)) return rc;
  if (int rc = piadmm_obca_edge_ensure(h, n)) return rc;
  const std::vector<int> ident = identity_list((size_t)2 * n);
  OWN_HIP(h, hipMemcpy(h->d_order, ident.data(), (size_t)2 * n * sizeof(int), hipMemcpyHostToDevice));

  p->cfg = *cfg;
  p->sigd = std::sqrt(0.95 / (1.0 - 0.95));
  p->n = n;
  const size_t ref_one = (size_t)2 * cfg->n_ref * 5;
  p->tab_rows = tab_rows;
  p->ref_rows = ref_rows;
  p->tab_stride = tab_rows > 1 ? TAB : 0;
  p->ref_stride = ref_rows > 1 ? (int)ref_one : 0;
  p->admm_rows.resize((size_t)tab_rows);
  for (int k = 0; k < tab_rows; ++k) p->admm_rows[(size_t)k] = (int)tab[(size_t)k * TAB + T_ADMM];
  p->max_iter_all = std::max(0, *std::max_element(p->admm_rows.begin(), p->admm_rows.end()));
  const size_t N = (size_t)n;
  int rc = 0;
  if ((rc = p->bar.alloc(h, N * STATE, false)) || (rc = p->barp.alloc(h, N * STATE, false)) ||
      (rc = p->ctrl.alloc(h, N * NCTRL, true)) || (rc = p->ctrlp.alloc(h, N * NCTRL, true)) ||
      (rc = p->X.alloc(h, N * NX, true)) || (rc = p->primal.alloc(h, N, true)) ||
      (rc = p->dual.alloc(h, N, true)) || (rc = p->pth.alloc(h, N, false)) ||
      (rc = p->dth.alloc(h, N, false)) || (rc = p->ref.alloc(h, ref_one * ref_rows, false)) ||
      (rc = p->tab.alloc(h, (size_t)tab_rows * TAB, false)) ||
      (rc = p->lamb.alloc(h, N * 126, true)) || (rc = p->iters.alloc(h, N, true)) ||
      (rc = p->stop.alloc(h, N, true)) || (rc = p->conv.alloc(h, N, true)) ||
      (rc = p->prob.alloc(h, N, false)) || (rc = p->act[0].alloc(h, N, false)) ||
      (rc = p->act[1].alloc(h, N, true)) || (rc = p->keep.alloc(h, N, true)) ||
      (rc = p->count.alloc(h, (size_t)1, true)) || (rc = p->mask.alloc(h, 2 * N, true)) ||
      (rc = p->h_count.alloc(h, 1, false))) {
    *p = piadmm_obca_plan_s();
    return rc;
  }
  OWN_HIP(h, hipMemcpy(p->bar, state, N * STATE * sizeof(double), hipMemcpyHostToDevice));
  OWN_HIP(h, hipMemcpy(p->barp, state, N * STATE * sizeof(double), hipMemcpyHostToDevice));
  OWN_HIP(h, hipMemcpy(p->pth, primal_thres, N * sizeof(double), hipMemcpyHostToDevice));
  OWN_HIP(h, hipMemcpy(p->dth, dual_thres, N * sizeof(double), hipMemcpyHostToDevice));
  OWN_HIP(h, hipMemcpy(p->ref, ref_traj, ref_one * ref_rows * sizeof(double), hipMemcpyHostToDevice));
  OWN_HIP(h, hipMemcpy(p->tab, tab.data(), (size_t)tab_rows * TAB * sizeof(double), hipMemcpyHostToDevice));
  OWN_HIP(h, hipMemcpy(p->prob, prob, N * sizeof(int), hipMemcpyHostToDevice));
  OWN_HIP(h, hipMemcpy(p->act[0], ident.data(), N * sizeof(int), hipMemcpyHostToDevice));
  p->t_step = cfg->t_step0;
  p->i_iter = 0;
  p->n_act = n;
  p->n_last = 0;
  p->cur = 0;
  p->open = true;
  return 0;
}
}  // namespace

// the staging buffer and the core arrays stay: only the attachments go
void piadmm_obca_plan_release(piadmm_obca_t h) {
  piadmm_obca_plan_s* p = h->plan;
  if (!p) return;
  if (p->tr.on || p->du.on || p->ord.on || p->ck.on || p->fb.on || p->dl.on || p->lp.on || p->lg.on) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    p->tr = {};
    p->du = {};
    p->ord = {};
    p->ck = {};
    p->fb = {};
    p->nz = {};    // the noise counts its steps by the feedback's: it goes whenever the feedback goes
    p->dl = {};
    p->lp = {};
    p->lg = {};
  }
  p->open = false;
}

// the plan's members free what they own
void piadmm_obca_plan_free(piadmm_obca_t h) {
  delete h->plan;
  h->plan = nullptr;
}

extern "C" {

int32_t piadmm_obca_plan_cfg_size(void) { return (int32_t)sizeof(piadmm_obca_plan_cfg_t); }

int32_t piadmm_obca_plan_begin(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob,
                               const double* primal_thres, const double* dual_thres, const double* ref_traj,
                               const double* state) {
  if (!h) return PIADMM_E_ARG;
  if (!cfg || !prob || !primal_thres || !dual_thres || !ref_traj || !state)
    return fail(h, PIADMM_E_ARG, "obca_plan_begin: null argument");
  std::vector<double> row(obca_plan::TAB);
  row_of_cfg(*cfg, row.data());
  if (const char* why = row_check(row.data())) return fail(h, PIADMM_E_ARG, std::string("obca_plan_begin: ") + why);
  if (int rc = shared_check(h, *cfg, prob, "obca_plan_begin")) return rc;
  return plan_open(h, cfg, prob, primal_thres, dual_thres, ref_traj, 1, row, 1, state);
}

int32_t piadmm_obca_fleet_begin(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob,
                                const double* primal_thres, const double* dual_thres, const double* ref_traj,
                                const double* par, const double* state) {
  if (!h) return PIADMM_E_ARG;
  if (!cfg || !prob || !primal_thres || !dual_thres || !ref_traj || !state)
    return fail(h, PIADMM_E_ARG, "obca_fleet_begin: null argument");
  if (int rc = shared_check(h, *cfg, prob, "obca_fleet_begin")) return rc;
  const int n = cfg->n_scenarios;
  // one row per scenario either way: without a table every row is the configuration's
  std::vector<double> tab((size_t)n * TAB);
  for (int k = 0; k < n; ++k) {
    double* row = tab.data() + (size_t)k * TAB;
    if (par) {
      for (int i = 0; i < TAB; ++i) row[i] = par[(size_t)k * TAB + i];
    } else {
      row_of_cfg(*cfg, row);
    }
    if (const char* why = row_check(row))
      return fail(h, PIADMM_E_ARG, "obca_fleet_begin: row " + std::to_string(k) + ": " + why);
  }
  return plan_open(h, cfg, prob, primal_thres, dual_thres, ref_traj, n, tab, n, state);
}

int32_t piadmm_obca_plan_iterate(piadmm_obca_t h, int32_t* n_active_after) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_iterate")) return rc;
  if (p->ck.on && p->ck.n_list == 0) return fail(h, PIADMM_E_STATE, "obca_plan_iterate: no scenario alive");
  if (p->n_act <= 0) return fail(h, PIADMM_E_STATE, "obca_plan_iterate: no active scenario (obca_plan_shift closes the step)");
  if (!p->ck.on && p->t_step + 8 > p->cfg.n_ref) return fail(h, PIADMM_E_STATE, "obca_plan_iterate: reference exhausted");
  if (const char* why = delay_refusal(p, 1)) return fail(h, PIADMM_E_STATE, std::string("obca_plan_iterate: ") + why);
  OWN_HIP(h, hipSetDevice(h->device));
  const int m = p->n_act;
  if (2 * m > h->cap || m > h->e_cap) return fail(h, PIADMM_E_STATE, "obca_plan_iterate: the handle's buffers shrank");
  hipStream_t st = h->stream;
  const int* act = p->act[p->cur];
  int* nxt = p->act[1 - p->cur];
  if (p->i_iter == 0) {
    // a new MPC step: the stop iterates and the status bits are the step's own
    OWN_HIP(h, hipMemsetAsync(p->iters, 0, (size_t)p->n * sizeof(int), st));
    OWN_HIP(h, hipMemsetAsync(p->mask, 0, (size_t)2 * p->n * sizeof(int), st));
  }
  const int i_iter = p->i_iter + 1;
  if (p->ck.on) {
    // every scenario's own 8 reference rows: its window, read as a reference of 8 rows at step 0
    hipLaunchKernelGGL(k_plan_pack_local, dim3(blocks_for(2 * m)), dim3(64 * PW), 0, st, act, m, p->bar, p->prob,
                       p->ck.win, WIN, 8, 0, p->tab, p->tab_stride, h->d_rec);
  } else {
    hipLaunchKernelGGL(k_plan_pack_local, dim3(blocks_for(2 * m)), dim3(64 * PW), 0, st, act, m, p->bar, p->prob, p->ref,
                       p->ref_stride, p->cfg.n_ref, p->t_step, p->tab, p->tab_stride, h->d_rec);
  }
  OWN_HIP(h, hipGetLastError());
  if (int rc = piadmm_obca_local_launch(h, 2 * m)) return rc;
  // the edge output starts from zeros, as in piadmm_obca_edge_solve
  OWN_HIP(h, hipMemsetAsync(h->e_out, 0, (size_t)m * EOUT * sizeof(double), st));
  if (p->dl.on || (p->lp.on && (p->lp.flags & 4))) {
    // the open step's latencies: the delay's, or the loop's (the two never attach together)
    hipLaunchKernelGGL(k_plan_exchange_stale, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, p->bar, p->prob,
                       h->d_out, p->tab, p->tab_stride, p->sigd, p->cfg.update_lamb_ij, p->ctrl, p->X, p->conv,
                       h->e_rec, p->dl.on ? (const double*)p->dl.tau : (const double*)p->lp.tau);
  } else {
    hipLaunchKernelGGL(k_plan_exchange, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, p->bar, p->prob, h->d_out,
                       p->tab, p->tab_stride, p->sigd, p->cfg.update_lamb_ij, p->ctrl, p->X, p->conv, h->e_rec);
  }
  OWN_HIP(h, hipGetLastError());
  if (int rc = piadmm_obca_edge_launch(h, m)) return rc;
  if (p->du.on) {
    // the law's lamb_bar_new and dres partials replace the fused update's in the edge output
    hipLaunchKernelGGL(k_plan_dual_pi, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, h->e_rec, h->e_out, h->e_ist,
                       p->du.par, p->du.stride, p->du.S, p->du.D, p->du.Sp, p->du.Dp);
    OWN_HIP(h, hipGetLastError());
  }
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_work, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, h->d_ist, h->e_ist, p->ord.work);
    OWN_HIP(h, hipGetLastError());
  }
  hipLaunchKernelGGL(k_plan_residual, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, i_iter, p->bar, p->barp,
                     p->ctrl, p->ctrlp, h->e_out, h->d_ist, h->e_ist, p->pth, p->dth, p->tab, p->tab_stride, p->primal,
                     p->dual,
                     p->stop, p->iters, p->mask, p->keep);
  OWN_HIP(h, hipGetLastError());
  // with the order on, the kept entries go to the scratch list and are sorted into the next list
  hipLaunchKernelGGL(k_plan_compact, dim3(1), dim3(CT), 0, st, act, p->keep, m, p->ord.on ? p->ord.tmp : nxt, p->count);
  OWN_HIP(h, hipGetLastError());
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(m)), dim3(64 * PW), 0, st, p->ord.tmp, p->count, m, p->ord.work,
                       nxt);
    OWN_HIP(h, hipGetLastError());
  }
  OWN_HIP(h, hipMemcpyAsync(p->h_count, p->count, sizeof(int), hipMemcpyDeviceToHost, st));
  OWN_HIP(h, hipStreamSynchronize(st));
  const int left = *p->h_count.get();
  if (left < 0 || left > m) return fail(h, PIADMM_E_STATE, "obca_plan_iterate: active count out of range");
  p->i_iter = i_iter;
  p->n_last = m;
  p->n_act = left;
  p->cur = 1 - p->cur;
  if (n_active_after) *n_active_after = left;
  return 0;
}

int32_t piadmm_obca_plan_shift(piadmm_obca_t h) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_shift")) return rc;
  if (const char* why = delay_refusal(p, 1)) return fail(h, PIADMM_E_STATE, std::string("obca_plan_shift: ") + why);
  if (p->n_act > 0) return fail(h, PIADMM_E_STATE, "obca_plan_shift: scenarios are still active");
  if (p->i_iter == 0) return fail(h, PIADMM_E_STATE, "obca_plan_shift: no iterate ran in this step");
  if (const char* why = step_refusal(p, 1)) return fail(h, PIADMM_E_STATE, std::string("obca_plan_shift: ") + why);
  OWN_HIP(h, hipSetDevice(h->device));
  if (p->ck.on) return clock_shift(h, p);
  if (p->fb.on) {
    // the plant step first: it reads the closing step's init_state and the stopping solution's first
    // control (k_plan_exchange wrote ctrl and X from the same local output), which the shift overwrites
    plant_io io = feedback_view(p, p->fb, p->fb.steps);
    if (p->nz.on) {
      // the step's disturbance rows first (the tape's row added in front), then read in the tape's place
      hipLaunchKernelGGL(k_plan_noise, dim3(lane_blocks(2 * p->n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr,
                         p->n, noise_view(p->nz, p->fb, p->fb.steps));
      OWN_HIP(h, hipGetLastError());
      io.w = p->nz.wbuf;  io.w_s = 10;
    }
    hipLaunchKernelGGL(k_plan_propagate, dim3(lane_blocks(2 * p->n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr,
                       p->n, io);
    OWN_HIP(h, hipGetLastError());
  }
  // every scenario is active again: the list the next iterate reads is the identity, or with the
  // order on the identity sorted by the work of the step that closes
  hipLaunchKernelGGL(k_plan_shift, dim3(p->n), dim3(64), 0, h->stream, p->n, p->bar, p->barp, p->X, p->lamb, p->ctrlp,
                     p->ord.on ? p->ord.tmp : p->act[p->cur]);
  OWN_HIP(h, hipGetLastError());
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->ord.tmp,
                       (const int*)nullptr, p->n, p->ord.work, p->act[p->cur]);
    OWN_HIP(h, hipGetLastError());
  }
  if (p->du.on) {
    hipLaunchKernelGGL(k_plan_dual_shift, dim3(p->n), dim3(64), 0, h->stream, p->n, p->du.S, p->du.D, p->du.Sp,
                       p->du.Dp);
    OWN_HIP(h, hipGetLastError());
  }
  if (p->fb.on) {
    // the state the vehicle reached over init_state of both copies, before the trace reads it
    hipLaunchKernelGGL(k_plan_set_init, dim3(lane_blocks(2 * p->n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr,
                       p->n, p->fb.next, p->bar, p->barp);
    OWN_HIP(h, hipGetLastError());
  }
  if (p->tr.on) {
    if (int rc = trace_append(h, p, p->tr.rows + 1)) return rc;
  }
  if (p->dl.on) {
    // the latencies of the step that opens
    if (int rc = delay_next(h, p)) return rc;
  }
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (p->tr.on) p->tr.rows += 1;
  if (p->fb.on) p->fb.steps += 1;
  if (p->dl.on) p->dl.steps += 1;
  p->t_step += 1;
  p->i_iter = 0;
  p->n_act = p->n;
  p->n_last = 0;
  return 0;
}

int32_t piadmm_obca_plan_step(piadmm_obca_t h, int32_t* iters_out) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_step")) return rc;
  if (p->ck.on && p->ck.n_list == 0) return fail(h, PIADMM_E_STATE, "obca_plan_step: no scenario alive");
  if (!p->ck.on && p->t_step + 8 > p->cfg.n_ref) return fail(h, PIADMM_E_STATE, "obca_plan_step: reference exhausted");
  if (const char* why = step_refusal(p, 1)) return fail(h, PIADMM_E_STATE, std::string("obca_plan_step: ") + why);
  if (const char* why = delay_refusal(p, 1)) return fail(h, PIADMM_E_STATE, std::string("obca_plan_step: ") + why);
  // i_iter > max_admm_iter stops a scenario: at most the largest max_admm_iter + 1 iterates in a step
  while (p->n_act > 0 && p->i_iter <= p->max_iter_all) {
    if (int rc = piadmm_obca_plan_iterate(h, nullptr)) return rc;
  }
  if (p->n_act > 0) return fail(h, PIADMM_E_STATE, "obca_plan_step: scenarios active after max_admm_iter + 1 iterates");
  if (iters_out) {
    OWN_HIP(h, hipMemcpyAsync(iters_out, p->iters, (size_t)p->n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    OWN_HIP(h, hipStreamSynchronize(h->stream));
  }
  return piadmm_obca_plan_shift(h);
}

int32_t piadmm_obca_plan_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_get")) return rc;
  const int64_t n = p->n, m = p->n_last, D = sizeof(double), I = sizeof(int32_t);
  const void* src = nullptr;
  int64_t want = -1;
  bool host = false;       // the item is a value of the plan's, not a device array
  const int32_t counts[3] = {p->n_last, p->n_act, p->i_iter};
  const uint64_t seed[2] = {p->nz.seed, (uint64_t)p->nz.k0};
  const uint64_t dseed[3] = {p->dl.seed, (uint64_t)p->dl.k0, (uint64_t)p->dl.steps};
  const uint64_t lseed[3] = {p->lp.seed, (uint64_t)p->lp.k0, (uint64_t)p->lp.flags};
  switch (what) {
    case PIADMM_OBCA_PLAN_GET_STATE: src = p->bar; want = n * STATE * D; break;
    case PIADMM_OBCA_PLAN_GET_STATE_PREV: src = p->barp; want = n * STATE * D; break;
    case PIADMM_OBCA_PLAN_GET_CTRL: src = p->ctrl; want = n * NCTRL * D; break;
    case PIADMM_OBCA_PLAN_GET_CTRL_PREV: src = p->ctrlp; want = n * NCTRL * D; break;
    case PIADMM_OBCA_PLAN_GET_X: src = p->X; want = n * NX * D; break;
    case PIADMM_OBCA_PLAN_GET_ITERS: src = p->iters; want = n * I; break;
    case PIADMM_OBCA_PLAN_GET_ACTIVE: src = p->act[1 - p->cur]; want = m * I; break;
    case PIADMM_OBCA_PLAN_GET_PRIMAL: src = p->primal; want = n * D; break;
    case PIADMM_OBCA_PLAN_GET_DUAL: src = p->dual; want = n * D; break;
    case PIADMM_OBCA_PLAN_GET_STOP: src = p->stop; want = n * I; break;
    case PIADMM_OBCA_PLAN_GET_CONVERGE: src = p->conv; want = n * I; break;
    case PIADMM_OBCA_PLAN_GET_LOCAL_REC: src = h->d_rec; want = 2 * m * REC * D; break;
    case PIADMM_OBCA_PLAN_GET_LOCAL_OUT: src = h->d_out; want = 2 * m * OUT * D; break;
    case PIADMM_OBCA_PLAN_GET_LOCAL_IST: src = h->d_ist; want = 2 * m * 3 * I; break;
    case PIADMM_OBCA_PLAN_GET_EDGE_REC: src = h->e_rec; want = m * EREC * D; break;
    case PIADMM_OBCA_PLAN_GET_EDGE_OUT: src = h->e_out; want = m * EOUT * D; break;
    case PIADMM_OBCA_PLAN_GET_EDGE_IST: src = h->e_ist; want = m * NT * 3 * I; break;
    case PIADMM_OBCA_PLAN_GET_LAMBDA: src = p->lamb; want = n * 126 * D; break;
    case PIADMM_OBCA_PLAN_GET_STATUS_MASK: src = p->mask; want = 2 * n * I; break;
    case PIADMM_OBCA_PLAN_GET_REF: src = p->ref; want = (int64_t)p->ref_rows * 2 * p->cfg.n_ref * 5 * D; break;
    case PIADMM_OBCA_PLAN_GET_PAR: src = p->tab; want = (int64_t)p->tab_rows * TAB * D; break;
    case PIADMM_OBCA_PLAN_GET_DUAL_S:
    case PIADMM_OBCA_PLAN_GET_DUAL_D:
    case PIADMM_OBCA_PLAN_GET_DUAL_PAR:
    case PIADMM_OBCA_PLAN_GET_DUAL_S_PREV:
    case PIADMM_OBCA_PLAN_GET_DUAL_D_PREV:
      if (!p->du.on) return fail(h, PIADMM_E_STATE, "obca_plan_get: no dual law attached (obca_dual_plan)");
      if (what == PIADMM_OBCA_PLAN_GET_DUAL_PAR) { src = p->du.par; want = (int64_t)p->du.rows * DPAR * D; break; }
      src = what == PIADMM_OBCA_PLAN_GET_DUAL_S ? p->du.S : what == PIADMM_OBCA_PLAN_GET_DUAL_D ? p->du.D
            : what == PIADMM_OBCA_PLAN_GET_DUAL_S_PREV ? p->du.Sp : p->du.Dp;
      want = n * 126 * D;
      break;
    case PIADMM_OBCA_PLAN_GET_PRIMAL_THRES: src = p->pth; want = n * D; break;
    case PIADMM_OBCA_PLAN_GET_DUAL_THRES: src = p->dth; want = n * D; break;
    case PIADMM_OBCA_PLAN_GET_PROB: src = p->prob; want = n * I; break;
    case PIADMM_OBCA_PLAN_GET_WORK:
      if (!p->ord.on) return fail(h, PIADMM_E_STATE, "obca_plan_get: no order attached (obca_order_plan)");
      src = p->ord.work; want = n * 2 * I; break;
    case PIADMM_OBCA_PLAN_GET_CLOCK:
    case PIADMM_OBCA_PLAN_GET_WINDOW:
      if (!p->ck.on) return fail(h, PIADMM_E_STATE, "obca_plan_get: no clock attached (obca_clock_plan)");
      if (what == PIADMM_OBCA_PLAN_GET_CLOCK) { src = p->ck.clk; want = n * 3 * I; }
      else { src = p->ck.win; want = n * WIN * D; }
      break;
    case PIADMM_OBCA_PLAN_GET_FEEDBACK_PAR:
    case PIADMM_OBCA_PLAN_GET_FEEDBACK_STEPS:
      if (!p->fb.on) return fail(h, PIADMM_E_STATE, "obca_plan_get: no feedback attached (obca_feedback_plan)");
      if (what == PIADMM_OBCA_PLAN_GET_FEEDBACK_PAR) { src = p->fb.par; want = (int64_t)p->fb.rows * FPAR * D; }
      else { src = &p->fb.steps; want = I; host = true; }
      break;
    case PIADMM_OBCA_NOISE_GET_PAR:
    case PIADMM_OBCA_NOISE_GET_STREAMS:
    case PIADMM_OBCA_NOISE_GET_SEED:
      if (!p->nz.on) return fail(h, PIADMM_E_STATE, "obca_plan_get: no noise attached (obca_noise_plan)");
      if (what == PIADMM_OBCA_NOISE_GET_PAR) { src = p->nz.par; want = (int64_t)p->nz.rows * ZPAR * D; }
      else if (what == PIADMM_OBCA_NOISE_GET_STREAMS) { src = p->nz.streams; want = n * (int64_t)sizeof(int64_t); }
      else { src = seed; want = 2 * (int64_t)sizeof(uint64_t); host = true; }
      break;
    case PIADMM_OBCA_DELAY_GET_PAR:
    case PIADMM_OBCA_DELAY_GET_TAU:
    case PIADMM_OBCA_DELAY_GET_STREAMS:
    case PIADMM_OBCA_DELAY_GET_SEED:
      if (!p->dl.on) return fail(h, PIADMM_E_STATE, "obca_plan_get: no delay attached (obca_delay_plan)");
      if (what == PIADMM_OBCA_DELAY_GET_PAR) { src = p->dl.par; want = (int64_t)p->dl.rows * YPAR * D; }
      else if (what == PIADMM_OBCA_DELAY_GET_TAU) { src = p->dl.tau; want = n * 2 * D; }
      else if (what == PIADMM_OBCA_DELAY_GET_STREAMS) { src = p->dl.streams; want = n * (int64_t)sizeof(int64_t); }
      else { src = dseed; want = 3 * (int64_t)sizeof(uint64_t); host = true; }
      break;
    case PIADMM_OBCA_LOOP_GET_PLANT:
    case PIADMM_OBCA_LOOP_GET_NOISE:
    case PIADMM_OBCA_LOOP_GET_DELAY:
    case PIADMM_OBCA_LOOP_GET_TAU:
    case PIADMM_OBCA_LOOP_GET_STREAMS:
    case PIADMM_OBCA_LOOP_GET_SEED:
      if (!p->lp.on) return fail(h, PIADMM_E_STATE, "obca_plan_get: no loop attached (obca_loop_plan)");
      if (what == PIADMM_OBCA_LOOP_GET_PLANT) { src = p->lp.plant; want = (int64_t)p->lp.plant_rows * FPAR * D; }
      else if (what == PIADMM_OBCA_LOOP_GET_NOISE) {
        if (!(p->lp.flags & 2)) return fail(h, PIADMM_E_STATE, "obca_plan_get: the loop has no noise rows");
        src = p->lp.noise; want = (int64_t)p->lp.noise_rows * ZPAR * D;
      } else if (what == PIADMM_OBCA_LOOP_GET_DELAY) {
        if (!(p->lp.flags & 4)) return fail(h, PIADMM_E_STATE, "obca_plan_get: the loop has no delay rows");
        src = p->lp.delay; want = (int64_t)p->lp.delay_rows * YPAR * D;
      } else if (what == PIADMM_OBCA_LOOP_GET_TAU) { src = p->lp.tau; want = n * 2 * D; }
      else if (what == PIADMM_OBCA_LOOP_GET_STREAMS) { src = p->lp.streams; want = n * (int64_t)sizeof(int64_t); }
      else { src = lseed; want = 3 * (int64_t)sizeof(uint64_t); host = true; }
      break;
    case PIADMM_OBCA_PLAN_GET_T_STEP: src = &p->t_step; want = I; host = true; break;
    case PIADMM_OBCA_PLAN_GET_COUNTS: src = counts; want = 3 * I; host = true; break;
    default: return fail(h, PIADMM_E_ARG, "obca_plan_get: unknown item " + std::to_string(what));
  }
  return get_finish(h, "obca_plan_get", what, src, host, want, out, bytes);
}

int32_t piadmm_obca_plan_end(piadmm_obca_t h) {
  if (!h) return PIADMM_E_ARG;
  if (!h->plan) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  piadmm_obca_plan_free(h);
  return 0;
}

}  // extern "C"
