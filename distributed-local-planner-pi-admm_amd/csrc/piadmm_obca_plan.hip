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

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "pd_common.h"
#include "piadmm.h"
#include "piadmm_obca_handle.h"

namespace obca_plan {

constexpr int NT = 7;
constexpr int PW = 4;                          // waves per workgroup
constexpr int STATE = PIADMM_OBCA_PLAN_STATE;
constexpr int REC = PIADMM_OBCA_REC, OUT = PIADMM_OBCA_OUT;
constexpr int EREC = PIADMM_OBCA_EDGE_REC, EOUT = PIADMM_OBCA_EDGE_OUT;
// the state's fields (include/piadmm.h)
constexpr int S_ZB = 0, S_A = 126, S_B = 238, S_LB = 294, S_LIJ = 420, S_LX = 476, S_INIT = 546;
static_assert(S_INIT + 10 == STATE, "state layout");
// local record / output (csrc/piadmm_obca.hip), edge record / output (csrc/piadmm_obca_edge.hip)
constexpr int R_INIT = 0, R_REF = 5, R_AO = 45, R_BO = 101, R_LIJ = 129, R_LB = 157, R_ZB = 220, R_PAR = 283;
constexpr int O_X = 0, O_U = 40, O_LAM = 54;
constexpr int E_LX = 0, E_LIJ = 70, E_LB = 126, E_PAR = 252;
constexpr int EO_ZB = 126, EO_LBN = 252, EO_DRES = 532;
constexpr int NCTRL = 28, NX = 80;

constexpr double LENGTH = 3.5, WIDTH = 2.0;
constexpr double AVG_DELAY = 0.05, VAR_DELAY = 0.025;

// a parameter row (include/piadmm.h): the integers are stored as doubles, as the records do
constexpr int TAB = PIADMM_OBCA_FLEET_PAR;
constexpr int T_RHO = 0, T_MIN_DIS = 1, T_CONV = 2, T_MAX_X = 3, T_MAX_Y = 4, T_R = 5, T_Q = 6, T_XB = 7,
              T_MU = 8, T_G = 9, T_ADMM = 10, T_SQP = 11, T_ROUND = 12, T_START = 13;
// the row entry behind parameter j of a local / an edge record, one hex digit each (prob, local 6
// and edge 2, comes from prob[])
constexpr unsigned LOCAL_PAR_ROW = 0xB0654310u;            // rho, min_dis, max_x, max_y, r, q, -, max_sqp_iter
constexpr unsigned long long EDGE_PAR_ROW = 0x987DCB010ull;  // rho, min_dis, -, max_sqp_iter, round_decimals, start,
                                                             // x_bound, mu_max, g_max
static_assert(T_START < TAB, "row layout");

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

// (A, b) of a vehicle at `st` -- halfspaces (piadmm/obca.py) in the host's order of operations,
// products and sums kept apart (no contraction) so the two stay within rounding of each other.
__device__ __forceinline__ void halfspaces(const double* st, int prob, double sigd, double A[4][2], double b[4]) {
#pragma clang fp contract(off)
  const double x = st[0], y = st[1], vel = st[2], th = st[3];
  const double c = cos(th), s = sin(th);
  double dx = 0.0, dy = 0.0;
  A[0][0] = c;  A[0][1] = s;
  A[2][0] = -c; A[2][1] = -s;
  if (prob) {
    A[1][0] = -s; A[1][1] = c;
    A[3][0] = s;  A[3][1] = -c;
    const double qx = VAR_DELAY * vel * c, qy = VAR_DELAY * vel * s;
    dx = AVG_DELAY * vel * c + sigd * (qx * qx);
    dy = AVG_DELAY * vel * s + sigd * (qy * qy);
  } else {
    A[1][0] = s;  A[1][1] = -c;
    A[3][0] = -s; A[3][1] = c;
  }
  const double px = x + dx, py = y + dy;
  const double b0[4] = {LENGTH / 2, WIDTH / 2, LENGTH / 2, WIDTH / 2};
#pragma unroll
  for (int i = 0; i < 4; ++i) b[i] = b0[i] + (A[i][0] * px + A[i][1] * py);
}

// One wave per active scenario; lane < 14 owns the (vehicle, slot) item lane = v * 7 + t.
__global__ void __launch_bounds__(64 * PW) k_plan_exchange(const int* __restrict__ active, int n_act,
                                                           double* __restrict__ bar, const int* __restrict__ prob,
                                                           const double* __restrict__ lout,
                                                           const double* __restrict__ tab, int tab_stride,
                                                           double sigd, int update_lamb_ij,
                                                           double* __restrict__ ctrl, double* __restrict__ X,
                                                           int* __restrict__ conv, double* __restrict__ erecs) {
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
constexpr int CT = 256;
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

// ---------------------------------------------------------------------------------------------
// The PI anti-windup dual law (piadmm_obca_dual_plan): the per-edge PI of
// ADMM_CVX_two_veh_intesection_PI_antiwindup.m:156-188 with a constant proportional gain, on the
// consensus error of the plan.  Opt-in: without a law neither kernel is launched.
// ---------------------------------------------------------------------------------------------
// a gains row (include/piadmm.h)
constexpr int DPAR = PIADMM_OBCA_DUAL_PAR;
constexpr int G_KP = 0, G_KI = 1, G_SAT = 2, G_DGAIN = 3, G_WINDUP = 4;
static_assert(G_WINDUP < DPAR, "gains row layout");

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
// The run record ("trace") of an open plan: k_plan_trace copies a closed step's row, and
// k_plan_clearance measures how close the two vehicles are at the states the row holds.
// ---------------------------------------------------------------------------------------------
constexpr int TSUM = 4;     // summary per scenario: min plain clearance, its row, min tightened clearance, sum of iterates

// One wave per scenario: row `row` of the record after k_plan_shift -- the new init_state and, for
// row >= 1, what the step that was closed left behind (the stop iterate, both status masks, the
// stopping iterate's residuals and, where kept, the step's lamb_bar).  Row 0 is the state the trace
// was attached at and has no step.  Pure copies; lane 0 owns the scenario's sum of iterates.
__global__ void __launch_bounds__(64 * PW) k_plan_trace(int n, int row, const double* __restrict__ bar,
                                                        const int* __restrict__ iters, const int* __restrict__ mask,
                                                        const double* __restrict__ primal,
                                                        const double* __restrict__ dual,
                                                        const double* __restrict__ lamb,
                                                        double* __restrict__ t_states, int* __restrict__ t_iters,
                                                        int* __restrict__ t_mask, double* __restrict__ t_primal,
                                                        double* __restrict__ t_dual, double* __restrict__ t_lamb,
                                                        double* __restrict__ summary) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= n) return;
  const size_t N = (size_t)n, S = (size_t)s;
  if (lane < 10) t_states[((size_t)row * N + S) * 10 + lane] = bar[S * STATE + S_INIT + lane];
  if (row == 0) {
    if (lane == 0) summary[S * TSUM + 3] = 0.0;
    return;
  }
  const size_t r = (size_t)(row - 1) * N + S;          // the step's index in the per-step arrays
  if (lane < 2) t_mask[r * 2 + lane] = mask[2 * S + lane];
  if (t_lamb)
    for (int i = lane; i < 126; i += 64) t_lamb[r * 126 + i] = lamb[S * 126 + i];
  if (lane == 0) {
    const int it = iters[s];
    t_iters[r] = it;
    t_primal[r] = primal[s];
    t_dual[r] = dual[s];
    summary[S * TSUM + 3] = summary[S * TSUM + 3] + (double)it;
  }
}

// One wave per scenario: the exact minimum distance between the two vehicles' rectangles
// (generate_vehicle_vertices, util.py:34-42) at the state pair st[2][5] = states + s * stride, for
// two box sets at once: the plain boxes (centre x, y) and the delay-tightened ones the planner
// constrains (compute_square_halfspaces_ca_prob, util.py:70-101: each centre moved as halfspaces()
// above moves it; prob = 0 moves nothing, so both outputs are the plain value).  The distance is 0
// when no edge normal of either rectangle separates them (SAT over the 4 axes), else the minimum of
// the 32 vertex-to-edge distances.  Lane = set * 32 + dir * 16 + vertex * 4 + edge: a vertex of
// vehicle `dir` against an edge of the other vehicle, whose normal (edge & 1: the lateral one) is
// the lane's SAT axis.  piadmm.obca.clearance is the same statements on the host; products and
// sums are kept apart (no contraction).  With `summary`, lane 0 keeps the scenario's running
// minima: row 0 starts them, a later row replaces the plain minimum only when it is smaller, so
// the row kept is the first at which the minimum was reached.
__global__ void __launch_bounds__(64 * PW) k_plan_clearance(int n, const double* __restrict__ states, int stride,
                                                            const int* __restrict__ prob, double sigd, int row,
                                                            double* __restrict__ out,
                                                            double* __restrict__ summary) {
#pragma clang fp contract(off)
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= n) return;
  const double* st = states + (size_t)s * stride;
  const int pr = prob[s];
  const int set = lane >> 5, dir = (lane >> 4) & 1, vi = (lane >> 2) & 3, ej = lane & 3;
  constexpr double HL = LENGTH / 2, HW = WIDTH / 2;
  // box a owns the lane's vertex, box o its edge
  const double* sa = st + dir * 5;
  const double* so = st + (1 - dir) * 5;
  const double ca = cos(sa[3]), sna = sin(sa[3]), co = cos(so[3]), sno = sin(so[3]);
  double ax = sa[0], ay = sa[1], ox = so[0], oy = so[1];
  if (set == 1 && pr) {
    const double va = sa[2], vo = so[2];
    const double qax = VAR_DELAY * va * ca, qay = VAR_DELAY * va * sna;
    const double qox = VAR_DELAY * vo * co, qoy = VAR_DELAY * vo * sno;
    const double dax = AVG_DELAY * va * ca + sigd * (qax * qax), day = AVG_DELAY * va * sna + sigd * (qay * qay);
    const double dox = AVG_DELAY * vo * co + sigd * (qox * qox), doy = AVG_DELAY * vo * sno + sigd * (qoy * qoy);
    ax = ax + dax;  ay = ay + day;
    ox = ox + dox;  oy = oy + doy;
  }
  // vertex i = centre + sl e + sw n: (+, +), (+, -), (-, -), (-, +)
  const double pl = vi < 2 ? HL : -HL, pw = (vi == 0 || vi == 3) ? HW : -HW;
  const double px = ax + pl * ca - pw * sna, py = ay + pl * sna + pw * ca;
  const int e1 = (ej + 1) & 3;
  const double al = ej < 2 ? HL : -HL, aw = (ej == 0 || ej == 3) ? HW : -HW;
  const double bl = e1 < 2 ? HL : -HL, bw = (e1 == 0 || e1 == 3) ? HW : -HW;
  const double e0x = ox + al * co - aw * sno, e0y = oy + al * sno + aw * co;
  const double e1x = ox + bl * co - bw * sno, e1y = oy + bl * sno + bw * co;
  const double abx = e1x - e0x, aby = e1y - e0y, apx = px - e0x, apy = py - e0y;
  double t = (apx * abx + apy * aby) / (abx * abx + aby * aby);
  t = fmin(fmax(t, 0.0), 1.0);
  const double rx = apx - t * abx, ry = apy - t * aby;
  const double dist = sqrt(rx * rx + ry * ry);
  // SAT along the edge's normal: |centre distance| against the two half extents
  const bool lateral = ej & 1;
  const double ux = lateral ? -sno : co, uy = lateral ? co : sno;
  const double cdx = ax - ox, cdy = ay - oy;
  const double pc = fabs(cdx * ux + cdy * uy);
  const double pe = fabs(ca * ux + sna * uy), pn = fabs(ca * uy - sna * ux);
  const double gap = pc - ((lateral ? HW : HL) + (HL * pe + HW * pn));
  // every lane is active here: the reductions are DPP scans over the whole wave
  const double inf = __builtin_inf();
  const double g0 = pd::wmax(set == 0 ? gap : -inf), g1 = pd::wmax(set == 1 ? gap : -inf);
  const double d0 = pd::wmin(set == 0 ? dist : inf), d1 = pd::wmin(set == 1 ? dist : inf);
  const double plain = g0 > 0.0 ? d0 : 0.0, tight = g1 > 0.0 ? d1 : 0.0;
  if (lane == 0) {
    out[(size_t)s * 2] = plain;
    out[(size_t)s * 2 + 1] = tight;
    if (summary) {
      double* S = summary + (size_t)s * TSUM;
      if (row == 0) {
        S[0] = plain;  S[1] = 0.0;  S[2] = tight;
      } else {
        if (plain < S[0]) { S[0] = plain;  S[1] = (double)row; }
        if (tight < S[2]) S[2] = tight;
      }
    }
  }
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
constexpr int WIN = 2 * 8 * 5;       // a window: ref_s[v][c .. c + 7], the 80 doubles k_plan_pack_local reads

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

// the plan's per-scenario arrays, by value.  S .. gains: only with a law (`law`); win, work, clk:
// nullptr without the clock / the order.  The strides are 0 where the plan shares one row.
struct tenant_arrays {
  double *bar, *barp, *ctrl, *ctrlp, *X, *lamb, *primal, *dual, *pth, *dth, *tab, *ref, *win, *S, *D, *Sp, *Dp, *gains;
  int *iters, *stop, *conv, *prob, *mask, *work, *clk;
  int tab_stride, ref_stride, g_stride, n_ref, t_step, law, f64_words;
};

// dst[0 .. len) = src[0 .. len) by the 64 lanes of a wave in strided passes: 16 bytes a lane where
// both ends sit on a 16-byte boundary and len is even, 8 bytes a lane otherwise.  The pointers are
// wave-uniform, so the choice is.
__device__ __forceinline__ void copy_seg(double* dst, const double* src, int len, int lane) {
  const bool wide = ((((uintptr_t)dst) | ((uintptr_t)src)) & 15u) == 0 && (len & 1) == 0;
  if (wide) {
    double2* d2 = reinterpret_cast<double2*>(dst);
    const double2* s2 = reinterpret_cast<const double2*>(src);
    for (int i = lane; i < len / 2; i += 64) d2[i] = s2[i];
  } else {
    for (int i = lane; i < len; i += 64) dst[i] = src[i];
  }
}

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

// ---------------------------------------------------------------------------------------------
// Closed-loop feedback (piadmm_obca_feedback_plan / _measure, piadmm_obca_propagate): the plant step
// between two MPC steps and the scatter of states over init_state.  Opt-in: without the attachment
// neither kernel is launched by piadmm_obca_plan_shift.
// ---------------------------------------------------------------------------------------------
// a plant row (include/piadmm.h): 8 doubles per vehicle, vehicle 0 first
constexpr int FPAR = PIADMM_OBCA_FEEDBACK_PAR, FV = FPAR / 2;
constexpr int F_METHOD = 0, F_NSUB = 1, F_LR = 2, F_LF = 3, F_GA = 4, F_GW = 5, F_AMAX = 6, F_WMAX = 7;
constexpr int F_NSUB_MAX = 64;
constexpr double PLANT_DT = 0.1, MAX_STEER = 0.6;
static_assert(F_WMAX + 1 == FV && FV % 2 == 0, "plant row layout");

// One plant step of one vehicle, all in registers: x (5) <- F(x, (a, om)) under the vehicle's row P
// (8), without the disturbance.  n_sub substeps of DT / n_sub; a substep is 1 stage (Euler) or 4
// (classical RK4) of the one right-hand side below, the stage loop kept rolled so that the libm
// calls are inlined once; then delta is clipped.  n_sub is clamped to its range, so the loop is
// bounded whatever the row holds.  piadmm.obca.propagate is the same statements on the host;
// products and sums are kept apart (no contraction).  The body of both entry points of
// k_plan_propagate: the stand-alone call and the in-plan step give the same bits.
__device__ __forceinline__ void plant_step(double x[5], double a, double om, const double P[FV]) {
#pragma clang fp contract(off)
  const double lr = P[F_LR], lf = P[F_LF];
  const double a_eff = fmin(P[F_AMAX], fmax(P[F_GA] * a, -P[F_AMAX]));
  const double w_eff = fmin(P[F_WMAX], fmax(P[F_GW] * om, -P[F_WMAX]));
  const int n_sub = min(max((int)P[F_NSUB], 1), F_NSUB_MAX);
  const int n_stage = P[F_METHOD] != 0.0 ? 4 : 1;
  const double hs = PLANT_DT / (double)n_sub;
  const double scale = n_stage == 4 ? hs / 6.0 : hs;
#pragma unroll 1
  for (int sub = 0; sub < n_sub; ++sub) {
    double xs[5], acc[5];
#pragma unroll
    for (int i = 0; i < 5; ++i) { xs[i] = x[i]; acc[i] = 0.0; }
#pragma unroll 1
    for (int st = 0; st < n_stage; ++st) {
      const double beta = atan(lr * tan(xs[4]) / (lr + lf));
      const double ph = xs[3] + beta;
      const double f[5] = {xs[2] * cos(ph), xs[2] * sin(ph), a_eff, xs[2] / lr * sin(beta), w_eff};
      const double wgt = (st == 1 || st == 2) ? 2.0 : 1.0;
      const double c = st < 2 ? 0.5 * hs : hs;          // the next stage's point: x + c f
#pragma unroll
      for (int i = 0; i < 5; ++i) {
        acc[i] = st == 0 ? f[i] : acc[i] + wgt * f[i];
        xs[i] = x[i] + c * f[i];
      }
    }
#pragma unroll
    for (int i = 0; i < 5; ++i) x[i] = x[i] + scale * acc[i];
    x[4] = fmin(MAX_STEER, fmax(x[4], -MAX_STEER));
  }
}

// where the arrays of one k_plan_propagate launch sit, all indexed by scenario: the strides in
// doubles per scenario; the vehicle's state row at + v * 5, its controls a and omega at
// ctrl + v * ctrl_v and + ctrl_w behind it, its plant row at + v * 8 (par_s = 0: one shared row),
// its disturbance row at + v * 5 (w = nullptr: none), its result at out + s * 10 + v * 5
struct plant_io {
  const double *x0, *ctrl, *par, *w;
  double* out;
  long long x0_s, w_s;
  int ctrl_s, ctrl_v, ctrl_w, par_s;
};

// One lane per vehicle: lane g of the grid = vehicle g & 1 of entry g >> 1 of `list` (nullptr: of
// scenario g >> 1), 2 m lanes.  No LDS; the state, the stage point and the RK4 sum stay in
// registers over the runtime substep loop.  The plant row is 64 bytes on a 64-byte boundary (the
// base comes from hipMalloc): four 16-byte loads.  The 5-wide rows (state, disturbance, result) are
// 40 bytes, only 8-byte aligned for the odd vehicle and inside the plan's state: five 8-byte
// accesses each; neighbouring lanes hold neighbouring rows, so a wave's accesses fall into the
// same few cache lines.
__global__ void __launch_bounds__(64 * PW) k_plan_propagate(const int* __restrict__ list, int m, plant_io io) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * m) return;
  const int v = g & 1;
  const size_t s = (size_t)(list ? list[g >> 1] : (g >> 1));
  const double2* P2 = reinterpret_cast<const double2*>(io.par + s * io.par_s + v * FV);
  double P[FV];
#pragma unroll
  for (int i = 0; i < FV / 2; ++i) {
    const double2 q = P2[i];
    P[2 * i] = q.x;
    P[2 * i + 1] = q.y;
  }
  const double* xin = io.x0 + s * io.x0_s + v * 5;
  const double* cu = io.ctrl + s * io.ctrl_s + v * io.ctrl_v;
  double x[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) x[i] = xin[i];
  plant_step(x, cu[0], cu[io.ctrl_w], P);
  double* o = io.out + s * 10 + v * 5;
  if (io.w) {
#pragma clang fp contract(off)
    const double* wr = io.w + s * io.w_s + v * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = x[i] + wr[i];
  } else {
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = x[i];
  }
}

// One lane per vehicle, 2 m lanes: init_state of both state copies of scenario list[k] (nullptr: of
// scenario k) = states[k] (m x 2 x 5).  Pure copies; nothing else of the state is written.
__global__ void __launch_bounds__(64 * PW) k_plan_set_init(const int* __restrict__ list, int m,
                                                           const double* __restrict__ states,
                                                           double* __restrict__ bar, double* __restrict__ barp) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * m) return;
  const int k = g >> 1, v = g & 1;
  const size_t s = (size_t)(list ? list[k] : k);
  const double* src = states + (size_t)k * 10 + v * 5;
  const size_t at = s * STATE + S_INIT + v * 5;
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    const double val = src[i];
    bar[at + i] = val;
    barp[at + i] = val;
  }
}

// ---------------------------------------------------------------------------------------------
// Device-side disturbance noise (piadmm_obca_noise_plan / piadmm_obca_noise_tape): the disturbance
// row of stream t at step k as a pure function of (seed, t, k).  Opt-in: without the attachment
// piadmm_obca_plan_shift does not launch k_plan_noise.
// ---------------------------------------------------------------------------------------------
// a noise row (include/piadmm.h): sigma[2][5], bias[2][5], trunc, one reserved zero
constexpr int ZPAR = PIADMM_OBCA_NOISE_PAR;
constexpr int Z_SIGMA = 0, Z_BIAS = 10, Z_TRUNC = 20, Z_RESERVED = 21;
static_assert(Z_RESERVED + 1 == ZPAR, "noise row layout");

// Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11):
// c the counter's four words, replaced by the result; (k0, k1) the key.  Ten rounds of two
// 32 x 32 -> 64 products (the high halves by __umulhi), the key bumped between rounds.  All 32-bit.
__device__ __forceinline__ void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
  constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
    const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
    c[0] = hi1 ^ c[1] ^ k0;
    c[1] = lo1;
    c[2] = hi0 ^ c[3] ^ k1;
    c[3] = lo0;
    k0 += W0;
    k1 += W1;
  }
}

// The five disturbances of vehicle v of stream t at step k under the row's sigma S, bias B and
// trunc: three Philox calls at counter (k, 4 v + j, t low, t high), each giving two uniforms in
// (0, 1) on 52 bits and by Box-Muller two normals; the sixth normal is discarded.  raw (12 words,
// or nullptr) receives the calls' words.  piadmm.obca.noise_tape is the same statements on the
// host; products and sums are kept apart (no contraction), so sigma = 0 gives the bias bit for bit.
// The body of k_plan_noise for the in-plan step and for the stand-alone tape: the same bits.
__device__ __forceinline__ void noise_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t t_lo, uint32_t t_hi,
                                           uint32_t k, int v, const double S[5], const double B[5], double trunc,
                                           double w[5], uint32_t* raw) {
#pragma clang fp contract(off)
  double z[6];
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    uint32_t c[4] = {k, (uint32_t)(4 * v + j), t_lo, t_hi};
    philox4x32_10(c, seed_lo, seed_hi);
    if (raw) {
#pragma unroll
      for (int q = 0; q < 4; ++q) raw[4 * j + q] = c[q];
    }
    const unsigned long long a = ((unsigned long long)c[0] << 32) | c[1];
    const unsigned long long b = ((unsigned long long)c[2] << 32) | c[3];
    const double u1 = ((double)(a >> 12) + 0.5) * 0x1p-52;
    const double u2 = ((double)(b >> 12) + 0.5) * 0x1p-52;
    const double rad = sqrt(-2.0 * log(u1));
    const double ang = 6.283185307179586 * u2;
    z[2 * j] = rad * cos(ang);
    z[2 * j + 1] = rad * sin(ang);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double zi = z[i];
    if (trunc != 0.0) zi = fmin(trunc, fmax(zi, -trunc));
    w[i] = B[i] + S[i] * zi;
  }
}

// where the arrays of one k_plan_noise launch sit, indexed by scenario: par the noise rows (par_s =
// 0: one shared row), streams the stream ids (nullptr: the scenario's number), tape the rows added
// in front (nullptr: none), out the result, raw the Philox words (nullptr: not kept); the strides
// in elements per scenario, and per step index (blockIdx.y) 10 doubles of tape and out and 24 words
// of raw; k = the step index of blockIdx.y = 0
struct noise_io {
  const double *par, *tape;
  const long long* streams;
  double* out;
  uint32_t* raw;
  long long tape_s, out_s, raw_s;
  uint32_t seed_lo, seed_hi, k;
  int par_s;
};

// One lane per vehicle: lane g of a grid row = vehicle g & 1 of entry g >> 1 of `list` (nullptr: of
// scenario g >> 1), 2 m lanes; grid row y is step index k + y (the in-plan step launches one row).
// No LDS, no atomics, nothing shared between lanes: the counter is the lane's own, the arithmetic
// 32-bit integer and fp64 in registers.  The lane's 11 parameters are 8-byte loads from the row;
// its five results 8-byte stores, neighbouring lanes to neighbouring rows as in k_plan_propagate.
// With a tape the written value is tape + w, the tape term first.
__global__ void __launch_bounds__(64 * PW) k_plan_noise(const int* __restrict__ list, int m, noise_io io) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * m) return;
  const int v = g & 1;
  const size_t s = (size_t)(list ? list[g >> 1] : (g >> 1));
  const size_t y = blockIdx.y;
  const double* P = io.par + s * io.par_s;
  double S[5], B[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    S[i] = P[Z_SIGMA + v * 5 + i];
    B[i] = P[Z_BIAS + v * 5 + i];
  }
  const unsigned long long t = io.streams ? (unsigned long long)io.streams[s] : (unsigned long long)s;
  uint32_t words[12];
  double w[5];
  noise_draw(io.seed_lo, io.seed_hi, (uint32_t)t, (uint32_t)(t >> 32), io.k + (uint32_t)y, v, S, B, P[Z_TRUNC], w,
             io.raw ? words : nullptr);
  double* o = io.out + s * io.out_s + y * 10 + v * 5;
  if (io.tape) {
#pragma clang fp contract(off)
    const double* tr = io.tape + s * io.tape_s + y * 10 + v * 5;
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = tr[i] + w[i];
  } else {
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = w[i];
  }
  if (io.raw) {
    uint32_t* r = io.raw + s * io.raw_s + y * 24 + v * 12;
#pragma unroll
    for (int q = 0; q < 12; ++q) r[q] = words[q];
  }
}

// ---------------------------------------------------------------------------------------------
// Fleet risk statistics and the worst-case gather of a run record (piadmm_obca_fleet_stats,
// piadmm_obca_stats_trace, piadmm_obca_gather_trace).  Every result is an integer count, a minimum
// of doubles or a comparison, so it is exact and does not depend on the order it is taken in: a
// workgroup reduces its ST scenarios with wave reductions (DPP scans read back through SGPRs, and
// ballots) and LDS partials, writes one partial record, and a second, small launch reduces the
// records.  No atomic, no wait for another workgroup; every output word has one writer.
//
// The ordering key: value ascending, then scenario ascending; a value that is not finite orders
// after every finite one, again by scenario.  Scenarios are distinct, so the order is strict.
// ---------------------------------------------------------------------------------------------
constexpr int SW = 2, ST = 64 * SW;    // a statistics workgroup: ST scenarios, one lane each
constexpr int SB = 64;                 // the most edges
constexpr int WCAND = 512;             // the candidates one merge workgroup of k_stats_worst ranks in LDS
static_assert(ST == 2 * SB, "one lane per (plain / tight, edge)");
static_assert(WCAND / SB >= 2 && ST <= WCAND, "a merge takes at least two lists");

// An idempotent reduction (max, or) of an int over the wave, uniform: the DPP scan of pd::wext, a
// lane without a source keeps its own value.
template <class Op>
__device__ __forceinline__ int wred_i(int v, Op op) {
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x111, 0xf, 0xf, false));
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x112, 0xf, 0xf, false));
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x114, 0xf, 0xf, false));
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x118, 0xf, 0xf, false));
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x142, 0xa, 0xf, false));
  v = op(v, __builtin_amdgcn_update_dpp(v, v, 0x143, 0xc, 0xf, false));
  return __builtin_amdgcn_readlane(v, 63);
}
// The sum of an int over the wave, uniform: the DPP scan of pd::scan_incl (a lane without a source
// adds 0), its last lane read back.  The caller keeps the total inside 31 bits.
__device__ __forceinline__ int wsum_i(int v) {
  v += __builtin_amdgcn_update_dpp(0, v, 0x111, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x112, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x114, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x118, 0xf, 0xf, true);
  v += __builtin_amdgcn_update_dpp(0, v, 0x142, 0xa, 0xf, false);
  v += __builtin_amdgcn_update_dpp(0, v, 0x143, 0xc, 0xf, false);
  return __builtin_amdgcn_readlane(v, 63);
}
// The sum of 0 <= v < 2^63 over the wave (the total below 2^63 too): three limbs of 21 bits, each
// limb's 64 summands inside an int.
__device__ __forceinline__ long long wsum_ll(long long v) {
  const int m21 = (1 << 21) - 1;
  const long long a = wsum_i((int)(v & m21)), b = wsum_i((int)((v >> 21) & m21)), c = wsum_i((int)(v >> 42));
  return a + (b << 21) + (c << 42);
}

__device__ __forceinline__ bool key_less(double va, int sa, double vb, int sb) {
  const bool fa = __builtin_isfinite(va), fb = __builtin_isfinite(vb);
  if (fa != fb) return fa;
  if (fa && va != vb) return va < vb;
  return sa < sb;
}

// The first (x, s) under the ordering key among the lanes with `fin` set (x finite there, the s
// distinct), uniform: the smallest value, then the smallest scenario among the lanes that hold it,
// then that lane's own value (its bits, so -0.0 stays what the scenario has).  +inf and -1 when no
// lane has `fin`.  Every lane of the wave must be here.
__device__ __forceinline__ void wave_minkey(double x, int s, bool fin, double& mv, int& ms) {
  const double inf = __builtin_huge_val();
  const double m = pd::wmin(fin ? x : inf);
  const bool hit = fin && x == m;
  const double sa = pd::wmin(hit ? (double)s : inf);
  const unsigned long long at = __ballot(hit && (double)s == sa);
  mv = inf;
  ms = -1;
  if (at) {
    const int l = __builtin_amdgcn_readfirstlane(__ffsll((long long)at) - 1);
    mv = pd::rdl(x, l);
    ms = __builtin_amdgcn_readlane(s, l);
  }
}

// The partial records: record g holds, for plain (k = 0) and tight (k = 1), the first finite value
// under the key and its scenario (pmin, parg: +inf, -1 for none), the number of finite values (pfin)
// and, per edge b, the number of finite values below it (pbel[(2 g + k) B + b]).
struct stat_parts {
  double* pmin;
  int *parg, *pfin, *pbel;
};
// what k_stats_fleet adds per record: the sum of the iterate sums, the largest iterate, the OR of
// either mask, the flagged scenarios
struct fleet_parts {
  long long* psum;
  int *pmax, *por, *pflag;
};

// One workgroup, one lane per scenario s (`valid`: s < n) with its pair (x0, x1): record g.
__device__ __forceinline__ void stats_chunk(double x0, double x1, bool valid, int s, const double* __restrict__ edges,
                                            int B, size_t g, const stat_parts& P) {
  __shared__ double l_min[SW][2];
  __shared__ int l_arg[SW][2], l_fin[SW][2], l_bel[SW][2][SB];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double x = k ? x1 : x0;
    const bool fin = valid && __builtin_isfinite(x);
    double mv;
    int ms;
    wave_minkey(x, s, fin, mv, ms);
    int below = 0;
    for (int b = 0; b < B; ++b) {
      const int c = __popcll(__ballot(fin && x < edges[b]));
      if (lane == b) below = c;
    }
    const int nf = __popcll(__ballot(fin));
    if (lane == 0) {
      l_min[w][k] = mv;
      l_arg[w][k] = ms;
      l_fin[w][k] = nf;
    }
    l_bel[w][k][lane] = below;
  }
  __syncthreads();
  if (tid < 2) {
    const int k = tid;
    double bv = l_min[0][k];
    int bs = l_arg[0][k], nf = l_fin[0][k];
    for (int v = 1; v < SW; ++v) {
      nf += l_fin[v][k];
      if (l_arg[v][k] >= 0 && (bs < 0 || key_less(l_min[v][k], l_arg[v][k], bv, bs))) {
        bv = l_min[v][k];
        bs = l_arg[v][k];
      }
    }
    P.pmin[2 * g + k] = bv;
    P.parg[2 * g + k] = bs;
    P.pfin[2 * g + k] = nf;
  }
  const int k = tid >> 6, b = tid & 63;
  if (b < B) {
    int t = 0;
    for (int v = 0; v < SW; ++v) t += l_bel[v][k][b];
    P.pbel[(2 * g + k) * (size_t)B + b] = t;
  }
}

// What the G records of row `row` reduce to, left in M (LDS of the caller) for every lane.
struct stat_merged {
  double mn[2];
  int arg[2], fin[2], below[2][SB];
};
__device__ __forceinline__ void stats_merge(size_t row, int G, int B, const stat_parts& P, stat_merged& M) {
  __shared__ double l_min[SW][2];
  __shared__ int l_arg[SW][2], l_fin[SW][2];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    double bv = __builtin_huge_val();
    int bs = -1, nf = 0;
    for (int g = tid; g < G; g += ST) {
      const size_t i = (row * G + g) * 2 + k;
      const double v = P.pmin[i];
      const int s = P.parg[i];
      nf += P.pfin[i];
      if (s >= 0 && (bs < 0 || key_less(v, s, bv, bs))) {
        bv = v;
        bs = s;
      }
    }
    double mv;
    int ms;
    wave_minkey(bv, bs, bs >= 0, mv, ms);
    const int nfw = wsum_i(nf);
    if (lane == 0) {
      l_min[w][k] = mv;
      l_arg[w][k] = ms;
      l_fin[w][k] = nfw;
    }
  }
  {
    const int k = tid >> 6, b = tid & 63;
    int t = 0;
    if (b < B)
      for (int g = 0; g < G; ++g) t += P.pbel[((row * G + g) * 2 + k) * (size_t)B + b];
    M.below[k][b] = t;
  }
  __syncthreads();
  if (tid < 2) {
    const int k = tid;
    double bv = l_min[0][k];
    int bs = l_arg[0][k], nf = l_fin[0][k];
    for (int v = 1; v < SW; ++v) {
      nf += l_fin[v][k];
      if (l_arg[v][k] >= 0 && (bs < 0 || key_less(l_min[v][k], l_arg[v][k], bv, bs))) {
        bv = l_min[v][k];
        bs = l_arg[v][k];
      }
    }
    M.mn[k] = bv;
    M.arg[k] = bs;
    M.fin[k] = nf;
  }
  __syncthreads();
}

// Over the n rows of a summary (n x 4: min plain, its row, min tight, sum of iterates) and the
// R x n iterates and R x n x 2 masks: workgroup g writes record g of P and F.  A lane walks its
// scenario's R rows (the loads of a wave are contiguous in s).
__global__ void __launch_bounds__(ST) k_stats_fleet(int n, int R, const double* __restrict__ summary,
                                                    const int* __restrict__ iters, const int* __restrict__ mask,
                                                    const double* __restrict__ edges, int B, stat_parts P,
                                                    fleet_parts F) {
  __shared__ long long l_sum[SW];
  __shared__ int l_max[SW], l_or[SW][2], l_flag[SW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int s = blockIdx.x * ST + tid;
  const bool valid = s < n;
  double x0 = 0.0, x1 = 0.0;
  long long it = 0;
  int mx = INT_MIN, m0 = 0, m1 = 0;
  if (valid) {
    const double4 q = reinterpret_cast<const double4*>(summary)[s];
    x0 = q.x;
    x1 = q.z;
    it = (long long)q.w;
    for (int r = 0; r < R; ++r) {
      const size_t i = (size_t)r * n + s;
      mx = max(mx, iters[i]);
      const int2 mm = reinterpret_cast<const int2*>(mask)[i];
      m0 |= mm.x;
      m1 |= mm.y;
    }
  }
  const bool flag = valid && ((m0 | m1) & ~(1 << PIADMM_OBCA_CONVERGED)) != 0;
  const long long sum_w = wsum_ll(it);
  const int max_w = wred_i(mx, [](int a, int b) { return max(a, b); });
  const int or0 = wred_i(m0, [](int a, int b) { return a | b; }), or1 = wred_i(m1, [](int a, int b) { return a | b; });
  const int flag_w = __popcll(__ballot(flag));
  if (lane == 0) {
    l_sum[w] = sum_w;
    l_max[w] = max_w;
    l_or[w][0] = or0;
    l_or[w][1] = or1;
    l_flag[w] = flag_w;
  }
  stats_chunk(x0, x1, valid, s, edges, B, blockIdx.x, P);      // its barrier is behind the stores above
  if (tid == 0) {
    long long sm = 0;
    int mxa = INT_MIN, o0 = 0, o1 = 0, fl = 0;
    for (int v = 0; v < SW; ++v) {
      sm += l_sum[v];
      mxa = max(mxa, l_max[v]);
      o0 |= l_or[v][0];
      o1 |= l_or[v][1];
      fl += l_flag[v];
    }
    F.psum[blockIdx.x] = sm;
    F.pmax[blockIdx.x] = mxa;
    F.por[2 * blockIdx.x] = o0;
    F.por[2 * blockIdx.x + 1] = o1;
    F.pflag[blockIdx.x] = fl;
  }
}

// The fleet's results (piadmm_obca_stats_t) and hist[2][B + 1] from the G records: one workgroup.
__global__ void __launch_bounds__(ST) k_stats_fleet_merge(int n, int R, int G, int B, stat_parts P, fleet_parts F,
                                                          piadmm_obca_stats_t* __restrict__ res,
                                                          long long* __restrict__ hist) {
  __shared__ stat_merged M;
  __shared__ long long l_sum[SW];
  __shared__ int l_max[SW], l_or[SW][2], l_flag[SW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  long long sm = 0;
  int mx = INT_MIN, o0 = 0, o1 = 0, fl = 0;
  for (int g = tid; g < G; g += ST) {
    sm += F.psum[g];
    mx = max(mx, F.pmax[g]);
    o0 |= F.por[2 * g];
    o1 |= F.por[2 * g + 1];
    fl += F.pflag[g];
  }
  const long long sum_w = wsum_ll(sm);
  const int max_w = wred_i(mx, [](int a, int b) { return max(a, b); });
  const int or0 = wred_i(o0, [](int a, int b) { return a | b; }), or1 = wred_i(o1, [](int a, int b) { return a | b; });
  const int flag_w = wsum_i(fl);
  if (lane == 0) {
    l_sum[w] = sum_w;
    l_max[w] = max_w;
    l_or[w][0] = or0;
    l_or[w][1] = or1;
    l_flag[w] = flag_w;
  }
  stats_merge(0, G, B, P, M);
  if (tid == 0) {
    long long st = 0;
    int mxa = INT_MIN, a0 = 0, a1 = 0, fa = 0;
    for (int v = 0; v < SW; ++v) {
      st += l_sum[v];
      mxa = max(mxa, l_max[v]);
      a0 |= l_or[v][0];
      a1 |= l_or[v][1];
      fa += l_flag[v];
    }
    for (int k = 0; k < 2; ++k) {
      res->nonfinite[k] = (long long)n - M.fin[k];
      res->fleet_min[k] = M.mn[k];
      res->fleet_arg[k] = M.arg[k];
    }
    res->iter_sum = st;
    res->flagged = fa;
    res->iter_max = R > 0 ? mxa : 0;
    res->mask_or[0] = a0;
    res->mask_or[1] = a1;
    res->reserved = 0;
  }
  // bin 0: below e_0; bin b: below e_b and not below e_(b-1); bin B: finite and not below e_(B-1)
  const int k = tid >> 6, b = tid & 63;
  if (b < B) hist[k * (B + 1) + b] = (long long)(M.below[k][b] - (b ? M.below[k][b - 1] : 0));
  if (b == 0) hist[k * (B + 1) + B] = (long long)(M.fin[k] - M.below[k][B - 1]);
}

// Over the rows x n x 2 clearances: workgroup (row r, chunk c) writes record r * chunks + c.
__global__ void __launch_bounds__(ST) k_stats_rows(int n, const double* __restrict__ clear,
                                                   const double* __restrict__ edges, int B, stat_parts P) {
  const int r = blockIdx.x, c = blockIdx.y;
  const int s = c * ST + (int)threadIdx.x;
  const bool valid = s < n;
  double2 q = make_double2(0.0, 0.0);
  if (valid) q = reinterpret_cast<const double2*>(clear)[(size_t)r * n + s];
  stats_chunk(q.x, q.y, valid, s, edges, B, (size_t)r * gridDim.y + c, P);
}

// row_min, row_arg (rows x 2) and the cumulative row_below (rows x 2 x B): one workgroup per row.
__global__ void __launch_bounds__(ST) k_stats_rows_merge(int G, int B, stat_parts P, double* __restrict__ row_min,
                                                         int* __restrict__ row_arg, int* __restrict__ row_below) {
  __shared__ stat_merged M;
  const int tid = threadIdx.x;
  const size_t row = blockIdx.x;
  stats_merge(row, G, B, P, M);
  if (tid < 2) {
    row_min[2 * row + tid] = M.mn[tid];
    row_arg[2 * row + tid] = M.arg[tid];
  }
  const int k = tid >> 6, b = tid & 63;
  if (b < B) row_below[(2 * row + k) * (size_t)B + b] = M.below[k][b];
}

// The K candidates that come first under the ordering key, in that order, of the `per` candidates
// of this workgroup (per <= WCAND): out list blockIdx.x, the slots past the candidates there are
// holding -1.  Candidate i is (v_in[i * stride], s_in[i]), s_in nullptr: scenario i (the first
// level, over the summary's plain minima, which reads every value once); s < 0: an empty slot of an
// earlier list.  A candidate's place is the number of candidates before it, counted in LDS: the keys
// are distinct, so the places are too.  The host launches the levels until one list is left.
__global__ void __launch_bounds__(ST) k_stats_worst(const double* __restrict__ v_in, int stride,
                                                    const int* __restrict__ s_in, int total, int per, int K,
                                                    double* __restrict__ out_v, int* __restrict__ out_s) {
  __shared__ double lv[WCAND];
  __shared__ int ls[WCAND], l_cnt[SW];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int base = blockIdx.x * per;
  const int C = min(per, total - base);
  int mine = 0;
  for (int i = tid; i < C; i += ST) {
    const int s = s_in ? s_in[base + i] : base + i;
    lv[i] = v_in[(size_t)(base + i) * stride];
    ls[i] = s;
    mine += s >= 0 ? 1 : 0;
  }
  const int cw = wsum_i(mine);
  if (lane == 0) l_cnt[w] = cw;
  __syncthreads();
  int cnt = 0;
  for (int v = 0; v < SW; ++v) cnt += l_cnt[v];
  const size_t o = (size_t)blockIdx.x * K;
  for (int i = tid; i < C; i += ST) {
    const double v = lv[i];
    const int s = ls[i];
    if (s < 0) continue;
    int rank = 0;
    for (int j = 0; j < C; ++j) rank += (ls[j] >= 0 && key_less(lv[j], ls[j], v, s)) ? 1 : 0;
    if (rank < K) {
      out_v[o + rank] = v;
      out_s[o + rank] = s;
    }
  }
  for (int t = tid; t < K; t += ST)
    if (t >= cnt) {
      out_v[o + t] = __builtin_huge_val();
      out_s[o + t] = -1;
    }
}

// One wave per (row r, column k) of the gathered record: every item of scenario slots[k] at row r
// of the attached trace, exact copies (the layout: include/piadmm.h).  Row 0 has no step and
// carries the column's summary instead.
struct gather_src {
  const double *states, *clear, *primal, *dual, *lamb, *summary;
  const int *iters, *mask;
};
struct gather_dst {
  double *states, *clear, *primal, *dual, *summary, *lamb;
  int *iters, *mask;
};
__global__ void __launch_bounds__(64 * PW) k_trace_gather(const int* __restrict__ slots, int m, int n, int rows,
                                                          gather_src a, gather_dst d) {
  const int lane = threadIdx.x & 63;
  const long long wv = (long long)blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (wv >= (long long)rows * m) return;
  const int r = (int)(wv / m), k = (int)(wv % m);
  const size_t s = (size_t)__builtin_amdgcn_readfirstlane(slots[k]);
  const size_t src = (size_t)r * n + s, dst = (size_t)r * m + k;
  if (lane < 10) d.states[dst * 10 + lane] = a.states[src * 10 + lane];
  else if (lane < 12) d.clear[dst * 2 + (lane - 10)] = a.clear[src * 2 + (lane - 10)];
  if (r == 0) {
    if (lane >= 12 && lane < 12 + TSUM) d.summary[(size_t)k * TSUM + (lane - 12)] = a.summary[s * TSUM + (lane - 12)];
    return;
  }
  const size_t sp = (size_t)(r - 1) * n + s, dp = (size_t)(r - 1) * m + k;
  if (lane == 12) d.iters[dp] = a.iters[sp];
  else if (lane == 13 || lane == 14) d.mask[dp * 2 + (lane - 13)] = a.mask[sp * 2 + (lane - 13)];
  else if (lane == 15) d.primal[dp] = a.primal[sp];
  else if (lane == 16) d.dual[dp] = a.dual[sp];
  if (a.lamb) copy_seg(d.lamb + dp * 126, a.lamb + sp * 126, 126, lane);
}

}  // namespace obca_plan

// ---------------------------------------------------------------------------------------------
// C-ABI (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
struct piadmm_obca_plan_s {
  piadmm_obca_plan_cfg_t cfg{};
  bool open = false;
  int n = 0, t_step = 0, i_iter = 0, n_act = 0, n_last = 0, cur = 0;
  // the parameter rows and the references: rows = 1 with stride 0 (piadmm_obca_plan_begin) or
  // rows = n (piadmm_obca_fleet_begin); max_iter_all = the largest max_admm_iter of the rows
  int tab_rows = 0, ref_rows = 0, tab_stride = 0, ref_stride = 0, max_iter_all = 0;
  double sigd = 0.0;
  double *bar = nullptr, *barp = nullptr, *ctrl = nullptr, *ctrlp = nullptr, *X = nullptr, *primal = nullptr,
         *dual = nullptr, *pth = nullptr, *dth = nullptr, *ref = nullptr, *lamb = nullptr, *tab = nullptr;
  int *iters = nullptr, *stop = nullptr, *conv = nullptr, *prob = nullptr, *act[2] = {nullptr, nullptr},
      *keep = nullptr, *count = nullptr, *mask = nullptr;
  int* h_count = nullptr;        // pinned: the 4 bytes read back per iterate
  // the run record (piadmm_obca_trace_begin): rows = MPC steps recorded, row-major over steps.
  // states / clear hold cap + 1 rows (row 0: where the trace was attached), the rest cap.
  struct trace_s {
    bool on = false;
    int cap = 0, rows = 0, flags = 0;
    double *states = nullptr, *clear = nullptr, *primal = nullptr, *dual = nullptr, *lamb = nullptr,
           *summary = nullptr;
    int *iters = nullptr, *mask = nullptr;
  } tr;
  // the PI anti-windup dual law (piadmm_obca_dual_plan): rows = 1 with stride 0 or n gains rows;
  // the integrator S, D and the previous iterate's copy of each, n x 126
  struct dual_s {
    bool on = false;
    int rows = 0, stride = 0;
    double *par = nullptr, *S = nullptr, *D = nullptr, *Sp = nullptr, *Dp = nullptr;
  } du;
  // the longest-first order (piadmm_obca_order_plan): work = (Q, I) per scenario, n x 2; tmp = the
  // unsorted list k_plan_compact / k_plan_shift write and k_plan_order reads, n ints
  struct order_s {
    bool on = false;
    int *work = nullptr, *tmp = nullptr;
  } ord;
  // the per-scenario clocks (piadmm_obca_clock_plan): clk = (c, len, alive) per scenario, n x 3, and
  // `host` its mirror; win = the reference windows, n x 80; flag[cur] = the alive flags (the next
  // tick's `ran`), flag[1 - cur] the ones the next tick writes; list = the n_list scenarios alive
  // when the open step opened, ascending (the active lists are overwritten as the step iterates);
  // ident = 0 .. n - 1, the list k_plan_compact filters by the flags
  struct clock_s {
    bool on = false;
    int cur = 0, n_list = 0;
    int *clk = nullptr, *flag[2] = {nullptr, nullptr}, *list = nullptr, *ident = nullptr;
    double* win = nullptr;
    std::vector<int> host;
  } ck;
  std::vector<int> admm_rows;    // max_admm_iter of every parameter row (max_iter_all is their maximum)
  // the closed-loop feedback (piadmm_obca_feedback_plan): rows = 1 with stride 0 or n plant rows; tape
  // = cap disturbance rows per scenario (nullptr: none), n x cap x 10; steps = the shifts since the
  // attachment (the tape row the next shift adds); next = the states the plant reached, n x 10
  struct feedback_s {
    bool on = false;
    int rows = 0, stride = 0, cap = 0, steps = 0;
    double *par = nullptr, *tape = nullptr, *next = nullptr;
  } fb;
  // the device-side noise on top of the feedback (piadmm_obca_noise_plan): rows = 1 with stride 0 or n
  // noise rows; streams = the stream id of every scenario; wbuf = the disturbance rows of the step
  // that closes, n x 10, which k_plan_noise writes and k_plan_propagate reads; the step index of a
  // shift is k0 + fb.steps
  struct noise_s {
    bool on = false;
    int rows = 0, stride = 0, k0 = 0;
    uint64_t seed = 0;
    double *par = nullptr, *wbuf = nullptr;
    long long* streams = nullptr;
  } nz;
  // the staging buffer of piadmm_obca_tenant_export / _import: the records, then the slot list; grown on demand
  struct stage_s {
    char* buf = nullptr;
    size_t cap = 0;
  } stg;
};

namespace {
using obca_plan::PW;

int pfail(piadmm_obca_t h, int code, const std::string& msg) {
  if (h) h->err = msg;
  return code;
}
#define PHIP(h, call)                                                                  \
  do {                                                                                 \
    hipError_t _e = (call);                                                            \
    if (_e != hipSuccess) return pfail(h, PIADMM_E_HIP, std::string(#call ": ") + hipGetErrorString(_e)); \
  } while (0)

void trace_free(piadmm_obca_plan_s* p) {
  void* d[] = {p->tr.states, p->tr.clear, p->tr.primal, p->tr.dual, p->tr.lamb, p->tr.summary, p->tr.iters,
               p->tr.mask};
  for (void* q : d)
    if (q) (void)hipFree(q);
  p->tr = piadmm_obca_plan_s::trace_s();
}

void dual_free(piadmm_obca_plan_s* p) {
  void* d[] = {p->du.par, p->du.S, p->du.D, p->du.Sp, p->du.Dp};
  for (void* q : d)
    if (q) (void)hipFree(q);
  p->du = piadmm_obca_plan_s::dual_s();
}

void order_free(piadmm_obca_plan_s* p) {
  if (p->ord.work) (void)hipFree(p->ord.work);
  if (p->ord.tmp) (void)hipFree(p->ord.tmp);
  p->ord = piadmm_obca_plan_s::order_s();
}

void clock_free_buffers(piadmm_obca_plan_s::clock_s& c) {
  void* d[] = {c.clk, c.flag[0], c.flag[1], c.list, c.ident, c.win};
  for (void* q : d)
    if (q) (void)hipFree(q);
  c = piadmm_obca_plan_s::clock_s();
}

void clock_free(piadmm_obca_plan_s* p) { clock_free_buffers(p->ck); }

void feedback_free_buffers(piadmm_obca_plan_s::feedback_s& f) {
  void* d[] = {f.par, f.tape, f.next};
  for (void* q : d)
    if (q) (void)hipFree(q);
  f = piadmm_obca_plan_s::feedback_s();
}

void noise_free_buffers(piadmm_obca_plan_s::noise_s& z) {
  void* d[] = {z.par, z.wbuf, z.streams};
  for (void* q : d)
    if (q) (void)hipFree(q);
  z = piadmm_obca_plan_s::noise_s();
}

// the noise counts its steps by the feedback's: it goes whenever the feedback goes or is replaced
void feedback_free(piadmm_obca_plan_s* p) {
  feedback_free_buffers(p->fb);
  noise_free_buffers(p->nz);
}

void stage_free(piadmm_obca_plan_s* p) {
  if (p->stg.buf) (void)hipFree(p->stg.buf);
  p->stg = piadmm_obca_plan_s::stage_s();
}

void plan_free_buffers(piadmm_obca_plan_s* p) {
  trace_free(p);
  dual_free(p);
  order_free(p);
  clock_free(p);
  feedback_free(p);
  stage_free(p);
  void* d[] = {p->bar, p->barp, p->ctrl, p->ctrlp, p->X, p->primal, p->dual, p->pth, p->dth, p->ref, p->lamb,
               p->tab, p->iters, p->stop, p->conv, p->prob, p->act[0], p->act[1], p->keep, p->count, p->mask};
  for (void* q : d)
    if (q) (void)hipFree(q);
  if (p->h_count) (void)hipHostFree(p->h_count);
  p->bar = p->barp = p->ctrl = p->ctrlp = p->X = p->primal = p->dual = p->pth = p->dth = p->ref = p->lamb = nullptr;
  p->tab = nullptr;
  p->iters = p->stop = p->conv = p->prob = p->act[0] = p->act[1] = p->keep = p->count = p->mask = nullptr;
  p->h_count = nullptr;
  p->open = false;
}

// the parameter row of a configuration (the row a plan without a table runs every scenario on)
void row_of_cfg(const piadmm_obca_plan_cfg_t& c, double* row) {
  using namespace obca_plan;
  for (int i = 0; i < TAB; ++i) row[i] = 0.0;
  row[T_RHO] = c.rho;  row[T_MIN_DIS] = c.min_dis;  row[T_CONV] = c.conv_thres;
  row[T_MAX_X] = c.max_x;  row[T_MAX_Y] = c.max_y;  row[T_R] = c.r;  row[T_Q] = c.q;
  row[T_XB] = c.x_bound;  row[T_MU] = c.mu_max;  row[T_G] = c.g_max;
  row[T_ADMM] = (double)c.max_admm_iter;  row[T_SQP] = (double)c.max_sqp_iter;
  row[T_ROUND] = (double)c.round_decimals;  row[T_START] = (double)c.start;
}

// One parameter row: the ranges check_recs (csrc/piadmm_obca.hip) and edge_check
// (csrc/piadmm_obca_edge.hip) enforce per record, on the row those records are packed from, and the
// integers integral.  nullptr when the row is good, else what is wrong with it.
const char* row_check(const double* row) {
  using namespace obca_plan;
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

// One gains row of the dual law: nullptr when it is good, else what is wrong with it.
const char* dual_row_check(const double* row) {
  using namespace obca_plan;
  for (int i = 0; i < DPAR; ++i)
    if (!std::isfinite(row[i])) return "every entry finite";
  if (row[G_WINDUP] != 0.0 && row[G_WINDUP] != 1.0) return "windup 0 or 1";
  if (row[G_WINDUP] == 1.0 && !(row[G_SAT] > 0.0)) return "windup_sat > 0 with windup set";
  for (int i = G_WINDUP + 1; i < DPAR; ++i)
    if (row[i] != 0.0) return "the trailing entries must be 0";
  return nullptr;
}

int dual_rows_check(piadmm_obca_t h, const double* gains, int rows, int n, const std::string& who) {
  if (rows != 1 && rows != n) return pfail(h, PIADMM_E_ARG, who + ": rows must be 1 or n (" + std::to_string(n) + ")");
  for (int k = 0; k < rows; ++k)
    if (const char* why = dual_row_check(gains + (size_t)k * obca_plan::DPAR))
      return pfail(h, PIADMM_E_ARG, who + ": row " + std::to_string(k) + ": " + why);
  return 0;
}

// One plant row of the feedback (both vehicles): nullptr when it is good, else what is wrong with it.
const char* feedback_row_check(const double* row) {
  using namespace obca_plan;
  for (int i = 0; i < FPAR; ++i)
    if (!std::isfinite(row[i])) return "every entry finite";
  for (int v = 0; v < 2; ++v) {
    const double* P = row + v * FV;
    if (P[F_METHOD] != 0.0 && P[F_METHOD] != 1.0) return "method 0 (Euler) or 1 (RK4)";
    if (!(P[F_NSUB] >= 1.0 && P[F_NSUB] <= (double)F_NSUB_MAX && P[F_NSUB] == std::floor(P[F_NSUB])))
      return "1 <= n_sub <= 64, an integer";
    if (!(P[F_LR] > 0.0) || !(P[F_LF] > 0.0)) return "lr, lf > 0";
    if (!(P[F_AMAX] > 0.0) || !(P[F_WMAX] > 0.0)) return "a_max, w_max > 0";
  }
  return nullptr;
}

// the nominal plant: the NLP's own transition
void feedback_row_nominal(double* row) {
  using namespace obca_plan;
  for (int v = 0; v < 2; ++v) {
    double* P = row + v * FV;
    P[F_METHOD] = 0.0;  P[F_NSUB] = 1.0;  P[F_LR] = 1.0;  P[F_LF] = 1.5;
    P[F_GA] = 1.0;  P[F_GW] = 1.0;  P[F_AMAX] = 5.0;  P[F_WMAX] = 20.0;
  }
}

// the first entry of a[0 .. count) that is not finite, or -1
int64_t first_not_finite(const double* a, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(a[i])) return (int64_t)i;
  return -1;
}

// what every scenario of a plan shares, and prob
int shared_check(piadmm_obca_t h, const piadmm_obca_plan_cfg_t& c, const int32_t* prob, const std::string& who) {
  if (c.update_lamb_ij != 0 && c.update_lamb_ij != 1) return pfail(h, PIADMM_E_ARG, who + ": update_lamb_ij 0 or 1");
  if (c.n_scenarios < 1) return pfail(h, PIADMM_E_ARG, who + ": n_scenarios >= 1");
  if (c.n_scenarios > (1 << 20)) return pfail(h, PIADMM_E_ARG, who + ": n_scenarios <= 2^20");
  if (c.t_step0 < 0 || c.n_ref < 8 || c.t_step0 > c.n_ref - 8)
    return pfail(h, PIADMM_E_ARG, who + ": t_step0 >= 0 and t_step0 + 8 <= n_ref");
  if (c.n_ref > (1 << 20)) return pfail(h, PIADMM_E_ARG, who + ": n_ref <= 2^20");
  for (int k = 0; k < c.n_scenarios; ++k)
    if (prob[k] != 0 && prob[k] != 1)
      return pfail(h, PIADMM_E_ARG, who + ": prob[" + std::to_string(k) + "] must be 0 or 1");
  return 0;
}

template <typename T>
int dalloc(piadmm_obca_t h, T** p, size_t count, bool zero) {
  PHIP(h, hipMalloc(p, count * sizeof(T)));
  if (zero) PHIP(h, hipMemset(*p, 0, count * sizeof(T)));
  return 0;
}

int open_plan(piadmm_obca_t h, piadmm_obca_plan_s** out, const char* who) {
  if (!h) return PIADMM_E_ARG;
  if (!h->plan || !h->plan->open) return pfail(h, PIADMM_E_STATE, std::string(who) + ": no open plan (obca_plan_begin)");
  *out = h->plan;
  return 0;
}

int blocks_for(int waves) { return (waves + PW - 1) / PW; }
// workgroups of 64 * PW lanes for a kernel that runs one lane per item
int lane_blocks(int lanes) { return (lanes + 64 * PW - 1) / (64 * PW); }
// true when the attached feedback has a tape and the next `steps` shifts do not fit what is left of it
bool feedback_exhausted(const piadmm_obca_plan_s* p, int64_t steps) {
  return p->fb.on && p->fb.tape && (int64_t)p->fb.steps + steps > p->fb.cap;
}
// true when the attached noise would pass step index 2^31 - 1 within the next `steps` shifts
bool noise_exhausted(const piadmm_obca_plan_s* p, int64_t steps) {
  return p->nz.on && (int64_t)p->nz.k0 + p->fb.steps + steps > ((int64_t)1 << 31);
}
}  // namespace

void piadmm_obca_plan_release(piadmm_obca_t h) {
  if (!h->plan) return;
  if (h->plan->tr.on || h->plan->du.on || h->plan->ord.on || h->plan->ck.on || h->plan->fb.on) {
    (void)hipSetDevice(h->device);
    if (h->stream) (void)hipStreamSynchronize(h->stream);
    trace_free(h->plan);
    dual_free(h->plan);
    order_free(h->plan);
    clock_free(h->plan);
    feedback_free(h->plan);
  }
  h->plan->open = false;
}

void piadmm_obca_plan_free(piadmm_obca_t h) {
  if (!h->plan) return;
  plan_free_buffers(h->plan);
  delete h->plan;
  h->plan = nullptr;
}

namespace {
// Opens the plan both entry points share: `tab` holds tab_rows parameter rows (1: every scenario
// reads row 0, stride 0; n: one each), ref_traj ref_rows references of 2 x n_ref x 5 likewise.
// Everything was checked before; this is the first device call.
int plan_open(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob, const double* primal_thres,
              const double* dual_thres, const double* ref_traj, int ref_rows, const std::vector<double>& tab,
              int tab_rows, const double* state) {
  using namespace obca_plan;
  const int n = cfg->n_scenarios;
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  if (!h->plan) h->plan = new piadmm_obca_plan_s();
  piadmm_obca_plan_s* p = h->plan;
  plan_free_buffers(p);
  // the takeover: the resident local batch and its longest-first history end here
  h->n = 0;
  h->cost_n = 0;
  h->plan_taken = true;
  if (int rc = piadmm_obca_local_ensure(h, 2 * n)) return rc;
  if (int rc = piadmm_obca_edge_ensure(h, n)) return rc;
  std::vector<int> ident((size_t)2 * n);
  for (int i = 0; i < 2 * n; ++i) ident[i] = i;
  PHIP(h, hipMemcpy(h->d_order, ident.data(), (size_t)2 * n * sizeof(int), hipMemcpyHostToDevice));

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
  if ((rc = dalloc(h, &p->bar, N * STATE, false)) || (rc = dalloc(h, &p->barp, N * STATE, false)) ||
      (rc = dalloc(h, &p->ctrl, N * NCTRL, true)) || (rc = dalloc(h, &p->ctrlp, N * NCTRL, true)) ||
      (rc = dalloc(h, &p->X, N * NX, true)) || (rc = dalloc(h, &p->primal, N, true)) ||
      (rc = dalloc(h, &p->dual, N, true)) || (rc = dalloc(h, &p->pth, N, false)) ||
      (rc = dalloc(h, &p->dth, N, false)) || (rc = dalloc(h, &p->ref, ref_one * ref_rows, false)) ||
      (rc = dalloc(h, &p->tab, (size_t)tab_rows * TAB, false)) ||
      (rc = dalloc(h, &p->lamb, N * 126, true)) || (rc = dalloc(h, &p->iters, N, true)) ||
      (rc = dalloc(h, &p->stop, N, true)) || (rc = dalloc(h, &p->conv, N, true)) ||
      (rc = dalloc(h, &p->prob, N, false)) || (rc = dalloc(h, &p->act[0], N, false)) ||
      (rc = dalloc(h, &p->act[1], N, true)) || (rc = dalloc(h, &p->keep, N, true)) ||
      (rc = dalloc(h, &p->count, (size_t)1, true)) || (rc = dalloc(h, &p->mask, 2 * N, true))) {
    plan_free_buffers(p);
    return rc;
  }
  PHIP(h, hipHostMalloc(reinterpret_cast<void**>(&p->h_count), sizeof(int)));
  PHIP(h, hipMemcpy(p->bar, state, N * STATE * sizeof(double), hipMemcpyHostToDevice));
  PHIP(h, hipMemcpy(p->barp, state, N * STATE * sizeof(double), hipMemcpyHostToDevice));
  PHIP(h, hipMemcpy(p->pth, primal_thres, N * sizeof(double), hipMemcpyHostToDevice));
  PHIP(h, hipMemcpy(p->dth, dual_thres, N * sizeof(double), hipMemcpyHostToDevice));
  PHIP(h, hipMemcpy(p->ref, ref_traj, ref_one * ref_rows * sizeof(double), hipMemcpyHostToDevice));
  PHIP(h, hipMemcpy(p->tab, tab.data(), (size_t)tab_rows * TAB * sizeof(double), hipMemcpyHostToDevice));
  PHIP(h, hipMemcpy(p->prob, prob, N * sizeof(int), hipMemcpyHostToDevice));
  PHIP(h, hipMemcpy(p->act[0], ident.data(), N * sizeof(int), hipMemcpyHostToDevice));
  p->t_step = cfg->t_step0;
  p->i_iter = 0;
  p->n_act = n;
  p->n_last = 0;
  p->cur = 0;
  p->open = true;
  return 0;
}

// Enqueues row `row` of the attached trace (0: the state it is attached at; rows + 1: the step
// k_plan_shift has just closed, on the same stream): the copies, then the clearances of the row's
// own states.  No synchronisation.
int trace_append(piadmm_obca_t h, piadmm_obca_plan_s* p, int row) {
  using namespace obca_plan;
  auto& t = p->tr;
  const size_t N = (size_t)p->n;
  hipLaunchKernelGGL(k_plan_trace, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->n, row, p->bar, p->iters,
                     p->mask, p->primal, p->dual, p->lamb, t.states, t.iters, t.mask, t.primal, t.dual, t.lamb,
                     t.summary);
  PHIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_plan_clearance, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->n,
                     t.states + (size_t)row * N * 10, 10, p->prob, p->sigd, row, t.clear + (size_t)row * N * 2,
                     t.summary);
  PHIP(h, hipGetLastError());
  return 0;
}

// One clock row (c0, len) against the plan's n_ref: nullptr when it is good, else what is wrong.
const char* clock_row_check(int c0, int len, int n_ref) {
  if (c0 < 0) return "c0 >= 0";
  if (len < 8 || len > n_ref) return "8 <= len <= n_ref";
  if (c0 > len - 8) return "c0 + 8 <= len";
  return nullptr;
}

// Enqueues what follows a change of the clocks: the tick of the scenarios flagged in `ran` (nullptr:
// nobody, the record is only rebuilt), the alive flags into flag[dst], the windows of the alive
// scenarios, their ascending list into ck.list and the list the next iterate reads (sorted, with
// the order on).  n_alive is the mirror's count of the flags the tick writes.  No synchronisation.
int clock_lists(piadmm_obca_t h, piadmm_obca_plan_s* p, const int* ran, int dst, int n_alive) {
  using namespace obca_plan;
  auto& c = p->ck;
  hipLaunchKernelGGL(k_plan_clock, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->n, c.clk, ran, p->ref,
                     p->ref_stride, p->cfg.n_ref, c.win, c.flag[dst]);
  PHIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_plan_compact, dim3(1), dim3(CT), 0, h->stream, c.ident, c.flag[dst], p->n, c.list, p->count);
  PHIP(h, hipGetLastError());
  if (n_alive <= 0) return 0;
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(n_alive)), dim3(64 * PW), 0, h->stream, c.list,
                       (const int*)nullptr, n_alive, p->ord.work, p->act[p->cur]);
    PHIP(h, hipGetLastError());
  } else {
    PHIP(h, hipMemcpyAsync(p->act[p->cur], c.list, (size_t)n_alive * sizeof(int), hipMemcpyDeviceToDevice, h->stream));
  }
  return 0;
}

// piadmm_obca_plan_shift of a clocked plan: the step closes for the scenarios it ran (ck.list), their
// clocks tick, and the next step's list is the scenarios still alive.
int clock_shift(piadmm_obca_t h, piadmm_obca_plan_s* p) {
  using namespace obca_plan;
  auto& c = p->ck;
  const int m = c.n_list;
  hipLaunchKernelGGL(k_plan_shift_list, dim3(m), dim3(64), 0, h->stream, c.list, m, p->bar, p->barp, p->X, p->lamb,
                     p->ctrlp);
  PHIP(h, hipGetLastError());
  if (p->du.on) {
    hipLaunchKernelGGL(k_plan_dual_shift_list, dim3(m), dim3(64), 0, h->stream, c.list, m, p->du.S, p->du.D, p->du.Sp,
                       p->du.Dp);
    PHIP(h, hipGetLastError());
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
  if (p->tr.on) {
    if (int rc = trace_append(h, p, p->tr.rows + 1)) return rc;
  }
  PHIP(h, hipStreamSynchronize(h->stream));
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

int open_trace(piadmm_obca_t h, piadmm_obca_plan_s** out, const char* who) {
  if (int rc = open_plan(h, out, who)) return rc;
  if (!(*out)->tr.on) return pfail(h, PIADMM_E_STATE, std::string(who) + ": no trace attached (obca_trace_begin)");
  return 0;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_plan_cfg_size(void) { return (int32_t)sizeof(piadmm_obca_plan_cfg_t); }

int32_t piadmm_obca_plan_begin(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob,
                               const double* primal_thres, const double* dual_thres, const double* ref_traj,
                               const double* state) {
  if (!h) return PIADMM_E_ARG;
  if (!cfg || !prob || !primal_thres || !dual_thres || !ref_traj || !state)
    return pfail(h, PIADMM_E_ARG, "obca_plan_begin: null argument");
  std::vector<double> row(obca_plan::TAB);
  row_of_cfg(*cfg, row.data());
  if (const char* why = row_check(row.data())) return pfail(h, PIADMM_E_ARG, std::string("obca_plan_begin: ") + why);
  if (int rc = shared_check(h, *cfg, prob, "obca_plan_begin")) return rc;
  return plan_open(h, cfg, prob, primal_thres, dual_thres, ref_traj, 1, row, 1, state);
}

int32_t piadmm_obca_fleet_begin(piadmm_obca_t h, const piadmm_obca_plan_cfg_t* cfg, const int32_t* prob,
                                const double* primal_thres, const double* dual_thres, const double* ref_traj,
                                const double* par, const double* state) {
  using obca_plan::TAB;
  if (!h) return PIADMM_E_ARG;
  if (!cfg || !prob || !primal_thres || !dual_thres || !ref_traj || !state)
    return pfail(h, PIADMM_E_ARG, "obca_fleet_begin: null argument");
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
      return pfail(h, PIADMM_E_ARG, "obca_fleet_begin: row " + std::to_string(k) + ": " + why);
  }
  return plan_open(h, cfg, prob, primal_thres, dual_thres, ref_traj, n, tab, n, state);
}

int32_t piadmm_obca_plan_iterate(piadmm_obca_t h, int32_t* n_active_after) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_iterate")) return rc;
  if (p->ck.on && p->ck.n_list == 0) return pfail(h, PIADMM_E_STATE, "obca_plan_iterate: no scenario alive");
  if (p->n_act <= 0) return pfail(h, PIADMM_E_STATE, "obca_plan_iterate: no active scenario (obca_plan_shift closes the step)");
  if (!p->ck.on && p->t_step + 8 > p->cfg.n_ref) return pfail(h, PIADMM_E_STATE, "obca_plan_iterate: reference exhausted");
  PHIP(h, hipSetDevice(h->device));
  const int m = p->n_act;
  if (2 * m > h->cap || m > h->e_cap) return pfail(h, PIADMM_E_STATE, "obca_plan_iterate: the handle's buffers shrank");
  hipStream_t st = h->stream;
  const int* act = p->act[p->cur];
  int* nxt = p->act[1 - p->cur];
  if (p->i_iter == 0) {
    // a new MPC step: the stop iterates and the status bits are the step's own
    PHIP(h, hipMemsetAsync(p->iters, 0, (size_t)p->n * sizeof(int), st));
    PHIP(h, hipMemsetAsync(p->mask, 0, (size_t)2 * p->n * sizeof(int), st));
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
  PHIP(h, hipGetLastError());
  if (int rc = piadmm_obca_local_launch(h, 2 * m)) return rc;
  // the edge output starts from zeros, as in piadmm_obca_edge_solve
  PHIP(h, hipMemsetAsync(h->e_out, 0, (size_t)m * EOUT * sizeof(double), st));
  hipLaunchKernelGGL(k_plan_exchange, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, p->bar, p->prob, h->d_out,
                     p->tab, p->tab_stride, p->sigd, p->cfg.update_lamb_ij, p->ctrl, p->X, p->conv, h->e_rec);
  PHIP(h, hipGetLastError());
  if (int rc = piadmm_obca_edge_launch(h, m)) return rc;
  if (p->du.on) {
    // the law's lamb_bar_new and dres partials replace the fused update's in the edge output
    hipLaunchKernelGGL(k_plan_dual_pi, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, h->e_rec, h->e_out, h->e_ist,
                       p->du.par, p->du.stride, p->du.S, p->du.D, p->du.Sp, p->du.Dp);
    PHIP(h, hipGetLastError());
  }
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_work, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, h->d_ist, h->e_ist, p->ord.work);
    PHIP(h, hipGetLastError());
  }
  hipLaunchKernelGGL(k_plan_residual, dim3(blocks_for(m)), dim3(64 * PW), 0, st, act, m, i_iter, p->bar, p->barp,
                     p->ctrl, p->ctrlp, h->e_out, h->d_ist, h->e_ist, p->pth, p->dth, p->tab, p->tab_stride, p->primal,
                     p->dual,
                     p->stop, p->iters, p->mask, p->keep);
  PHIP(h, hipGetLastError());
  // with the order on, the kept entries go to the scratch list and are sorted into the next list
  hipLaunchKernelGGL(k_plan_compact, dim3(1), dim3(CT), 0, st, act, p->keep, m, p->ord.on ? p->ord.tmp : nxt, p->count);
  PHIP(h, hipGetLastError());
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(m)), dim3(64 * PW), 0, st, p->ord.tmp, p->count, m, p->ord.work,
                       nxt);
    PHIP(h, hipGetLastError());
  }
  PHIP(h, hipMemcpyAsync(p->h_count, p->count, sizeof(int), hipMemcpyDeviceToHost, st));
  PHIP(h, hipStreamSynchronize(st));
  const int left = *p->h_count;
  if (left < 0 || left > m) return pfail(h, PIADMM_E_STATE, "obca_plan_iterate: active count out of range");
  p->i_iter = i_iter;
  p->n_last = m;
  p->n_act = left;
  p->cur = 1 - p->cur;
  if (n_active_after) *n_active_after = left;
  return 0;
}

int32_t piadmm_obca_plan_shift(piadmm_obca_t h) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_shift")) return rc;
  if (p->n_act > 0) return pfail(h, PIADMM_E_STATE, "obca_plan_shift: scenarios are still active");
  if (p->i_iter == 0) return pfail(h, PIADMM_E_STATE, "obca_plan_shift: no iterate ran in this step");
  if (p->tr.on && p->tr.rows >= p->tr.cap) return pfail(h, PIADMM_E_STATE, "obca_plan_shift: trace full");
  if (feedback_exhausted(p, 1)) return pfail(h, PIADMM_E_STATE, "obca_plan_shift: disturbance tape exhausted");
  if (noise_exhausted(p, 1)) return pfail(h, PIADMM_E_STATE, "obca_plan_shift: noise step index exhausted");
  PHIP(h, hipSetDevice(h->device));
  if (p->ck.on) return clock_shift(h, p);
  if (p->fb.on) {
    // the plant step first: it reads the closing step's init_state and the stopping solution's first
    // control (k_plan_exchange wrote ctrl and X from the same local output), which the shift overwrites
    plant_io io{};
    io.x0 = p->bar + S_INIT;  io.x0_s = STATE;
    io.ctrl = p->ctrl;  io.ctrl_s = NCTRL;  io.ctrl_v = NCTRL / 2;  io.ctrl_w = NT;
    io.par = p->fb.par;  io.par_s = p->fb.stride;
    io.w = p->fb.tape ? p->fb.tape + (size_t)p->fb.steps * 10 : nullptr;  io.w_s = (long long)p->fb.cap * 10;
    io.out = p->fb.next;
    if (p->nz.on) {
      // the step's disturbance rows first (the tape's row added in front), then read in the tape's place
      noise_io zo{};
      zo.par = p->nz.par;  zo.par_s = p->nz.stride;
      zo.streams = p->nz.streams;
      zo.tape = io.w;  zo.tape_s = io.w_s;
      zo.out = p->nz.wbuf;  zo.out_s = 10;
      zo.seed_lo = (uint32_t)p->nz.seed;  zo.seed_hi = (uint32_t)(p->nz.seed >> 32);
      zo.k = (uint32_t)p->nz.k0 + (uint32_t)p->fb.steps;
      hipLaunchKernelGGL(k_plan_noise, dim3(lane_blocks(2 * p->n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr,
                         p->n, zo);
      PHIP(h, hipGetLastError());
      io.w = p->nz.wbuf;  io.w_s = 10;
    }
    hipLaunchKernelGGL(k_plan_propagate, dim3(lane_blocks(2 * p->n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr,
                       p->n, io);
    PHIP(h, hipGetLastError());
  }
  // every scenario is active again: the list the next iterate reads is the identity, or with the
  // order on the identity sorted by the work of the step that closes
  hipLaunchKernelGGL(k_plan_shift, dim3(p->n), dim3(64), 0, h->stream, p->n, p->bar, p->barp, p->X, p->lamb, p->ctrlp,
                     p->ord.on ? p->ord.tmp : p->act[p->cur]);
  PHIP(h, hipGetLastError());
  if (p->ord.on) {
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->ord.tmp,
                       (const int*)nullptr, p->n, p->ord.work, p->act[p->cur]);
    PHIP(h, hipGetLastError());
  }
  if (p->du.on) {
    hipLaunchKernelGGL(k_plan_dual_shift, dim3(p->n), dim3(64), 0, h->stream, p->n, p->du.S, p->du.D, p->du.Sp,
                       p->du.Dp);
    PHIP(h, hipGetLastError());
  }
  if (p->fb.on) {
    // the state the vehicle reached over init_state of both copies, before the trace reads it
    hipLaunchKernelGGL(k_plan_set_init, dim3(lane_blocks(2 * p->n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr,
                       p->n, p->fb.next, p->bar, p->barp);
    PHIP(h, hipGetLastError());
  }
  if (p->tr.on) {
    if (int rc = trace_append(h, p, p->tr.rows + 1)) return rc;
  }
  PHIP(h, hipStreamSynchronize(h->stream));
  if (p->tr.on) p->tr.rows += 1;
  if (p->fb.on) p->fb.steps += 1;
  p->t_step += 1;
  p->i_iter = 0;
  p->n_act = p->n;
  p->n_last = 0;
  return 0;
}

int32_t piadmm_obca_plan_step(piadmm_obca_t h, int32_t* iters_out) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_step")) return rc;
  if (p->ck.on && p->ck.n_list == 0) return pfail(h, PIADMM_E_STATE, "obca_plan_step: no scenario alive");
  if (!p->ck.on && p->t_step + 8 > p->cfg.n_ref) return pfail(h, PIADMM_E_STATE, "obca_plan_step: reference exhausted");
  if (p->tr.on && p->tr.rows >= p->tr.cap) return pfail(h, PIADMM_E_STATE, "obca_plan_step: trace full");
  if (feedback_exhausted(p, 1)) return pfail(h, PIADMM_E_STATE, "obca_plan_step: disturbance tape exhausted");
  if (noise_exhausted(p, 1)) return pfail(h, PIADMM_E_STATE, "obca_plan_step: noise step index exhausted");
  // i_iter > max_admm_iter stops a scenario: at most the largest max_admm_iter + 1 iterates in a step
  while (p->n_act > 0 && p->i_iter <= p->max_iter_all) {
    if (int rc = piadmm_obca_plan_iterate(h, nullptr)) return rc;
  }
  if (p->n_act > 0) return pfail(h, PIADMM_E_STATE, "obca_plan_step: scenarios active after max_admm_iter + 1 iterates");
  if (iters_out) {
    PHIP(h, hipMemcpyAsync(iters_out, p->iters, (size_t)p->n * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
  }
  return piadmm_obca_plan_shift(h);
}

int32_t piadmm_obca_plan_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_plan_get")) return rc;
  const int64_t n = p->n, m = p->n_last, D = sizeof(double), I = sizeof(int32_t);
  const void* src = nullptr;
  int64_t want = -1;
  int32_t counts[3] = {p->n_last, p->n_act, p->i_iter};
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
      if (!p->du.on) return pfail(h, PIADMM_E_STATE, "obca_plan_get: no dual law attached (obca_dual_plan)");
      if (what == PIADMM_OBCA_PLAN_GET_DUAL_PAR) { src = p->du.par; want = (int64_t)p->du.rows * DPAR * D; }
      else { src = what == PIADMM_OBCA_PLAN_GET_DUAL_S ? p->du.S : p->du.D; want = n * 126 * D; }
      break;
    case PIADMM_OBCA_PLAN_GET_DUAL_S_PREV:
    case PIADMM_OBCA_PLAN_GET_DUAL_D_PREV:
      if (!p->du.on) return pfail(h, PIADMM_E_STATE, "obca_plan_get: no dual law attached (obca_dual_plan)");
      src = what == PIADMM_OBCA_PLAN_GET_DUAL_S_PREV ? p->du.Sp : p->du.Dp; want = n * 126 * D; break;
    case PIADMM_OBCA_PLAN_GET_PRIMAL_THRES: src = p->pth; want = n * D; break;
    case PIADMM_OBCA_PLAN_GET_DUAL_THRES: src = p->dth; want = n * D; break;
    case PIADMM_OBCA_PLAN_GET_PROB: src = p->prob; want = n * I; break;
    case PIADMM_OBCA_PLAN_GET_WORK:
      if (!p->ord.on) return pfail(h, PIADMM_E_STATE, "obca_plan_get: no order attached (obca_order_plan)");
      src = p->ord.work; want = n * 2 * I; break;
    case PIADMM_OBCA_PLAN_GET_CLOCK:
    case PIADMM_OBCA_PLAN_GET_WINDOW:
      if (!p->ck.on) return pfail(h, PIADMM_E_STATE, "obca_plan_get: no clock attached (obca_clock_plan)");
      if (what == PIADMM_OBCA_PLAN_GET_CLOCK) { src = p->ck.clk; want = n * 3 * I; }
      else { src = p->ck.win; want = n * WIN * D; }
      break;
    case PIADMM_OBCA_PLAN_GET_FEEDBACK_PAR:
    case PIADMM_OBCA_PLAN_GET_FEEDBACK_STEPS:
      if (!p->fb.on) return pfail(h, PIADMM_E_STATE, "obca_plan_get: no feedback attached (obca_feedback_plan)");
      if (what == PIADMM_OBCA_PLAN_GET_FEEDBACK_PAR) { src = p->fb.par; want = (int64_t)p->fb.rows * FPAR * D; }
      else want = I;
      break;
    case PIADMM_OBCA_NOISE_GET_PAR:
    case PIADMM_OBCA_NOISE_GET_STREAMS:
    case PIADMM_OBCA_NOISE_GET_SEED:
      if (!p->nz.on) return pfail(h, PIADMM_E_STATE, "obca_plan_get: no noise attached (obca_noise_plan)");
      if (what == PIADMM_OBCA_NOISE_GET_PAR) { src = p->nz.par; want = (int64_t)p->nz.rows * ZPAR * D; }
      else if (what == PIADMM_OBCA_NOISE_GET_STREAMS) { src = p->nz.streams; want = n * (int64_t)sizeof(int64_t); }
      else want = 2 * (int64_t)sizeof(uint64_t);
      break;
    case PIADMM_OBCA_PLAN_GET_T_STEP: want = I; break;
    case PIADMM_OBCA_PLAN_GET_COUNTS: want = 3 * I; break;
    default: return pfail(h, PIADMM_E_ARG, "obca_plan_get: unknown item " + std::to_string(what));
  }
  if (bytes != want)
    return pfail(h, PIADMM_E_ARG, "obca_plan_get: item " + std::to_string(what) + " is " + std::to_string(want) +
                 " bytes, not " + std::to_string(bytes));
  if (want == 0) return 0;
  if (!out) return pfail(h, PIADMM_E_ARG, "obca_plan_get: out");
  if (what == PIADMM_OBCA_PLAN_GET_T_STEP) { *static_cast<int32_t*>(out) = p->t_step; return 0; }
  if (what == PIADMM_OBCA_PLAN_GET_FEEDBACK_STEPS) { *static_cast<int32_t*>(out) = p->fb.steps; return 0; }
  if (what == PIADMM_OBCA_NOISE_GET_SEED) {
    static_cast<uint64_t*>(out)[0] = p->nz.seed;
    static_cast<uint64_t*>(out)[1] = (uint64_t)p->nz.k0;
    return 0;
  }
  if (what == PIADMM_OBCA_PLAN_GET_COUNTS) { for (int i = 0; i < 3; ++i) static_cast<int32_t*>(out)[i] = counts[i]; return 0; }
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipMemcpyAsync(out, src, (size_t)want, hipMemcpyDeviceToHost, h->stream));
  PHIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_plan_end(piadmm_obca_t h) {
  if (!h) return PIADMM_E_ARG;
  if (!h->plan) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  piadmm_obca_plan_free(h);
  return 0;
}

int32_t piadmm_obca_clearance(piadmm_obca_t h, int32_t n, const double* states, const int32_t* prob, double* out) {
  using namespace obca_plan;
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_clearance: 1 <= n <= 2^20");
  if (!states || !prob || !out) return pfail(h, PIADMM_E_ARG, "obca_clearance: null argument");
  for (int k = 0; k < n; ++k) {
    if (prob[k] != 0 && prob[k] != 1)
      return pfail(h, PIADMM_E_ARG, "obca_clearance: prob[" + std::to_string(k) + "] must be 0 or 1");
    for (int i = 0; i < 10; ++i)
      if (!std::isfinite(states[(size_t)k * 10 + i]))
        return pfail(h, PIADMM_E_ARG, "obca_clearance: state pair " + std::to_string(k) + " is not finite");
  }
  PHIP(h, hipSetDevice(h->device));
  // the call's own buffers: neither the handle's local and edge buffers nor an open plan is touched
  double *d_st = nullptr, *d_out = nullptr;
  int* d_pr = nullptr;
  const size_t N = (size_t)n;
  auto run = [&]() -> int {
    if (int rc = dalloc(h, &d_st, N * 10, false)) return rc;
    if (int rc = dalloc(h, &d_pr, N, false)) return rc;
    if (int rc = dalloc(h, &d_out, N * 2, true)) return rc;
    PHIP(h, hipMemcpyAsync(d_st, states, N * 10 * sizeof(double), hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_pr, prob, N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_plan_clearance, dim3(blocks_for(n)), dim3(64 * PW), 0, h->stream, n, d_st, 10, d_pr,
                       std::sqrt(0.95 / (1.0 - 0.95)), 0, d_out, (double*)nullptr);
    PHIP(h, hipGetLastError());
    PHIP(h, hipMemcpyAsync(out, d_out, N * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  if (d_st) (void)hipFree(d_st);
  if (d_pr) (void)hipFree(d_pr);
  if (d_out) (void)hipFree(d_out);
  return rc;
}

int32_t piadmm_obca_dual_plan(piadmm_obca_t h, const double* gains, int32_t rows) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_dual_plan")) return rc;
  const bool detach = !gains || rows == 0;
  if (!detach)
    if (int rc = dual_rows_check(h, gains, rows, p->n, "obca_dual_plan")) return rc;
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_dual_plan: only at a step boundary (an MPC step is open)");
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  dual_free(p);
  if (detach) return 0;
  auto& d = p->du;
  const size_t N = (size_t)p->n, L = 126 * sizeof(double);
  int rc = 0;
  if ((rc = dalloc(h, &d.par, (size_t)rows * DPAR, false)) || (rc = dalloc(h, &d.S, N * 126, false)) ||
      (rc = dalloc(h, &d.Sp, N * 126, false)) || (rc = dalloc(h, &d.D, N * 126, true)) ||
      (rc = dalloc(h, &d.Dp, N * 126, true))) {
    dual_free(p);
    return rc;
  }
  // S = lamb_bar of the current state (at a step boundary also the previous one's), D = 0: with
  // kP = 0, kI = rho and no saturation the law is then the plain update
  hipError_t e = hipMemcpy(d.par, gains, (size_t)rows * DPAR * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess)
    e = hipMemcpy2DAsync(d.S, L, p->bar + S_LB, STATE * sizeof(double), L, N, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipMemcpyAsync(d.Sp, d.S, N * L, hipMemcpyDeviceToDevice, h->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    dual_free(p);
    return pfail(h, PIADMM_E_HIP, std::string("obca_dual_plan: ") + hipGetErrorString(e));
  }
  d.rows = rows;
  d.stride = rows > 1 ? DPAR : 0;
  d.on = true;
  return 0;
}

int32_t piadmm_obca_dual_pi(piadmm_obca_t h, int32_t n, const double* w, const double* zb, const double* lamb,
                            const int32_t* status, const double* gains, int32_t rows, double* S, double* D,
                            double* lamb_out, double* dres_out) {
  using namespace obca_plan;
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_dual_pi: 1 <= n <= 2^20");
  if (!w || !zb || !lamb || !status || !gains || !S || !D || !lamb_out || !dres_out)
    return pfail(h, PIADMM_E_ARG, "obca_dual_pi: null argument");
  if (int rc = dual_rows_check(h, gains, rows, n, "obca_dual_pi")) return rc;
  const size_t N = (size_t)n;
  const double* in[] = {w, zb, lamb, S, D};
  const char* names[] = {"w", "zb", "lamb", "S", "D"};
  for (int a = 0; a < 5; ++a)
    for (size_t i = 0; i < N * 126; ++i)
      if (!std::isfinite(in[a][i]))
        return pfail(h, PIADMM_E_ARG, std::string("obca_dual_pi: ") + names[a] + " of scenario " +
                     std::to_string(i / 126) + " is not finite");
  // the kernel reads an edge record, an edge output and the slots' statuses: the caller's arrays in
  // those layouts, scenario k of the identity list
  std::vector<double> rec(N * EREC, 0.0), out(N * EOUT, 0.0);
  std::vector<int> ist(N * NT * 3, 0), ident(N);
  for (size_t k = 0; k < N; ++k) {
    ident[k] = (int)k;
    for (int i = 0; i < 126; ++i) {
      const int vt = i / 9, li = i % 9;
      rec[k * EREC + (li < 5 ? E_LX + vt * 5 + li : E_LIJ + vt * 4 + (li - 5))] = w[k * 126 + i];
      rec[k * EREC + E_LB + i] = lamb[k * 126 + i];
      out[k * EOUT + EO_ZB + i] = zb[k * 126 + i];
    }
    for (int t = 0; t < NT; ++t) ist[(k * NT + t) * 3] = status[k * NT + t];
  }
  PHIP(h, hipSetDevice(h->device));
  // the call's own buffers: neither the handle's local and edge buffers nor an open plan is touched
  double *d_rec = nullptr, *d_out = nullptr, *d_g = nullptr, *d_S = nullptr, *d_D = nullptr, *d_Sp = nullptr,
         *d_Dp = nullptr;
  int *d_ist = nullptr, *d_act = nullptr;
  const size_t B = sizeof(double);
  auto run = [&]() -> int {
    if (int rc = dalloc(h, &d_rec, N * EREC, false)) return rc;
    if (int rc = dalloc(h, &d_out, N * EOUT, false)) return rc;
    if (int rc = dalloc(h, &d_g, (size_t)rows * DPAR, false)) return rc;
    if (int rc = dalloc(h, &d_S, N * 126, false)) return rc;
    if (int rc = dalloc(h, &d_D, N * 126, false)) return rc;
    if (int rc = dalloc(h, &d_Sp, N * 126, true)) return rc;
    if (int rc = dalloc(h, &d_Dp, N * 126, true)) return rc;
    if (int rc = dalloc(h, &d_ist, N * NT * 3, false)) return rc;
    if (int rc = dalloc(h, &d_act, N, false)) return rc;
    PHIP(h, hipMemcpyAsync(d_rec, rec.data(), N * EREC * B, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_out, out.data(), N * EOUT * B, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_g, gains, (size_t)rows * DPAR * B, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_S, S, N * 126 * B, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_D, D, N * 126 * B, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_ist, ist.data(), N * NT * 3 * sizeof(int), hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_act, ident.data(), N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_plan_dual_pi, dim3(blocks_for(n)), dim3(64 * PW), 0, h->stream, d_act, n, d_rec, d_out, d_ist,
                       d_g, rows > 1 ? DPAR : 0, d_S, d_D, d_Sp, d_Dp);
    PHIP(h, hipGetLastError());
    PHIP(h, hipMemcpyAsync(out.data(), d_out, N * EOUT * B, hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipMemcpyAsync(S, d_S, N * 126 * B, hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipMemcpyAsync(D, d_D, N * 126 * B, hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  void* dev[] = {d_rec, d_out, d_g, d_S, d_D, d_Sp, d_Dp, d_ist, d_act};
  for (void* q : dev)
    if (q) (void)hipFree(q);
  if (rc) return rc;
  for (size_t k = 0; k < N; ++k) {
    for (int i = 0; i < 126; ++i) lamb_out[k * 126 + i] = out[k * EOUT + EO_LBN + i];
    for (int t = 0; t < NT; ++t) dres_out[k * NT + t] = out[k * EOUT + EO_DRES + t];
  }
  return 0;
}

int32_t piadmm_obca_order_plan(piadmm_obca_t h, int32_t mode, const int32_t* work_init) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_order_plan")) return rc;
  if (mode != 0 && mode != 1) return pfail(h, PIADMM_E_ARG, "obca_order_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  if (mode == 1) {
    if (n > ORDER_CLAMP) return pfail(h, PIADMM_E_ARG, "obca_order_plan: n_scenarios < 2^21");
    if (work_init)
      for (int k = 0; k < n; ++k)
        if (work_init[2 * (size_t)k] < 0 || work_init[2 * (size_t)k + 1] < 0)
          return pfail(h, PIADMM_E_ARG, "obca_order_plan: row " + std::to_string(k) + ": work_init >= 0");
  }
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_order_plan: only at a step boundary (an MPC step is open)");
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  // at a step boundary every scenario is active: the current list is all n of them
  const size_t N = (size_t)n;
  std::vector<int> ident(N);
  for (int k = 0; k < n; ++k) ident[k] = k;
  // with a clock the current list is the alive scenarios, ascending in ck.list
  const int m_cur = p->ck.on ? p->ck.n_list : n;
  if (mode == 0) {
    if (p->ord.on && p->ck.on) {
      if (m_cur > 0)
        PHIP(h, hipMemcpy(p->act[p->cur], p->ck.list, (size_t)m_cur * sizeof(int), hipMemcpyDeviceToDevice));
    } else if (p->ord.on) {
      PHIP(h, hipMemcpy(p->act[p->cur], ident.data(), N * sizeof(int), hipMemcpyHostToDevice));
    }
    order_free(p);
    return 0;
  }
  int *work = nullptr, *tmp = nullptr;
  hipError_t e = hipMalloc(&work, 2 * N * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&tmp, N * sizeof(int));
  if (e == hipSuccess)
    e = work_init ? hipMemcpy(work, work_init, 2 * N * sizeof(int), hipMemcpyHostToDevice)
                  : hipMemset(work, 0, 2 * N * sizeof(int));
  if (e == hipSuccess) e = hipMemcpy(tmp, ident.data(), N * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess && m_cur > 0) {
    // the current list re-sorted at once (zero work: ascending, as it was)
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(m_cur)), dim3(64 * PW), 0, h->stream,
                       p->ck.on ? (const int*)p->ck.list : (const int*)tmp, (const int*)nullptr, m_cur, work,
                       p->act[p->cur]);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    if (work) (void)hipFree(work);
    if (tmp) (void)hipFree(tmp);
    return pfail(h, PIADMM_E_HIP, std::string("obca_order_plan: ") + hipGetErrorString(e));
  }
  order_free(p);
  p->ord.work = work;
  p->ord.tmp = tmp;
  p->ord.on = true;
  return 0;
}

int32_t piadmm_obca_order(piadmm_obca_t h, const int32_t* list, int32_t m, const int32_t* work, int32_t n,
                          int32_t* out) {
  using namespace obca_plan;
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > ORDER_CLAMP) return pfail(h, PIADMM_E_ARG, "obca_order: 1 <= n < 2^21");
  if (m < 1 || m > n) return pfail(h, PIADMM_E_ARG, "obca_order: 1 <= m <= n");
  if (!list || !work || !out) return pfail(h, PIADMM_E_ARG, "obca_order: null argument");
  std::vector<char> seen((size_t)n, 0);
  for (int k = 0; k < m; ++k) {
    if (list[k] < 0 || list[k] >= n || seen[(size_t)list[k]])
      return pfail(h, PIADMM_E_ARG, "obca_order: list[" + std::to_string(k) + "] must be a scenario below n, listed once");
    seen[(size_t)list[k]] = 1;
  }
  for (int k = 0; k < n; ++k)
    if (work[2 * (size_t)k] < 0 || work[2 * (size_t)k + 1] < 0)
      return pfail(h, PIADMM_E_ARG, "obca_order: row " + std::to_string(k) + ": work >= 0");
  PHIP(h, hipSetDevice(h->device));
  // the call's own buffers: neither the handle's local and edge buffers nor an open plan is touched
  int *d_in = nullptr, *d_work = nullptr, *d_out = nullptr;
  const size_t M = (size_t)m, N = (size_t)n;
  auto run = [&]() -> int {
    if (int rc = dalloc(h, &d_in, M, false)) return rc;
    if (int rc = dalloc(h, &d_work, 2 * N, false)) return rc;
    if (int rc = dalloc(h, &d_out, M, true)) return rc;
    PHIP(h, hipMemcpyAsync(d_in, list, M * sizeof(int), hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_work, work, 2 * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_plan_order, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, d_in, (const int*)nullptr, m,
                       d_work, d_out);
    PHIP(h, hipGetLastError());
    PHIP(h, hipMemcpyAsync(out, d_out, M * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  if (d_in) (void)hipFree(d_in);
  if (d_work) (void)hipFree(d_work);
  if (d_out) (void)hipFree(d_out);
  return rc;
}

int32_t piadmm_obca_clock_plan(piadmm_obca_t h, int32_t mode, const int32_t* clock_init) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_clock_plan")) return rc;
  if (mode != 0 && mode != 1) return pfail(h, PIADMM_E_ARG, "obca_clock_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n, n_ref = p->cfg.n_ref;
  const size_t N = (size_t)n;
  std::vector<int> rec(3 * N);
  if (mode == 1) {
    for (int k = 0; k < n; ++k) {
      const int c0 = clock_init ? clock_init[2 * (size_t)k] : p->t_step;
      const int len = clock_init ? clock_init[2 * (size_t)k + 1] : n_ref;
      if (const char* why = clock_row_check(c0, len, n_ref))
        return pfail(h, PIADMM_E_ARG, "obca_clock_plan: row " + std::to_string(k) + ": " + why);
      rec[3 * (size_t)k] = c0;
      rec[3 * (size_t)k + 1] = len;
      rec[3 * (size_t)k + 2] = 1;
    }
  }
  if (mode == 1 && p->fb.on)
    return pfail(h, PIADMM_E_STATE, "obca_clock_plan: feedback is attached (obca_feedback_plan: the tape has no per-scenario clocks)");
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_clock_plan: only at a step boundary (an MPC step is open)");
  if (mode == 0) {
    if (!p->ck.on) return 0;
    const std::vector<int>& k = p->ck.host;
    for (int s = 0; s < n; ++s)
      if (!k[3 * (size_t)s + 2] || k[3 * (size_t)s] != k[0] || k[3 * (size_t)s + 1] != n_ref)
        return pfail(h, PIADMM_E_STATE, "obca_clock_plan: detaching needs every scenario alive, on one c and with len = n_ref (scenario " +
                     std::to_string(s) + ")");
    PHIP(h, hipSetDevice(h->device));
    PHIP(h, hipStreamSynchronize(h->stream));
    // every scenario is alive: the current list already holds all n, in the plan's order
    p->t_step = k[0];
    clock_free(p);
    return 0;
  }
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  piadmm_obca_plan_s::clock_s nk;
  std::vector<int> ident(N);
  for (int k = 0; k < n; ++k) ident[(size_t)k] = k;
  hipError_t e = hipMalloc(&nk.clk, 3 * N * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&nk.flag[0], N * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&nk.flag[1], N * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&nk.list, N * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&nk.ident, N * sizeof(int));
  if (e == hipSuccess) e = hipMalloc(&nk.win, N * WIN * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(nk.clk, rec.data(), 3 * N * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(nk.ident, ident.data(), N * sizeof(int), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemset(nk.flag[0], 0, N * sizeof(int));
  if (e == hipSuccess) e = hipMemset(nk.flag[1], 0, N * sizeof(int));
  if (e == hipSuccess) e = hipMemset(nk.list, 0, N * sizeof(int));
  if (e == hipSuccess) e = hipMemset(nk.win, 0, N * WIN * sizeof(double));
  if (e != hipSuccess) {
    clock_free_buffers(nk);
    return pfail(h, PIADMM_E_HIP, std::string("obca_clock_plan: ") + hipGetErrorString(e));
  }
  clock_free(p);
  p->ck = nk;
  p->ck.host = rec;
  p->ck.cur = 0;
  p->ck.n_list = n;
  p->ck.on = true;
  // every row is alive: the windows, the flags and the list of all n (sorted, with the order on)
  if (int rc = clock_lists(h, p, nullptr, 0, n)) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  PHIP(h, hipStreamSynchronize(h->stream));
  p->n_act = n;
  return 0;
}

int32_t piadmm_obca_clock_admit(piadmm_obca_t h, int32_t m, const int32_t* slots, const int32_t* clock,
                                const double* state, const double* ref, const double* par, const int32_t* prob,
                                const double* primal_thres, const double* dual_thres) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_clock_admit")) return rc;
  const int n = p->n, n_ref = p->cfg.n_ref;
  if (m < 1 || m > n) return pfail(h, PIADMM_E_ARG, "obca_clock_admit: 1 <= m <= n_scenarios");
  if (!slots || !clock) return pfail(h, PIADMM_E_ARG, "obca_clock_admit: null argument (slots, clock)");
  std::vector<char> seen((size_t)n, 0);
  for (int k = 0; k < m; ++k) {
    if (slots[k] < 0 || slots[k] >= n || seen[(size_t)slots[k]])
      return pfail(h, PIADMM_E_ARG, "obca_clock_admit: slots[" + std::to_string(k) + "] must be a scenario below n, listed once");
    seen[(size_t)slots[k]] = 1;
  }
  for (int k = 0; k < m; ++k) {
    const std::string row = "obca_clock_admit: row " + std::to_string(k) + ": ";
    if (const char* why = clock_row_check(clock[2 * (size_t)k], clock[2 * (size_t)k + 1], n_ref))
      return pfail(h, PIADMM_E_ARG, row + why);
    if (par)
      if (const char* why = row_check(par + (size_t)k * TAB)) return pfail(h, PIADMM_E_ARG, row + why);
    if (prob && prob[k] != 0 && prob[k] != 1) return pfail(h, PIADMM_E_ARG, row + "prob must be 0 or 1");
  }
  if (!p->ck.on) return pfail(h, PIADMM_E_STATE, "obca_clock_admit: no clock attached (obca_clock_plan)");
  if (p->tr.on) return pfail(h, PIADMM_E_STATE, "obca_clock_admit: a trace is attached (its minima would mix two tenants)");
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_clock_admit: only at a step boundary (an MPC step is open)");
  if (ref && p->ref_rows != n) return pfail(h, PIADMM_E_STATE, "obca_clock_admit: ref needs a plan with a reference per scenario (obca_fleet_begin)");
  if (par && p->tab_rows != n) return pfail(h, PIADMM_E_STATE, "obca_clock_admit: par needs a plan with a parameter row per scenario (obca_fleet_begin)");
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  const size_t D = sizeof(double), ref_one = (size_t)2 * n_ref * 5;
  for (int k = 0; k < m; ++k) {
    const size_t s = (size_t)slots[k], K = (size_t)k;
    if (state) {
      PHIP(h, hipMemcpy(p->bar + s * STATE, state + K * STATE, STATE * D, hipMemcpyHostToDevice));
      PHIP(h, hipMemcpy(p->barp + s * STATE, state + K * STATE, STATE * D, hipMemcpyHostToDevice));
    }
    if (ref) PHIP(h, hipMemcpy(p->ref + s * ref_one, ref + K * ref_one, ref_one * D, hipMemcpyHostToDevice));
    if (par) {
      PHIP(h, hipMemcpy(p->tab + s * TAB, par + K * TAB, TAB * D, hipMemcpyHostToDevice));
      p->admm_rows[s] = (int)par[K * TAB + T_ADMM];
    }
    if (prob) PHIP(h, hipMemcpy(p->prob + s, prob + K, sizeof(int), hipMemcpyHostToDevice));
    if (primal_thres) PHIP(h, hipMemcpy(p->pth + s, primal_thres + K, D, hipMemcpyHostToDevice));
    if (dual_thres) PHIP(h, hipMemcpy(p->dth + s, dual_thres + K, D, hipMemcpyHostToDevice));
    // the slot starts as a scenario of a fresh plan does
    PHIP(h, hipMemset(p->ctrl + s * NCTRL, 0, NCTRL * D));
    PHIP(h, hipMemset(p->ctrlp + s * NCTRL, 0, NCTRL * D));
    PHIP(h, hipMemset(p->X + s * NX, 0, NX * D));
    PHIP(h, hipMemset(p->lamb + s * 126, 0, 126 * D));
    PHIP(h, hipMemset(p->iters + s, 0, sizeof(int)));
    PHIP(h, hipMemset(p->mask + 2 * s, 0, 2 * sizeof(int)));
    if (p->du.on) {
      PHIP(h, hipMemcpy(p->du.S + s * 126, p->bar + s * STATE + S_LB, 126 * D, hipMemcpyDeviceToDevice));
      PHIP(h, hipMemcpy(p->du.Sp + s * 126, p->bar + s * STATE + S_LB, 126 * D, hipMemcpyDeviceToDevice));
      PHIP(h, hipMemset(p->du.D + s * 126, 0, 126 * D));
      PHIP(h, hipMemset(p->du.Dp + s * 126, 0, 126 * D));
    }
    if (p->ord.on) PHIP(h, hipMemset(p->ord.work + 2 * s, 0, 2 * sizeof(int)));
    int* k3 = p->ck.host.data() + 3 * s;
    k3[0] = clock[2 * K];
    k3[1] = clock[2 * K + 1];
    k3[2] = 1;
    PHIP(h, hipMemcpy(p->ck.clk + 3 * s, k3, 3 * sizeof(int), hipMemcpyHostToDevice));
  }
  p->max_iter_all = std::max(0, *std::max_element(p->admm_rows.begin(), p->admm_rows.end()));
  int n_alive = 0;
  for (int s = 0; s < n; ++s) n_alive += p->ck.host[3 * (size_t)s + 2];
  // the windows, the flags and the list again, over all n (the order, when attached, re-sorts it)
  if (int rc = clock_lists(h, p, nullptr, p->ck.cur, n_alive)) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  PHIP(h, hipStreamSynchronize(h->stream));
  p->ck.n_list = n_alive;
  p->n_act = n_alive;
  return 0;
}

int32_t piadmm_obca_clock_tick(piadmm_obca_t h, int32_t n, const int32_t* clock_in, const int32_t* ran,
                               const double* ref, int32_t ref_rows, int32_t n_ref, int32_t* clock_out,
                               double* window_out, int32_t* list_out, int32_t* count_out) {
  using namespace obca_plan;
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_clock_tick: 1 <= n <= 2^20");
  if (!clock_in || !ran || !ref || !clock_out || !window_out || !list_out || !count_out)
    return pfail(h, PIADMM_E_ARG, "obca_clock_tick: null argument");
  if (ref_rows != 1 && ref_rows != n) return pfail(h, PIADMM_E_ARG, "obca_clock_tick: ref_rows must be 1 or n");
  if (n_ref < 8 || n_ref > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_clock_tick: 8 <= n_ref <= 2^20");
  for (int k = 0; k < n; ++k) {
    const int c = clock_in[3 * (size_t)k], len = clock_in[3 * (size_t)k + 1];
    const char* why = c < 0 || c > (1 << 30) ? "0 <= c <= 2^30" : len < 8 || len > n_ref ? "8 <= len <= n_ref"
                      : ran[k] != 0 && ran[k] != 1 ? "ran 0 or 1" : nullptr;
    if (why) return pfail(h, PIADMM_E_ARG, "obca_clock_tick: row " + std::to_string(k) + ": " + why);
  }
  PHIP(h, hipSetDevice(h->device));
  // the call's own buffers: neither the handle's local and edge buffers nor an open plan is touched
  int *d_clk = nullptr, *d_ran = nullptr, *d_alive = nullptr, *d_ident = nullptr, *d_list = nullptr, *d_count = nullptr;
  double *d_ref = nullptr, *d_win = nullptr;
  const size_t N = (size_t)n, ref_one = (size_t)2 * n_ref * 5, R = ref_one * (size_t)ref_rows;
  std::vector<int> ident(N);
  for (int k = 0; k < n; ++k) ident[(size_t)k] = k;
  auto run = [&]() -> int {
    if (int rc = dalloc(h, &d_clk, 3 * N, false)) return rc;
    if (int rc = dalloc(h, &d_ran, N, false)) return rc;
    if (int rc = dalloc(h, &d_alive, N, true)) return rc;
    if (int rc = dalloc(h, &d_ident, N, false)) return rc;
    if (int rc = dalloc(h, &d_list, N, true)) return rc;
    if (int rc = dalloc(h, &d_count, (size_t)1, true)) return rc;
    if (int rc = dalloc(h, &d_ref, R, false)) return rc;
    if (int rc = dalloc(h, &d_win, N * WIN, true)) return rc;
    PHIP(h, hipMemcpyAsync(d_clk, clock_in, 3 * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_ran, ran, N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_ident, ident.data(), N * sizeof(int), hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_ref, ref, R * sizeof(double), hipMemcpyHostToDevice, h->stream));
    hipLaunchKernelGGL(k_plan_clock, dim3(blocks_for(n)), dim3(64 * PW), 0, h->stream, n, d_clk, d_ran, d_ref,
                       ref_rows > 1 ? (int)ref_one : 0, n_ref, d_win, d_alive);
    PHIP(h, hipGetLastError());
    hipLaunchKernelGGL(k_plan_compact, dim3(1), dim3(CT), 0, h->stream, d_ident, d_alive, n, d_list, d_count);
    PHIP(h, hipGetLastError());
    PHIP(h, hipMemcpyAsync(clock_out, d_clk, 3 * N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipMemcpyAsync(window_out, d_win, N * WIN * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipMemcpyAsync(list_out, d_list, N * sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipMemcpyAsync(count_out, d_count, sizeof(int), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  void* dev[] = {d_clk, d_ran, d_alive, d_ident, d_list, d_count, d_ref, d_win};
  for (void* q : dev)
    if (q) (void)hipFree(q);
  return rc;
}

int32_t piadmm_obca_trace_begin(piadmm_obca_t h, int32_t cap_steps, int32_t flags) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_trace_begin")) return rc;
  if (cap_steps < 1 || cap_steps > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_trace_begin: 1 <= cap_steps <= 2^20");
  if (flags & ~PIADMM_OBCA_TRACE_LAMBDA) return pfail(h, PIADMM_E_ARG, "obca_trace_begin: unknown flag bits");
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_trace_begin: only at a step boundary (an MPC step is open)");
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  trace_free(p);
  auto& t = p->tr;
  const size_t N = (size_t)p->n, C = (size_t)cap_steps;
  int rc = 0;
  if ((rc = dalloc(h, &t.states, (C + 1) * N * 10, false)) || (rc = dalloc(h, &t.clear, (C + 1) * N * 2, false)) ||
      (rc = dalloc(h, &t.iters, C * N, false)) || (rc = dalloc(h, &t.mask, C * N * 2, false)) ||
      (rc = dalloc(h, &t.primal, C * N, false)) || (rc = dalloc(h, &t.dual, C * N, false)) ||
      (rc = dalloc(h, &t.summary, N * TSUM, true)) ||
      ((flags & PIADMM_OBCA_TRACE_LAMBDA) && (rc = dalloc(h, &t.lamb, C * N * 126, false)))) {
    trace_free(p);
    return rc;
  }
  t.cap = cap_steps;
  t.rows = 0;
  t.flags = flags;
  if ((rc = trace_append(h, p, 0))) {
    (void)hipStreamSynchronize(h->stream);
    trace_free(p);
    return rc;
  }
  PHIP(h, hipStreamSynchronize(h->stream));
  t.on = true;
  return 0;
}

int32_t piadmm_obca_trace_run(piadmm_obca_t h, int32_t n_steps, int32_t* steps_done) {
  piadmm_obca_plan_s* p = nullptr;
  if (steps_done) *steps_done = 0;
  if (int rc = open_trace(h, &p, "obca_trace_run")) return rc;
  if (n_steps < 1) return pfail(h, PIADMM_E_ARG, "obca_trace_run: n_steps >= 1");
  if ((int64_t)p->tr.rows + n_steps > p->tr.cap)
    return pfail(h, PIADMM_E_STATE, "obca_trace_run: " + std::to_string(n_steps) + " steps do not fit the trace (" +
                 std::to_string(p->tr.rows) + " of " + std::to_string(p->tr.cap) + " rows used)");
  if (feedback_exhausted(p, n_steps))
    return pfail(h, PIADMM_E_STATE, "obca_trace_run: disturbance tape exhausted before " + std::to_string(n_steps) +
                 " steps (" + std::to_string(p->fb.steps) + " of " + std::to_string(p->fb.cap) + " rows used)");
  if (noise_exhausted(p, n_steps))
    return pfail(h, PIADMM_E_STATE, "obca_trace_run: noise step index exhausted before " + std::to_string(n_steps) + " steps");
  if (p->ck.on) {
    // the steps the longest-lived scenario has left
    int left = 0;
    for (int s = 0; s < p->n; ++s)
      if (p->ck.host[3 * (size_t)s + 2])
        left = std::max(left, p->ck.host[3 * (size_t)s + 1] - 8 - p->ck.host[3 * (size_t)s] + 1);
    if (left == 0) return pfail(h, PIADMM_E_STATE, "obca_trace_run: no scenario alive");
    if (n_steps > left)
      return pfail(h, PIADMM_E_STATE, "obca_trace_run: every reference ends before " + std::to_string(n_steps) +
                   " steps (" + std::to_string(left) + " left)");
  } else if ((int64_t)p->t_step + n_steps - 1 + 8 > p->cfg.n_ref)
    return pfail(h, PIADMM_E_STATE, "obca_trace_run: the reference ends before " + std::to_string(n_steps) + " steps");
  // a host loop of the plan's bounded launches: every step ends in piadmm_obca_plan_shift, which appends its row
  for (int k = 0; k < n_steps; ++k) {
    if (int rc = piadmm_obca_plan_step(h, nullptr)) return rc;
    if (steps_done) *steps_done = k + 1;
  }
  return 0;
}

int32_t piadmm_obca_trace_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_trace(h, &p, "obca_trace_get")) return rc;
  const auto& t = p->tr;
  const int64_t n = p->n, R = t.rows, D = sizeof(double), I = sizeof(int32_t);
  const void* src = nullptr;
  int64_t want = -1;
  switch (what) {
    case PIADMM_OBCA_TRACE_GET_STATES: src = t.states; want = (R + 1) * n * 10 * D; break;
    case PIADMM_OBCA_TRACE_GET_CLEARANCE: src = t.clear; want = (R + 1) * n * 2 * D; break;
    case PIADMM_OBCA_TRACE_GET_ITERS: src = t.iters; want = R * n * I; break;
    case PIADMM_OBCA_TRACE_GET_STATUS_MASK: src = t.mask; want = R * n * 2 * I; break;
    case PIADMM_OBCA_TRACE_GET_PRIMAL: src = t.primal; want = R * n * D; break;
    case PIADMM_OBCA_TRACE_GET_DUAL: src = t.dual; want = R * n * D; break;
    case PIADMM_OBCA_TRACE_GET_LAMBDA:
      if (!t.lamb) return pfail(h, PIADMM_E_STATE, "obca_trace_get: the trace keeps no lamb_bar (PIADMM_OBCA_TRACE_LAMBDA)");
      src = t.lamb; want = R * n * 126 * D; break;
    case PIADMM_OBCA_TRACE_GET_SUMMARY: src = t.summary; want = n * TSUM * D; break;
    case PIADMM_OBCA_TRACE_GET_ROWS: want = I; break;
    default: return pfail(h, PIADMM_E_ARG, "obca_trace_get: unknown item " + std::to_string(what));
  }
  if (bytes != want)
    return pfail(h, PIADMM_E_ARG, "obca_trace_get: item " + std::to_string(what) + " is " + std::to_string(want) +
                 " bytes, not " + std::to_string(bytes));
  if (want == 0) return 0;
  if (!out) return pfail(h, PIADMM_E_ARG, "obca_trace_get: out");
  if (what == PIADMM_OBCA_TRACE_GET_ROWS) { *static_cast<int32_t*>(out) = t.rows; return 0; }
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipMemcpyAsync(out, src, (size_t)want, hipMemcpyDeviceToHost, h->stream));
  PHIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_trace_end(piadmm_obca_t h) {
  if (!h) return PIADMM_E_ARG;
  if (!h->plan || !h->plan->tr.on) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  trace_free(h->plan);
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Export and import of running tenants (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
namespace {
// the fp64 words of a record of a plan with references of n_ref rows, with or without a law
int64_t tenant_f64(int n_ref, bool law) {
  return (int64_t)PIADMM_OBCA_TENANT_F64 + 10 * (int64_t)n_ref + (law ? PIADMM_OBCA_TENANT_F64_LAW : 0);
}
int64_t tenant_rec_bytes(int n_ref, bool law) { return 8 * tenant_f64(n_ref, law) + 4 * PIADMM_OBCA_TENANT_INTS; }

// m and the slots of an export or an import: distinct scenarios below n
int tenant_slots_check(piadmm_obca_t h, const piadmm_obca_plan_s* p, int m, const int32_t* slots, const void* blob,
                       const std::string& who) {
  const int n = p->n;
  if (m < 1 || m > n) return pfail(h, PIADMM_E_ARG, who + ": 1 <= m <= n_scenarios");
  if (!slots || !blob) return pfail(h, PIADMM_E_ARG, who + ": null argument (slots, blob)");
  std::vector<char> seen((size_t)n, 0);
  for (int k = 0; k < m; ++k) {
    if (slots[k] < 0 || slots[k] >= n || seen[(size_t)slots[k]])
      return pfail(h, PIADMM_E_ARG, who + ": slots[" + std::to_string(k) + "] must be a scenario below n, listed once");
    seen[(size_t)slots[k]] = 1;
  }
  return 0;
}

// the staging buffer holds `bytes` of records and m slot numbers behind them
int stage_ensure(piadmm_obca_t h, piadmm_obca_plan_s* p, size_t bytes, int m) {
  const size_t need = bytes + (size_t)m * sizeof(int);
  if (p->stg.cap >= need) return 0;
  PHIP(h, hipStreamSynchronize(h->stream));
  stage_free(p);
  PHIP(h, hipMalloc(reinterpret_cast<void**>(&p->stg.buf), need));
  p->stg.cap = need;
  return 0;
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
  a.f64_words = (int)tenant_f64(p->cfg.n_ref, p->du.on);
  return a;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_tenant_export_bytes(piadmm_obca_t h, int32_t m, int64_t* bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_tenant_export_bytes")) return rc;
  if (m < 1 || m > p->n) return pfail(h, PIADMM_E_ARG, "obca_tenant_export_bytes: 1 <= m <= n_scenarios");
  if (!bytes) return pfail(h, PIADMM_E_ARG, "obca_tenant_export_bytes: null argument");
  *bytes = PIADMM_OBCA_TENANT_HEADER + (int64_t)m * tenant_rec_bytes(p->cfg.n_ref, p->du.on);
  return 0;
}

int32_t piadmm_obca_tenant_export(piadmm_obca_t h, int32_t m, const int32_t* slots, void* blob, int64_t bytes) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_tenant_export")) return rc;
  if (int rc = tenant_slots_check(h, p, m, slots, blob, "obca_tenant_export")) return rc;
  const int64_t rec_bytes = tenant_rec_bytes(p->cfg.n_ref, p->du.on), body = (int64_t)m * rec_bytes;
  if (bytes != PIADMM_OBCA_TENANT_HEADER + body)
    return pfail(h, PIADMM_E_ARG, "obca_tenant_export: the blob is " + std::to_string(PIADMM_OBCA_TENANT_HEADER + body) +
                 " bytes, not " + std::to_string(bytes));
  if (p->fb.on) return pfail(h, PIADMM_E_STATE, "obca_tenant_export: feedback is attached (the tenant record has no room for the tape)");
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_tenant_export: only at a step boundary (an MPC step is open)");
  PHIP(h, hipSetDevice(h->device));
  if (int rc = stage_ensure(h, p, (size_t)body, m)) return rc;
  int* d_list = reinterpret_cast<int*>(p->stg.buf + body);
  char* out = static_cast<char*>(blob);
  PHIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_export, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, (const int*)d_list, m,
                     tenant_view(p), reinterpret_cast<double*>(p->stg.buf));
  PHIP(h, hipGetLastError());
  PHIP(h, hipMemcpyAsync(out + PIADMM_OBCA_TENANT_HEADER, p->stg.buf, (size_t)body, hipMemcpyDeviceToHost, h->stream));
  PHIP(h, hipStreamSynchronize(h->stream));
  const int32_t hdr[PIADMM_OBCA_TENANT_HEADER / 4] = {
      PIADMM_OBCA_TENANT_MAGIC, PIADMM_ABI_VERSION, m, p->cfg.n_ref, p->cfg.update_lamb_ij, p->du.on ? 1 : 0,
      p->ord.on ? 1 : 0, (int32_t)tenant_f64(p->cfg.n_ref, p->du.on), PIADMM_OBCA_TENANT_INTS, (int32_t)rec_bytes,
      PIADMM_OBCA_TENANT_HEADER, 0, 0, 0, 0, 0};
  std::memcpy(out, hdr, sizeof(hdr));
  return 0;
}

int32_t piadmm_obca_tenant_import(piadmm_obca_t h, int32_t m, const int32_t* slots, const void* blob, int64_t bytes) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_tenant_import")) return rc;
  if (int rc = tenant_slots_check(h, p, m, slots, blob, "obca_tenant_import")) return rc;
  const int n = p->n, n_ref = p->cfg.n_ref;
  const char* in = static_cast<const char*>(blob);
  // the header against itself, then against the plan
  if (bytes < PIADMM_OBCA_TENANT_HEADER) return pfail(h, PIADMM_E_ARG, "obca_tenant_import: the blob is shorter than its header");
  int32_t hdr[PIADMM_OBCA_TENANT_HEADER / 4];
  std::memcpy(hdr, in, sizeof(hdr));
  if (hdr[0] != PIADMM_OBCA_TENANT_MAGIC) return pfail(h, PIADMM_E_ARG, "obca_tenant_import: bad magic (not a tenant blob)");
  if (hdr[1] != PIADMM_ABI_VERSION)
    return pfail(h, PIADMM_E_ARG, "obca_tenant_import: the blob is of ABI " + std::to_string(hdr[1]));
  if (hdr[2] != m) return pfail(h, PIADMM_E_ARG, "obca_tenant_import: the blob holds " + std::to_string(hdr[2]) + " tenants, not m");
  const bool law = hdr[5] == 1, order = hdr[6] == 1;
  if (hdr[3] < 8 || hdr[3] > (1 << 20) || (hdr[4] != 0 && hdr[4] != 1) || (hdr[5] != 0 && hdr[5] != 1) ||
      (hdr[6] != 0 && hdr[6] != 1) || hdr[10] != PIADMM_OBCA_TENANT_HEADER || hdr[8] != PIADMM_OBCA_TENANT_INTS ||
      (int64_t)hdr[7] != tenant_f64(hdr[3], law) || (int64_t)hdr[9] != tenant_rec_bytes(hdr[3], law))
    return pfail(h, PIADMM_E_ARG, "obca_tenant_import: bad header (flags or section sizes)");
  const int64_t rec_bytes = hdr[9], body = (int64_t)m * rec_bytes;
  if (bytes != PIADMM_OBCA_TENANT_HEADER + body)
    return pfail(h, PIADMM_E_ARG, "obca_tenant_import: the blob is " + std::to_string(PIADMM_OBCA_TENANT_HEADER + body) +
                 " bytes, not " + std::to_string(bytes));
  if (hdr[3] != n_ref)
    return pfail(h, PIADMM_E_ARG, "obca_tenant_import: n_ref mismatch (the blob " + std::to_string(hdr[3]) + ", the plan " +
                 std::to_string(n_ref) + ")");
  if (hdr[4] != p->cfg.update_lamb_ij) return pfail(h, PIADMM_E_ARG, "obca_tenant_import: update_lamb_ij mismatch");
  // the records: what the kernels rely on (the rows, prob, the clocks)
  const size_t F = (size_t)hdr[7];
  const size_t law_at = (size_t)PIADMM_OBCA_TENANT_F64 + 10 * (size_t)n_ref;
  auto rec_f64 = [&](int k, size_t word, double* dst, int count) {
    std::memcpy(dst, in + PIADMM_OBCA_TENANT_HEADER + (size_t)k * rec_bytes + 8 * word, sizeof(double) * (size_t)count);
  };
  std::vector<int32_t> ints((size_t)m * TR_INTS);
  std::vector<int> admm((size_t)m);
  for (int k = 0; k < m; ++k) {
    const std::string row = "obca_tenant_import: row " + std::to_string(k) + ": ";
    double par[TAB];
    rec_f64(k, TR_PAR, par, TAB);
    if (const char* why = row_check(par)) return pfail(h, PIADMM_E_ARG, row + why);
    admm[(size_t)k] = (int)par[T_ADMM];
    int32_t* ri = ints.data() + (size_t)k * TR_INTS;
    std::memcpy(ri, in + PIADMM_OBCA_TENANT_HEADER + (size_t)k * rec_bytes + 8 * F, sizeof(int32_t) * TR_INTS);
    if (ri[TI_PROB] != 0 && ri[TI_PROB] != 1) return pfail(h, PIADMM_E_ARG, row + "prob must be 0 or 1");
    if (ri[TI_CLOCK] < 0) return pfail(h, PIADMM_E_ARG, row + "c >= 0");
    if (ri[TI_CLOCK + 1] < 8 || ri[TI_CLOCK + 1] > n_ref) return pfail(h, PIADMM_E_ARG, row + "8 <= len <= n_ref");
    if (law) {
      double g[DPAR];
      rec_f64(k, law_at + 504, g, DPAR);
      if (const char* why = dual_row_check(g)) return pfail(h, PIADMM_E_ARG, row + "gains: " + why);
    }
  }
  // the destination
  if (p->fb.on) return pfail(h, PIADMM_E_STATE, "obca_tenant_import: feedback is attached (the tenant record has no room for the tape)");
  if (!p->ck.on) return pfail(h, PIADMM_E_STATE, "obca_tenant_import: no clock attached (obca_clock_plan)");
  if (p->tr.on) return pfail(h, PIADMM_E_STATE, "obca_tenant_import: a trace is attached (its minima would mix two tenants)");
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_tenant_import: only at a step boundary (an MPC step is open)");
  if (p->ref_rows != n || p->tab_rows != n)
    return pfail(h, PIADMM_E_STATE, "obca_tenant_import: needs a plan with a reference and a parameter row per scenario (obca_fleet_begin)");
  if (law != p->du.on)
    return pfail(h, PIADMM_E_STATE, law ? "obca_tenant_import: the blob carries a dual law, the plan has none attached"
                                        : "obca_tenant_import: the plan has a dual law attached, the blob carries none");
  if (order != p->ord.on)
    return pfail(h, PIADMM_E_STATE, order ? "obca_tenant_import: the blob carries the order's record, the plan has no order attached"
                                          : "obca_tenant_import: the plan has the order attached, the blob carries no record");
  PHIP(h, hipSetDevice(h->device));
  const bool gains_travel = law && p->du.rows == n;
  if (law && !gains_travel) {
    // one shared gains row: a read of 8 doubles, nothing is written
    double shared[DPAR], g[DPAR];
    PHIP(h, hipMemcpyAsync(shared, p->du.par, sizeof(shared), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    for (int k = 0; k < m; ++k) {
      rec_f64(k, law_at + 504, g, DPAR);
      if (std::memcmp(g, shared, sizeof(g)) != 0)
        return pfail(h, PIADMM_E_ARG, "obca_tenant_import: row " + std::to_string(k) +
                     ": the gains row differs from the plan's shared one");
    }
  }
  if (int rc = stage_ensure(h, p, (size_t)body, m)) return rc;
  int* d_list = reinterpret_cast<int*>(p->stg.buf + body);
  PHIP(h, hipMemcpyAsync(p->stg.buf, in + PIADMM_OBCA_TENANT_HEADER, (size_t)body, hipMemcpyHostToDevice, h->stream));
  PHIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  tenant_arrays a = tenant_view(p);
  if (!gains_travel) a.gains = nullptr;
  hipLaunchKernelGGL(k_plan_import, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, (const int*)d_list, m, a,
                     reinterpret_cast<const double*>(p->stg.buf));
  PHIP(h, hipGetLastError());
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
  p->max_iter_all = std::max(0, *std::max_element(p->admm_rows.begin(), p->admm_rows.end()));
  int n_alive = 0;
  for (int s = 0; s < n; ++s) n_alive += p->ck.host[3 * (size_t)s + 2];
  if (int rc = clock_lists(h, p, nullptr, p->ck.cur, n_alive)) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  PHIP(h, hipStreamSynchronize(h->stream));
  p->ck.n_list = n_alive;
  p->n_act = n_alive;
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Closed-loop feedback (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
extern "C" {

int32_t piadmm_obca_propagate(piadmm_obca_t h, int32_t n, const double* states, const double* ctrl, const double* par,
                              const double* w, double* out) {
  using namespace obca_plan;
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_propagate: 1 <= n <= 2^20");
  if (!states || !ctrl || !par || !out) return pfail(h, PIADMM_E_ARG, "obca_propagate: null argument");
  const size_t N = (size_t)n;
  int64_t bad = -1;
  if ((bad = first_not_finite(states, N * 10)) >= 0)
    return pfail(h, PIADMM_E_ARG, "obca_propagate: state pair " + std::to_string(bad / 10) + " is not finite");
  if ((bad = first_not_finite(ctrl, N * 4)) >= 0)
    return pfail(h, PIADMM_E_ARG, "obca_propagate: ctrl of scenario " + std::to_string(bad / 4) + " is not finite");
  if (w && (bad = first_not_finite(w, N * 10)) >= 0)
    return pfail(h, PIADMM_E_ARG, "obca_propagate: w of scenario " + std::to_string(bad / 10) + " is not finite");
  for (int k = 0; k < n; ++k)
    if (const char* why = feedback_row_check(par + (size_t)k * FPAR))
      return pfail(h, PIADMM_E_ARG, "obca_propagate: row " + std::to_string(k) + ": " + why);
  PHIP(h, hipSetDevice(h->device));
  // the call's own buffers: neither the handle's local and edge buffers nor an open plan is touched
  double *d_st = nullptr, *d_ct = nullptr, *d_par = nullptr, *d_w = nullptr, *d_out = nullptr;
  const size_t B = sizeof(double);
  auto run = [&]() -> int {
    if (int rc = dalloc(h, &d_st, N * 10, false)) return rc;
    if (int rc = dalloc(h, &d_ct, N * 4, false)) return rc;
    if (int rc = dalloc(h, &d_par, N * FPAR, false)) return rc;
    if (w)
      if (int rc = dalloc(h, &d_w, N * 10, false)) return rc;
    if (int rc = dalloc(h, &d_out, N * 10, true)) return rc;
    PHIP(h, hipMemcpyAsync(d_st, states, N * 10 * B, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_ct, ctrl, N * 4 * B, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(d_par, par, N * FPAR * B, hipMemcpyHostToDevice, h->stream));
    if (w) PHIP(h, hipMemcpyAsync(d_w, w, N * 10 * B, hipMemcpyHostToDevice, h->stream));
    plant_io io{};
    io.x0 = d_st;  io.x0_s = 10;
    io.ctrl = d_ct;  io.ctrl_s = 4;  io.ctrl_v = 2;  io.ctrl_w = 1;
    io.par = d_par;  io.par_s = FPAR;
    io.w = d_w;  io.w_s = 10;
    io.out = d_out;
    hipLaunchKernelGGL(k_plan_propagate, dim3(lane_blocks(2 * n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr, n,
                       io);
    PHIP(h, hipGetLastError());
    PHIP(h, hipMemcpyAsync(out, d_out, N * 10 * B, hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  void* dev[] = {d_st, d_ct, d_par, d_w, d_out};
  for (void* q : dev)
    if (q) (void)hipFree(q);
  return rc;
}

int32_t piadmm_obca_feedback_plan(piadmm_obca_t h, int32_t mode, const double* par, int32_t rows, const double* tape,
                                  int32_t cap) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_feedback_plan")) return rc;
  if (mode != 0 && mode != 1) return pfail(h, PIADMM_E_ARG, "obca_feedback_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  const size_t N = (size_t)n;
  double nominal[FPAR];
  feedback_row_nominal(nominal);
  if (mode == 1) {
    if (par) {
      if (rows != 1 && rows != n)
        return pfail(h, PIADMM_E_ARG, "obca_feedback_plan: rows must be 1 or n (" + std::to_string(n) + ")");
      for (int k = 0; k < rows; ++k)
        if (const char* why = feedback_row_check(par + (size_t)k * FPAR))
          return pfail(h, PIADMM_E_ARG, "obca_feedback_plan: row " + std::to_string(k) + ": " + why);
    } else {
      par = nominal;
      rows = 1;
    }
    if (tape) {
      if (cap < 0 || cap > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_feedback_plan: 0 <= cap <= 2^20");
      const int64_t bad = first_not_finite(tape, N * (size_t)cap * 10);
      if (bad >= 0)
        return pfail(h, PIADMM_E_ARG, "obca_feedback_plan: the tape of scenario " +
                     std::to_string(bad / ((int64_t)cap * 10)) + " is not finite (step " +
                     std::to_string(bad / 10 % cap) + ")");
    }
    if (p->ck.on)
      return pfail(h, PIADMM_E_STATE, "obca_feedback_plan: a clock is attached (obca_clock_plan: the tape has no per-scenario clocks)");
  }
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_feedback_plan: only at a step boundary (an MPC step is open)");
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  if (mode == 0) {
    feedback_free(p);
    return 0;
  }
  // the new attachment is complete before it replaces the earlier one
  piadmm_obca_plan_s::feedback_s nf;
  const size_t T = N * (size_t)cap * 10;
  hipError_t e = hipMalloc(&nf.par, (size_t)rows * FPAR * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&nf.next, N * 10 * sizeof(double));
  if (e == hipSuccess) e = hipMemset(nf.next, 0, N * 10 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(nf.par, par, (size_t)rows * FPAR * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && tape) {
    // a tape without rows still counts as one: every shift is then refused
    e = hipMalloc(&nf.tape, std::max(T, (size_t)1) * sizeof(double));
    if (e == hipSuccess && T) e = hipMemcpy(nf.tape, tape, T * sizeof(double), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) {
    feedback_free_buffers(nf);
    return pfail(h, PIADMM_E_HIP, std::string("obca_feedback_plan: ") + hipGetErrorString(e));
  }
  feedback_free(p);
  p->fb = nf;
  p->fb.rows = rows;
  p->fb.stride = rows > 1 ? FPAR : 0;
  p->fb.cap = tape ? cap : 0;
  p->fb.steps = 0;
  p->fb.on = true;
  return 0;
}

int32_t piadmm_obca_feedback_measure(piadmm_obca_t h, int32_t m, const int32_t* slots, const double* states) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_feedback_measure")) return rc;
  const int n = p->n;
  if (m < 1 || m > n) return pfail(h, PIADMM_E_ARG, "obca_feedback_measure: 1 <= m <= n_scenarios");
  if (!slots || !states) return pfail(h, PIADMM_E_ARG, "obca_feedback_measure: null argument");
  for (int k = 0; k < m; ++k)
    if (slots[k] < 0 || slots[k] >= n || (k > 0 && slots[k] <= slots[k - 1]))
      return pfail(h, PIADMM_E_ARG, "obca_feedback_measure: slots[" + std::to_string(k) +
                   "] must be a scenario below n, the slots ascending and distinct");
  const int64_t bad = first_not_finite(states, (size_t)m * 10);
  if (bad >= 0)
    return pfail(h, PIADMM_E_ARG, "obca_feedback_measure: state pair " + std::to_string(bad / 10) + " is not finite");
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_feedback_measure: only at a step boundary (an MPC step is open)");
  if (p->tr.on)
    return pfail(h, PIADMM_E_STATE, "obca_feedback_measure: a trace is attached (its last row was computed from the state being replaced)");
  PHIP(h, hipSetDevice(h->device));
  // the states, then the slot numbers, through the staging buffer; one scatter launch
  const size_t body = (size_t)m * 10 * sizeof(double);
  if (int rc = stage_ensure(h, p, body, m)) return rc;
  int* d_list = reinterpret_cast<int*>(p->stg.buf + body);
  PHIP(h, hipMemcpyAsync(p->stg.buf, states, body, hipMemcpyHostToDevice, h->stream));
  PHIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_set_init, dim3(lane_blocks(2 * m)), dim3(64 * PW), 0, h->stream, (const int*)d_list, m,
                     reinterpret_cast<const double*>(p->stg.buf), p->bar, p->barp);
  PHIP(h, hipGetLastError());
  PHIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Device-side disturbance noise (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
namespace {
// One noise row: nullptr when it is good, else what is wrong with it.
const char* noise_row_check(const double* row) {
  using namespace obca_plan;
  for (int i = 0; i < ZPAR; ++i)
    if (!std::isfinite(row[i])) return "every entry finite";
  for (int i = 0; i < 10; ++i)
    if (!(row[Z_SIGMA + i] >= 0.0)) return "sigma >= 0";
  if (!(row[Z_TRUNC] >= 0.0)) return "trunc 0 (none) or > 0";
  if (row[Z_RESERVED] != 0.0) return "the reserved entry must be 0";
  return nullptr;
}

// rows, streams and k0 of both noise calls, on the host
int noise_args_check(piadmm_obca_t h, int n, const double* par, int rows, const int64_t* streams, int32_t k0,
                     int64_t steps, const std::string& who) {
  if (!par) return pfail(h, PIADMM_E_ARG, who + ": null argument");
  if (rows != 1 && rows != n) return pfail(h, PIADMM_E_ARG, who + ": rows must be 1 or n (" + std::to_string(n) + ")");
  for (int k = 0; k < rows; ++k)
    if (const char* why = noise_row_check(par + (size_t)k * obca_plan::ZPAR))
      return pfail(h, PIADMM_E_ARG, who + ": row " + std::to_string(k) + ": " + why);
  if (streams)
    for (int k = 0; k < n; ++k)
      if (streams[k] < 0) return pfail(h, PIADMM_E_ARG, who + ": streams[" + std::to_string(k) + "] must be >= 0");
  if (k0 < 0 || (int64_t)k0 + steps > ((int64_t)1 << 31))
    return pfail(h, PIADMM_E_ARG, who + ": k0 >= 0 and every step index below 2^31");
  return 0;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_noise_tape(piadmm_obca_t h, int32_t n, int32_t cap, const double* par, int32_t rows,
                               const int64_t* streams, uint64_t seed, int32_t k0, double* tape_out, uint32_t* raw_out) {
  using namespace obca_plan;
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_noise_tape: 1 <= n <= 2^20");
  if (cap < 0 || cap > (1 << 20)) return pfail(h, PIADMM_E_ARG, "obca_noise_tape: 0 <= cap <= 2^20");
  const size_t N = (size_t)n, C = (size_t)cap, B = sizeof(double);
  if (N * C * 10 * B >= ((size_t)1 << 31))
    return pfail(h, PIADMM_E_ARG, "obca_noise_tape: n x cap x 80 bytes must stay below 2 GiB");
  if (int rc = noise_args_check(h, n, par, rows, streams, k0, cap, "obca_noise_tape")) return rc;
  if (cap == 0) return 0;
  if (!tape_out) return pfail(h, PIADMM_E_ARG, "obca_noise_tape: null argument");
  PHIP(h, hipSetDevice(h->device));
  // the call's own buffers: neither the handle's local and edge buffers nor an open plan is touched
  double *d_par = nullptr, *d_out = nullptr;
  long long* d_str = nullptr;
  uint32_t* d_raw = nullptr;
  auto run = [&]() -> int {
    if (int rc = dalloc(h, &d_par, (size_t)rows * ZPAR, false)) return rc;
    if (int rc = dalloc(h, &d_out, N * C * 10, false)) return rc;
    if (streams)
      if (int rc = dalloc(h, &d_str, N, false)) return rc;
    if (raw_out)
      if (int rc = dalloc(h, &d_raw, N * C * 24, false)) return rc;
    PHIP(h, hipMemcpyAsync(d_par, par, (size_t)rows * ZPAR * B, hipMemcpyHostToDevice, h->stream));
    if (streams) PHIP(h, hipMemcpyAsync(d_str, streams, N * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    noise_io zo{};
    zo.par = d_par;  zo.par_s = rows > 1 ? ZPAR : 0;
    zo.streams = d_str;
    zo.out_s = (long long)C * 10;  zo.raw_s = (long long)C * 24;
    zo.seed_lo = (uint32_t)seed;  zo.seed_hi = (uint32_t)(seed >> 32);
    // one grid row per step index, at most 32768 rows a launch
    for (int at = 0; at < cap; at += 32768) {
      const int ny = std::min(cap - at, 32768);
      zo.out = d_out + (size_t)at * 10;
      zo.raw = d_raw ? d_raw + (size_t)at * 24 : nullptr;
      zo.k = (uint32_t)k0 + (uint32_t)at;
      hipLaunchKernelGGL(k_plan_noise, dim3(lane_blocks(2 * n), ny), dim3(64 * PW), 0, h->stream, (const int*)nullptr,
                         n, zo);
      PHIP(h, hipGetLastError());
    }
    PHIP(h, hipMemcpyAsync(tape_out, d_out, N * C * 10 * B, hipMemcpyDeviceToHost, h->stream));
    if (raw_out)
      PHIP(h, hipMemcpyAsync(raw_out, d_raw, N * C * 24 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  void* dev[] = {d_par, d_out, d_str, d_raw};
  for (void* q : dev)
    if (q) (void)hipFree(q);
  return rc;
}

int32_t piadmm_obca_noise_plan(piadmm_obca_t h, int32_t mode, const double* par, int32_t rows, const int64_t* streams,
                               uint64_t seed, int32_t k0) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_noise_plan")) return rc;
  if (mode != 0 && mode != 1) return pfail(h, PIADMM_E_ARG, "obca_noise_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  const size_t N = (size_t)n;
  if (mode == 1)
    if (int rc = noise_args_check(h, n, par, rows, streams, k0, 0, "obca_noise_plan")) return rc;
  if (mode == 1 && !p->fb.on)
    return pfail(h, PIADMM_E_STATE, "obca_noise_plan: no feedback attached (obca_feedback_plan: the noise enters through the plant step)");
  if (p->i_iter != 0) return pfail(h, PIADMM_E_STATE, "obca_noise_plan: only at a step boundary (an MPC step is open)");
  PHIP(h, hipSetDevice(h->device));
  PHIP(h, hipStreamSynchronize(h->stream));
  if (mode == 0) {
    noise_free_buffers(p->nz);
    return 0;
  }
  // the new attachment is complete before it replaces the earlier one
  piadmm_obca_plan_s::noise_s nz;
  std::vector<long long> ident;
  if (!streams) {
    ident.resize(N);
    for (size_t k = 0; k < N; ++k) ident[k] = (long long)k;
  }
  const void* src = streams ? static_cast<const void*>(streams) : static_cast<const void*>(ident.data());
  hipError_t e = hipMalloc(&nz.par, (size_t)rows * ZPAR * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&nz.wbuf, N * 10 * sizeof(double));
  if (e == hipSuccess) e = hipMalloc(&nz.streams, N * sizeof(long long));
  if (e == hipSuccess) e = hipMemset(nz.wbuf, 0, N * 10 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(nz.par, par, (size_t)rows * ZPAR * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(nz.streams, src, N * sizeof(long long), hipMemcpyHostToDevice);
  if (e != hipSuccess) {
    noise_free_buffers(nz);
    return pfail(h, PIADMM_E_HIP, std::string("obca_noise_plan: ") + hipGetErrorString(e));
  }
  noise_free_buffers(p->nz);
  p->nz = nz;
  p->nz.rows = rows;
  p->nz.stride = rows > 1 ? ZPAR : 0;
  p->nz.seed = seed;
  p->nz.k0 = k0;
  p->nz.on = true;
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Fleet risk statistics and the worst-case gather (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
namespace {
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

struct stats_out {
  piadmm_obca_stats_t* stats;
  int64_t* hist;
  double* row_min;
  int32_t *row_arg, *row_below, *worst;
};

// what both statistics calls check of their arguments, before any device call
int stats_args_check(piadmm_obca_t h, const std::string& who, int n, const double* edges, int B, int K,
                     const stats_out& o) {
  if (B < 1 || B > PIADMM_OBCA_STATS_EDGES) return pfail(h, PIADMM_E_ARG, who + ": 1 <= B <= 64");
  if (K < 1 || K > PIADMM_OBCA_STATS_WORST || K > n) return pfail(h, PIADMM_E_ARG, who + ": 1 <= K <= min(64, n)");
  if (!edges || !o.stats || !o.hist || !o.row_min || !o.row_arg || !o.row_below || !o.worst)
    return pfail(h, PIADMM_E_ARG, who + ": null argument");
  for (int k = 0; k < B; ++k) {
    if (!std::isfinite(edges[k])) return pfail(h, PIADMM_E_ARG, who + ": edge " + std::to_string(k) + ": not finite");
    if (k > 0 && !(edges[k] > edges[k - 1]))
      return pfail(h, PIADMM_E_ARG, who + ": edge " + std::to_string(k) + ": the edges must be strictly ascending");
  }
  return 0;
}

// The reductions over device arrays (clear (R + 1) x n x 2, summary n x 4, iters R x n, mask
// R x n x 2; the last two are not read for R = 0), on the handle's stream: one workspace for the
// edges, the partial records and the results, one copy of the results back, then into `o`.
int stats_run(piadmm_obca_t h, int R, int n, const double* d_clear, const double* d_summary, const int* d_iters,
              const int* d_mask, const double* edges, int B, int K, const stats_out& o) {
  using namespace obca_plan;
  const size_t rows = (size_t)R + 1, G = ((size_t)n + ST - 1) / ST, Bz = (size_t)B, Kz = (size_t)K;
  // the workspace, every array on a 256-byte boundary; the results first, in the order they go back
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t a = at; at = up256(at + bytes); return a; };
  const size_t o_res = take(sizeof(piadmm_obca_stats_t)), o_hist = take(2 * (Bz + 1) * 8), o_rmin = take(rows * 2 * 8),
               o_rarg = take(rows * 2 * 4), o_rbel = take(rows * 2 * Bz * 4), o_worst = take(Kz * 4);
  const size_t res_bytes = at;
  const size_t o_edges = take(Bz * 8);
  // the fleet's records, then the rows'
  const size_t f_min = take(G * 2 * 8), f_arg = take(G * 2 * 4), f_fin = take(G * 2 * 4), f_bel = take(G * 2 * Bz * 4),
               f_sum = take(G * 8), f_max = take(G * 4), f_or = take(G * 2 * 4), f_flag = take(G * 4);
  const size_t r_min = take(rows * G * 2 * 8), r_arg = take(rows * G * 2 * 4), r_fin = take(rows * G * 2 * 4),
               r_bel = take(rows * G * 2 * Bz * 4);
  // the two list buffers of k_stats_worst
  const size_t w_v[2] = {take(G * Kz * 8), take(G * Kz * 8)}, w_s[2] = {take(G * Kz * 4), take(G * Kz * 4)};
  const size_t total = at;
  char* ws = nullptr;
  std::vector<char> back(res_bytes);
  auto run = [&]() -> int {
    PHIP(h, hipMalloc(reinterpret_cast<void**>(&ws), total));
    auto D = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
    auto I = [&](size_t off) { return reinterpret_cast<int*>(ws + off); };
    PHIP(h, hipMemcpyAsync(ws + o_edges, edges, Bz * 8, hipMemcpyHostToDevice, h->stream));
    const stat_parts FP{D(f_min), I(f_arg), I(f_fin), I(f_bel)}, RP{D(r_min), I(r_arg), I(r_fin), I(r_bel)};
    const fleet_parts FF{reinterpret_cast<long long*>(ws + f_sum), I(f_max), I(f_or), I(f_flag)};
    hipLaunchKernelGGL(k_stats_fleet, dim3((unsigned)G), dim3(ST), 0, h->stream, n, R, d_summary, d_iters, d_mask,
                       (const double*)D(o_edges), B, FP, FF);
    PHIP(h, hipGetLastError());
    hipLaunchKernelGGL(k_stats_fleet_merge, dim3(1), dim3(ST), 0, h->stream, n, R, (int)G, B, FP, FF,
                       reinterpret_cast<piadmm_obca_stats_t*>(ws + o_res), reinterpret_cast<long long*>(ws + o_hist));
    PHIP(h, hipGetLastError());
    hipLaunchKernelGGL(k_stats_rows, dim3((unsigned)rows, (unsigned)G), dim3(ST), 0, h->stream, n, d_clear,
                       (const double*)D(o_edges), B, RP);
    PHIP(h, hipGetLastError());
    hipLaunchKernelGGL(k_stats_rows_merge, dim3((unsigned)rows), dim3(ST), 0, h->stream, (int)G, B, RP, D(o_rmin),
                       I(o_rarg), I(o_rbel));
    PHIP(h, hipGetLastError());
    // the first level reads the summary's plain minima once, ST a workgroup; every further level
    // merges WCAND / K lists a workgroup until one is left
    hipLaunchKernelGGL(k_stats_worst, dim3((unsigned)G), dim3(ST), 0, h->stream, d_summary, (int)TSUM,
                       (const int*)nullptr, n, (int)ST, K, D(w_v[0]), I(w_s[0]));
    PHIP(h, hipGetLastError());
    int cur = 0;
    const int per_lists = WCAND / K;
    for (size_t lists = G; lists > 1; cur ^= 1) {
      const size_t next = (lists + per_lists - 1) / per_lists;
      hipLaunchKernelGGL(k_stats_worst, dim3((unsigned)next), dim3(ST), 0, h->stream, (const double*)D(w_v[cur]), 1,
                         (const int*)I(w_s[cur]), (int)(lists * Kz), per_lists * K, K, D(w_v[cur ^ 1]), I(w_s[cur ^ 1]));
      PHIP(h, hipGetLastError());
      lists = next;
    }
    PHIP(h, hipMemcpyAsync(ws + o_worst, ws + w_s[cur], Kz * 4, hipMemcpyDeviceToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(back.data(), ws, res_bytes, hipMemcpyDeviceToHost, h->stream));
    PHIP(h, hipStreamSynchronize(h->stream));
    return 0;
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  if (ws) (void)hipFree(ws);
  if (rc) return rc;
  std::memcpy(o.stats, back.data() + o_res, sizeof(piadmm_obca_stats_t));
  std::memcpy(o.hist, back.data() + o_hist, 2 * (Bz + 1) * 8);
  std::memcpy(o.row_min, back.data() + o_rmin, rows * 2 * 8);
  std::memcpy(o.row_arg, back.data() + o_rarg, rows * 2 * 4);
  std::memcpy(o.row_below, back.data() + o_rbel, rows * 2 * Bz * 4);
  std::memcpy(o.worst, back.data() + o_worst, Kz * 4);
  return 0;
}

// the offsets of a gathered record's segments, in bytes (include/piadmm.h)
struct gather_layout {
  int64_t states, clear, primal, dual, summary, iters, mask, lamb, bytes;
};
gather_layout gather_offsets(int64_t R, int64_t m, bool lambda) {
  gather_layout g{};
  const int64_t P = R * m;
  g.states = 0;
  g.clear = 80 * (R + 1) * m;
  g.primal = 96 * (R + 1) * m;
  g.dual = g.primal + 8 * P;
  g.summary = g.dual + 8 * P;
  g.iters = g.summary + 32 * m;
  g.mask = g.iters + 4 * P;
  g.lamb = g.mask + 8 * P + ((P & 1) ? 4 : 0);
  g.bytes = g.lamb + (lambda ? 1008 * P : 0);
  return g;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_stats_size(void) { return (int32_t)sizeof(piadmm_obca_stats_t); }

int32_t piadmm_obca_fleet_stats(piadmm_obca_t h, int32_t rows_R, int32_t n, const double* clear, const double* summary,
                                const int32_t* iters, const int32_t* mask, const double* edges, int32_t B, int32_t K,
                                piadmm_obca_stats_t* stats, int64_t* hist, double* row_min, int32_t* row_arg,
                                int32_t* row_below, int32_t* worst) {
  using namespace obca_plan;
  if (!h) return PIADMM_E_ARG;
  const std::string who = "obca_fleet_stats";
  if (n < 1 || n > (1 << 20)) return pfail(h, PIADMM_E_ARG, who + ": 1 <= n <= 2^20");
  if (rows_R < 0 || rows_R > (1 << 20)) return pfail(h, PIADMM_E_ARG, who + ": 0 <= rows_R <= 2^20");
  if (!clear || !summary || (rows_R > 0 && (!iters || !mask))) return pfail(h, PIADMM_E_ARG, who + ": null argument");
  const stats_out o{stats, hist, row_min, row_arg, row_below, worst};
  if (int rc = stats_args_check(h, who, n, edges, B, K, o)) return rc;
  for (int k = 0; k < n; ++k) {
    const double v = summary[(size_t)k * TSUM + 3];
    if (!(v >= 0.0 && v <= 1099511627776.0 && v == std::floor(v)))
      return pfail(h, PIADMM_E_ARG, who + ": row " + std::to_string(k) + ": the sum of iterates must be an integer in [0, 2^40]");
  }
  PHIP(h, hipSetDevice(h->device));
  // the call's own buffers: neither the handle's local and edge buffers nor an open plan is touched
  const size_t N = (size_t)n, R = (size_t)rows_R;
  const size_t b_clear = (R + 1) * N * 2 * 8, b_sum = N * TSUM * 8, b_it = R * N * 4, b_mask = R * N * 2 * 4;
  const size_t o_sum = up256(b_clear), o_it = o_sum + up256(b_sum), o_mask = o_it + up256(b_it);
  char* in = nullptr;
  auto run = [&]() -> int {
    PHIP(h, hipMalloc(reinterpret_cast<void**>(&in), o_mask + up256(b_mask) + 256));
    PHIP(h, hipMemcpyAsync(in, clear, b_clear, hipMemcpyHostToDevice, h->stream));
    PHIP(h, hipMemcpyAsync(in + o_sum, summary, b_sum, hipMemcpyHostToDevice, h->stream));
    if (R) {
      PHIP(h, hipMemcpyAsync(in + o_it, iters, b_it, hipMemcpyHostToDevice, h->stream));
      PHIP(h, hipMemcpyAsync(in + o_mask, mask, b_mask, hipMemcpyHostToDevice, h->stream));
    }
    return stats_run(h, rows_R, n, reinterpret_cast<const double*>(in), reinterpret_cast<const double*>(in + o_sum),
                     reinterpret_cast<const int*>(in + o_it), reinterpret_cast<const int*>(in + o_mask), edges, B, K, o);
  };
  const int rc = run();
  if (rc) (void)hipStreamSynchronize(h->stream);
  if (in) (void)hipFree(in);
  return rc;
}

int32_t piadmm_obca_stats_trace(piadmm_obca_t h, const double* edges, int32_t B, int32_t K, piadmm_obca_stats_t* stats,
                                int64_t* hist, double* row_min, int32_t* row_arg, int32_t* row_below, int32_t* worst) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_trace(h, &p, "obca_stats_trace")) return rc;
  const stats_out o{stats, hist, row_min, row_arg, row_below, worst};
  if (int rc = stats_args_check(h, "obca_stats_trace", p->n, edges, B, K, o)) return rc;
  PHIP(h, hipSetDevice(h->device));
  const auto& t = p->tr;
  return stats_run(h, t.rows, p->n, t.clear, t.summary, t.iters, t.mask, edges, B, K, o);
}

int32_t piadmm_obca_gather_trace_bytes(piadmm_obca_t h, int32_t m, int64_t* bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_trace(h, &p, "obca_gather_trace_bytes")) return rc;
  if (m < 1 || m > p->n) return pfail(h, PIADMM_E_ARG, "obca_gather_trace_bytes: 1 <= m <= n_scenarios");
  if (!bytes) return pfail(h, PIADMM_E_ARG, "obca_gather_trace_bytes: null argument");
  *bytes = gather_offsets(p->tr.rows, m, p->tr.lamb != nullptr).bytes;
  return 0;
}

int32_t piadmm_obca_gather_trace(piadmm_obca_t h, int32_t m, const int32_t* slots, void* blob, int64_t bytes) {
  using namespace obca_plan;
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_trace(h, &p, "obca_gather_trace")) return rc;
  if (int rc = tenant_slots_check(h, p, m, slots, blob, "obca_gather_trace")) return rc;
  const auto& t = p->tr;
  const gather_layout g = gather_offsets(t.rows, m, t.lamb != nullptr);
  if (bytes != g.bytes)
    return pfail(h, PIADMM_E_ARG, "obca_gather_trace: the blob is " + std::to_string(g.bytes) + " bytes, not " +
                 std::to_string(bytes));
  const int64_t waves = ((int64_t)t.rows + 1) * m, blocks = (waves + PW - 1) / PW;
  if (blocks > INT_MAX) return pfail(h, PIADMM_E_ARG, "obca_gather_trace: (rows + 1) m must stay below 2^33");
  PHIP(h, hipSetDevice(h->device));
  if (int rc = stage_ensure(h, p, (size_t)g.bytes, m)) return rc;
  char* st = p->stg.buf;
  int* d_list = reinterpret_cast<int*>(st + g.bytes);
  auto D = [&](int64_t off) { return reinterpret_cast<double*>(st + off); };
  const gather_src a{t.states, t.clear, t.primal, t.dual, t.lamb, t.summary, t.iters, t.mask};
  const gather_dst d{D(g.states), D(g.clear), D(g.primal), D(g.dual), D(g.summary), D(g.lamb),
                     reinterpret_cast<int*>(st + g.iters), reinterpret_cast<int*>(st + g.mask)};
  PHIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  // the pad word between STATUS_MASK and LAMBDA has no writer: it goes out as 0
  if (g.lamb != g.mask + 8 * (int64_t)t.rows * m) PHIP(h, hipMemsetAsync(st + g.lamb - 4, 0, 4, h->stream));
  hipLaunchKernelGGL(k_trace_gather, dim3((unsigned)blocks), dim3(64 * PW), 0, h->stream, (const int*)d_list, m, p->n,
                     t.rows + 1, a, d);
  PHIP(h, hipGetLastError());
  PHIP(h, hipMemcpyAsync(blob, st, (size_t)g.bytes, hipMemcpyDeviceToHost, h->stream));
  PHIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
