// piadmm_obca_plan.h -- what the units of the device-resident OBCA-ADMM consensus loop share
// (internal, not installed): the layouts, the kernel-argument structs, the owners of device memory,
// the plan and the small host helpers.  csrc/piadmm_obca_plan.hip holds the iterate and the shift and
// describes the launch sequence; csrc/piadmm_obca_plan_{attach,trace,tenant,feedback,delay,loop,ledger}.hip hold
// the attachments.  Every kernel is defined in one unit; there is no relocatable device code, a unit
// launches another unit's kernel through the declaration here.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <string>
#include <utility>
#include <vector>

#include "pd_common.h"
#include "pd_obca.h"
#include "pd_owners.h"
#include "piadmm.h"
#include "piadmm_obca_handle.h"

namespace obca_plan {

using namespace pd_obca;     // NT, the vehicle constants, the record layouts R_*, O_*, E_*, EO_*
constexpr int PW = 4;                          // waves per workgroup
constexpr int STATE = PIADMM_OBCA_PLAN_STATE;
constexpr int REC = PIADMM_OBCA_REC, OUT = PIADMM_OBCA_OUT;
constexpr int EREC = PIADMM_OBCA_EDGE_REC, EOUT = PIADMM_OBCA_EDGE_OUT;
// the state's fields (include/piadmm.h)
constexpr int S_ZB = 0, S_A = 126, S_B = 238, S_LB = 294, S_LIJ = 420, S_LX = 476, S_INIT = 546;
static_assert(S_INIT + 10 == STATE, "state layout");
constexpr int NCTRL = 28, NX = 80;

// a parameter row (include/piadmm.h): the integers are stored as doubles, as the records do
constexpr int TAB = PIADMM_OBCA_FLEET_PAR;
constexpr int T_RHO = 0, T_MIN_DIS = 1, T_CONV = 2, T_MAX_X = 3, T_MAX_Y = 4, T_R = 5, T_Q = 6, T_XB = 7,
              T_MU = 8, T_G = 9, T_ADMM = 10, T_SQP = 11, T_ROUND = 12, T_START = 13;
static_assert(T_START < TAB, "row layout");

constexpr int CT = 256;              // the one workgroup of k_plan_compact
// a gains row of the dual law (include/piadmm.h)
constexpr int DPAR = PIADMM_OBCA_DUAL_PAR;
constexpr int G_KP = 0, G_KI = 1, G_SAT = 2, G_DGAIN = 3, G_WINDUP = 4;
static_assert(G_WINDUP < DPAR, "gains row layout");
constexpr int TSUM = 4;     // summary per scenario: min plain clearance, its row, min tightened clearance, sum of iterates
constexpr int WIN = 2 * 8 * 5;       // a window: ref_s[v][c .. c + 7], the 80 doubles k_plan_pack_local reads
// a plant row (include/piadmm.h): 8 doubles per vehicle, vehicle 0 first
constexpr int FPAR = PIADMM_OBCA_FEEDBACK_PAR, FV = FPAR / 2;
constexpr int F_METHOD = 0, F_NSUB = 1, F_LR = 2, F_LF = 3, F_GA = 4, F_GW = 5, F_AMAX = 6, F_WMAX = 7;
constexpr int F_NSUB_MAX = 64;
constexpr double PLANT_DT = 0.1, MAX_STEER = 0.6;
static_assert(F_WMAX + 1 == FV && FV % 2 == 0, "plant row layout");
// a noise row (include/piadmm.h): sigma[2][5], bias[2][5], trunc, one reserved zero
constexpr int ZPAR = PIADMM_OBCA_NOISE_PAR;
constexpr int Z_SIGMA = 0, Z_BIAS = 10, Z_TRUNC = 20, Z_RESERVED = 21;
static_assert(Z_RESERVED + 1 == ZPAR, "noise row layout");
// a delay row (include/piadmm.h): avg[2], std[2], tau_max[2], trunc, one reserved zero
constexpr int YPAR = PIADMM_OBCA_DELAY_PAR;
constexpr int Y_AVG = 0, Y_STD = 2, Y_TMAX = 4, Y_TRUNC = 6, Y_RESERVED = 7;
static_assert(Y_RESERVED + 1 == YPAR, "delay row layout");

// a ledger record (include/piadmm.h): 22 words of 8 bytes
constexpr int LREC = PIADMM_OBCA_LEDGER_REC / 8;
constexpr int L_ID = 0, L_STREAM = 1, L_SLOT = 2, L_FIRST = 3, L_PLAIN = 4, L_TIGHT = 5, L_CMIN = 6, L_SUM = 7, L_MASK = 8,
              L_PRIMAL = 9, L_DUAL = 10, L_TSTEP = 11, L_STATE = 12;
static_assert(L_STATE + 10 == LREC && PIADMM_OBCA_LEDGER_REC % 8 == 0, "ledger record layout");
constexpr int LVIEW = 11;            // the words of the statistics' view per record: summary 4, clear 2 x 2, iters 1, mask 2

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

// where the arrays of one k_plan_delay launch sit, indexed by scenario: par the delay rows (par_s =
// 0: one shared row), streams the stream ids (nullptr: the scenario's number), tape the recorded
// latencies added in front (nullptr: none), out the latencies, raw the Philox words (nullptr: not
// kept); the strides in elements per scenario, and per step index (blockIdx.y) 2 doubles of tape and
// out and 8 words of raw; k = the step index of blockIdx.y = 0
struct delay_io {
  const double *par, *tape;
  const long long* streams;
  double* out;
  uint32_t* raw;
  long long tape_s, out_s, raw_s;
  uint32_t seed_lo, seed_hi, k;
  int par_s;
};

// where the arrays of the loop's launches sit (piadmm_obca_loop_plan), indexed by scenario: plant,
// noise and delay the rows (a stride 0: one shared row; noise / delay nullptr: that kind is absent),
// streams the stream ids (nullptr: the scenario's number), clk the clocks (c, len, alive; the step
// index of scenario s is k0 + clk[3 s]), x0 and ctrl what k_plan_propagate reads of the plan, next
// the closing states by list position (m x 10), tau the latencies (n x 2)
struct loop_io {
  const double *plant, *noise, *delay, *x0, *ctrl;
  const long long* streams;
  const int* clk;
  double *next, *tau;
  int plant_s, noise_s, delay_s;
  uint32_t seed_lo, seed_hi, k0;
};

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

// The state a vehicle's message describes when it arrives tau late: x1 = X[t + 1] is what the
// vehicle plans for the slot, x0 = X[t] where it planned to be one step earlier.  tau == 0 is x1 bit
// for bit; otherwise x1 + (tau / DT) (x0 - x1), all five entries, the heading linearly.
// piadmm.obca.stale_states is the same statements on the host; products and sums are kept apart, and
// every operation is exact IEEE arithmetic, so the two agree bit for bit.  The body of the plan's
// stale exchange and of the stand-alone k_delay_exchange.
__device__ __forceinline__ void stale_state(const double* x0, const double* x1, double tau, double st[5]) {
#pragma clang fp contract(off)
  if (tau == 0.0) {
#pragma unroll
    for (int j = 0; j < 5; ++j) st[j] = x1[j];
  } else {
    const double f = tau / PLANT_DT;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
      const double a = x1[j];
      st[j] = a + f * (x0[j] - a);
    }
  }
}

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

// One plant step of one vehicle, all in registers: x (5) <- F(x, (a, om)) under the vehicle's row P
// (8), without the disturbance.  n_sub substeps of DT / n_sub; a substep is 1 stage (Euler) or 4
// (classical RK4) of the one right-hand side below, the stage loop kept rolled so that the libm
// calls are inlined once; then delta is clipped.  n_sub is clamped to its range, so the loop is
// bounded whatever the row holds.  piadmm.obca.propagate is the same statements on the host;
// products and sums are kept apart (no contraction).  The body of
// k_plan_propagate (the stand-alone call and the in-plan step) and of k_loop_close: the same bits.
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

// The five disturbances of vehicle v of stream t at step k under the row's sigma S, bias B and
// trunc: three Philox calls at counter (k, 4 v + j, t low, t high), each giving two uniforms in
// (0, 1) on 52 bits and by Box-Muller two normals; the sixth normal is discarded.  raw (12 words,
// or nullptr) receives the calls' words.  piadmm.obca.noise_tape is the same statements on the
// host; products and sums are kept apart (no contraction), so sigma = 0 gives the bias bit for bit.
// The body of k_plan_noise (the in-plan step and the stand-alone tape) and of k_loop_close and
// k_loop_draw: the same bits.
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

// The latency of vehicle v of stream t at step k under the row's avg, std, tau_max and trunc: one
// Philox call at counter (k, 4 v + 3, t low, t high) -- the call index the noise leaves free -- two
// uniforms in (0, 1) on 52 bits as noise_draw forms them, the first Box-Muller normal; the second is
// discarded.  tape is the recorded latency added in front (0 without one).  raw (4 words, or
// nullptr) receives the call's words.  piadmm.obca.delay_tau is the same statements on the host;
// products and sums are kept apart (no contraction), so std = 0 gives min(tau_max, tape + avg) bit
// for bit.  The body of k_plan_delay (the in-plan step and the stand-alone call), of k_loop_open and
// of k_loop_draw: the same bits.
__device__ __forceinline__ double delay_draw(uint32_t seed_lo, uint32_t seed_hi, uint32_t t_lo, uint32_t t_hi,
                                             uint32_t k, int v, double avg, double sd, double tau_max, double trunc,
                                             double tape, uint32_t* raw) {
#pragma clang fp contract(off)
  uint32_t c[4] = {k, (uint32_t)(4 * v + 3), t_lo, t_hi};
  philox4x32_10(c, seed_lo, seed_hi);
  if (raw) {
#pragma unroll
    for (int q = 0; q < 4; ++q) raw[q] = c[q];
  }
  const unsigned long long a = ((unsigned long long)c[0] << 32) | c[1];
  const unsigned long long b = ((unsigned long long)c[2] << 32) | c[3];
  const double u1 = ((double)(a >> 12) + 0.5) * 0x1p-52;
  const double u2 = ((double)(b >> 12) + 0.5) * 0x1p-52;
  const double rad = sqrt(-2.0 * log(u1));
  const double ang = 6.283185307179586 * u2;
  double z = rad * cos(ang);
  if (trunc != 0.0) z = fmin(trunc, fmax(z, -trunc));
  const double x = tape + (avg + sd * z);
  const double lo = x > 0.0 ? x : 0.0;
  return lo < tau_max ? lo : tau_max;
}

// The exact minimum distance between the two vehicles' rectangles (generate_vehicle_vertices,
// util.py:34-42) at the state pair st[2][5], for two box sets at once: the plain boxes (centre x, y)
// and the delay-tightened ones the planner constrains (compute_square_halfspaces_ca_prob,
// util.py:70-101: each centre moved as halfspaces() above moves it; pr = 0 moves nothing, so both
// results are the plain value).  The distance is 0 when no edge normal of either rectangle separates
// them (SAT over the 4 axes), else the minimum of the 32 vertex-to-edge distances.  Lane = set * 32 +
// dir * 16 + vertex * 4 + edge: a vertex of vehicle `dir` against an edge of the other vehicle, whose
// normal (edge & 1: the lateral one) is the lane's SAT axis.  Every lane of the wave must be here (the
// reductions are DPP scans over the whole wave) and st, pr are wave-uniform; plain and tight come back
// uniform.  piadmm.obca.clearance is the same statements on the host; products and sums are kept
// apart (no contraction).  The body of k_plan_clearance and of the ledger's k_ledger_open and
// k_ledger_step: the same bits.
__device__ __forceinline__ void clearance_pair(const double* st, int pr, double sigd, int lane, double& plain,
                                               double& tight) {
#pragma clang fp contract(off)
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
  plain = g0 > 0.0 ? d0 : 0.0;
  tight = g1 > 0.0 ? d1 : 0.0;
}

// The kernels launched from a unit other than their own (the comments are at the definitions).
// csrc/piadmm_obca_plan.hip
__global__ void __launch_bounds__(CT) k_plan_compact(const int* __restrict__ active, const int* __restrict__ keep,
                                                     int n_act, int* __restrict__ next, int* __restrict__ count);
__global__ void __launch_bounds__(64) k_plan_shift_list(const int* __restrict__ list, int m,
                                                        double* __restrict__ bar, double* __restrict__ barp,
                                                        const double* __restrict__ X, double* __restrict__ lamb,
                                                        double* __restrict__ ctrlp);
// csrc/piadmm_obca_plan_attach.hip
__global__ void __launch_bounds__(64 * PW) k_plan_dual_pi(const int* __restrict__ active, int n_act,
                                                          const double* __restrict__ erecs,
                                                          double* __restrict__ eout, const int* __restrict__ eist,
                                                          const double* __restrict__ gains, int g_stride,
                                                          double* __restrict__ S, double* __restrict__ D,
                                                          double* __restrict__ Sp, double* __restrict__ Dp);
__global__ void __launch_bounds__(64) k_plan_dual_shift(int n, double* __restrict__ S, double* __restrict__ D,
                                                        double* __restrict__ Sp, double* __restrict__ Dp);
__global__ void __launch_bounds__(64 * PW) k_plan_work(const int* __restrict__ active, int n_act,
                                                       const int* __restrict__ list, const int* __restrict__ eist,
                                                       int* __restrict__ work);
__global__ void __launch_bounds__(64 * PW) k_plan_order(const int* __restrict__ list_in,
                                                        const int* __restrict__ count, int m,
                                                        const int* __restrict__ work, int* __restrict__ list_out);
// csrc/piadmm_obca_plan_feedback.hip
__global__ void __launch_bounds__(64 * PW) k_plan_propagate(const int* __restrict__ list, int m, plant_io io);
__global__ void __launch_bounds__(64 * PW) k_plan_set_init(const int* __restrict__ list, int m,
                                                           const double* __restrict__ states,
                                                           double* __restrict__ bar, double* __restrict__ barp);
__global__ void __launch_bounds__(64 * PW) k_plan_noise(const int* __restrict__ list, int m, noise_io io);
// csrc/piadmm_obca_plan_delay.hip
__global__ void __launch_bounds__(64 * PW) k_plan_delay(const int* __restrict__ list, int m, delay_io io);
// csrc/piadmm_obca_plan_loop.hip
__global__ void __launch_bounds__(64 * PW) k_loop_close(const int* __restrict__ list, int m, loop_io io);
__global__ void __launch_bounds__(64 * PW) k_loop_open(const int* __restrict__ list, int m, loop_io io);

// ---------------------------------------------------------------------------------------------
// The host side
// ---------------------------------------------------------------------------------------------
// The owners of device memory (pd_owners.h).  scratch: the device arrays of one stand-alone call, on
// the stack: neither the handle's local and edge buffers nor an open plan is touched.
using pd_own::dev_buf;
using scratch = pd_own::arena<piadmm_obca_s>;

}  // namespace obca_plan

// The plan.  Every array is owned: detaching a feature is assigning a fresh one of its struct
// (p->tr = {}), and an attach builds its struct in a local and moves it in once it is complete, so
// a failure on the way releases the local and leaves the attached one as it was.
struct piadmm_obca_plan_s {
  template <typename T>
  using dbuf = obca_plan::dev_buf<T>;
  piadmm_obca_plan_cfg_t cfg{};
  bool open = false;
  int n = 0, t_step = 0, i_iter = 0, n_act = 0, n_last = 0, cur = 0;
  // the parameter rows and the references: rows = 1 with stride 0 (piadmm_obca_plan_begin) or
  // rows = n (piadmm_obca_fleet_begin); max_iter_all = the largest max_admm_iter of the rows
  int tab_rows = 0, ref_rows = 0, tab_stride = 0, ref_stride = 0, max_iter_all = 0;
  double sigd = 0.0;
  dbuf<double> bar, barp, ctrl, ctrlp, X, primal, dual, pth, dth, ref, lamb, tab;
  dbuf<int> iters, stop, conv, prob, act[2], keep, count, mask;
  obca_plan::dev_buf<int, true> h_count;        // pinned: the 4 bytes read back per iterate
  // the run record (piadmm_obca_trace_begin): rows = MPC steps recorded, row-major over steps.
  // states / clear hold cap + 1 rows (row 0: where the trace was attached), the rest cap.
  struct trace_s {
    bool on = false;
    int cap = 0, rows = 0, flags = 0;
    dbuf<double> states, clear, primal, dual, lamb, summary;
    dbuf<int> iters, mask;
  } tr;
  // the PI anti-windup dual law (piadmm_obca_dual_plan): rows = 1 with stride 0 or n gains rows;
  // the integrator S, D and the previous iterate's copy of each, n x 126
  struct dual_s {
    bool on = false;
    int rows = 0, stride = 0;
    dbuf<double> par, S, D, Sp, Dp;
  } du;
  // the longest-first order (piadmm_obca_order_plan): work = (Q, I) per scenario, n x 2; tmp = the
  // unsorted list k_plan_compact / k_plan_shift write and k_plan_order reads, n ints
  struct order_s {
    bool on = false;
    dbuf<int> work, tmp;
  } ord;
  // the per-scenario clocks (piadmm_obca_clock_plan): clk = (c, len, alive) per scenario, n x 3, and
  // `host` its mirror; win = the reference windows, n x 80; flag[cur] = the alive flags (the next
  // tick's `ran`), flag[1 - cur] the ones the next tick writes; list = the n_list scenarios alive
  // when the open step opened, ascending (the active lists are overwritten as the step iterates);
  // ident = 0 .. n - 1, the list k_plan_compact filters by the flags
  struct clock_s {
    bool on = false;
    int cur = 0, n_list = 0;
    dbuf<int> clk, flag[2], list, ident;
    dbuf<double> win;
    std::vector<int> host;
  } ck;
  std::vector<int> admm_rows;    // max_admm_iter of every parameter row (max_iter_all is their maximum)
  // the closed-loop feedback (piadmm_obca_feedback_plan): rows = 1 with stride 0 or n plant rows; tape
  // = cap disturbance rows per scenario (nullptr: none), n x cap x 10; steps = the shifts since the
  // attachment (the tape row the next shift adds); next = the states the plant reached, n x 10
  struct feedback_s {
    bool on = false;
    int rows = 0, stride = 0, cap = 0, steps = 0;
    dbuf<double> par, tape, next;
  } fb;
  // the device-side noise on top of the feedback (piadmm_obca_noise_plan): rows = 1 with stride 0 or n
  // noise rows; streams = the stream id of every scenario; wbuf = the disturbance rows of the step
  // that closes, n x 10, which k_plan_noise writes and k_plan_propagate reads; the step index of a
  // shift is k0 + fb.steps
  struct noise_s {
    bool on = false;
    int rows = 0, stride = 0, k0 = 0;
    uint64_t seed = 0;
    dbuf<double> par, wbuf;
    dbuf<long long> streams;
  } nz;
  // the communication delay of the exchange (piadmm_obca_delay_plan): rows = 1 with stride 0 or n
  // delay rows; streams = the stream id of every scenario; tape = cap recorded latencies per scenario
  // (nullptr: none), n x cap x 2; steps = the shifts since the attachment; tau = the open step's
  // latencies, n x 2, which k_plan_delay writes at the attachment and after every shift and
  // k_plan_exchange_stale reads; the open step's index is k0 + steps
  struct delay_s {
    bool on = false;
    int rows = 0, stride = 0, k0 = 0, cap = 0, steps = 0;
    uint64_t seed = 0;
    dbuf<double> par, tape, tau;
    dbuf<long long> streams;
  } dl;
  // the loop (piadmm_obca_loop_plan): the closed loop of a clocked plan, its step index each tenant's
  // own clock.  flags = 1 (on) + 2 (noise rows) + 4 (delay rows); of each kind rows = 1 with stride 0
  // or n; streams = the stream id of every scenario; tau = the open step's latencies, n x 2 (zeros
  // without delay rows), which k_loop_open writes and k_plan_exchange_stale reads; next = the states
  // the plant reached, by position in ck.list; the step index of scenario s is k0 + its clock
  struct loop_s {
    bool on = false;
    int flags = 0, k0 = 0, plant_rows = 0, noise_rows = 0, delay_rows = 0;
    uint64_t seed = 0;
    dbuf<double> plant, noise, delay, tau, next;
    dbuf<long long> streams;
  } lp;
  // the tenant ledger (piadmm_obca_ledger_begin): rec = the appended records, cap x 22 words; run = the
  // open record of every slot, n x 22; list / pos / ids = what an admission uploads for k_ledger_close and
  // k_ledger_open, n each; view = the statistics' R = 1 view, grown on demand.  The host mirrors what
  // decides a position: count, next_id and per slot the tenant's id (-1: none) and c_first
  struct ledger_s {
    bool on = false;
    int cap = 0, count = 0;
    long long next_id = 0;
    dbuf<long long> rec, run, ids;
    dbuf<int> list, pos;
    dbuf<char> view;
    size_t view_cap = 0;
    std::vector<long long> id;
    std::vector<int> c_first;
  } lg;
  // the staging buffer of piadmm_obca_tenant_export / _import: the records, then the slot list; grown on demand
  struct stage_s {
    dbuf<char> buf;
    size_t cap = 0;
  } stg;
};

namespace obca_plan {

inline int open_plan(piadmm_obca_t h, piadmm_obca_plan_s** out, const char* who) {
  if (!h) return PIADMM_E_ARG;
  if (!h->plan || !h->plan->open) return fail(h, PIADMM_E_STATE, std::string(who) + ": no open plan (obca_plan_begin)");
  *out = h->plan;
  return 0;
}
inline int open_trace(piadmm_obca_t h, piadmm_obca_plan_s** out, const char* who) {
  if (int rc = open_plan(h, out, who)) return rc;
  if (!(*out)->tr.on) return fail(h, PIADMM_E_STATE, std::string(who) + ": no trace attached (obca_trace_begin)");
  return 0;
}

inline std::vector<int> identity_list(size_t n) {      // 0 .. n - 1
  std::vector<int> v(n);
  std::iota(v.begin(), v.end(), 0);
  return v;
}
inline int blocks_for(int waves) { return (waves + PW - 1) / PW; }
// workgroups of 64 * PW lanes for a kernel that runs one lane per item
inline int lane_blocks(int lanes) { return (lanes + 64 * PW - 1) / (64 * PW); }
// true when the attached feedback has a tape and the next `steps` shifts do not fit what is left of it
inline bool feedback_exhausted(const piadmm_obca_plan_s* p, int64_t steps) {
  return p->fb.on && p->fb.tape && (int64_t)p->fb.steps + steps > p->fb.cap;
}
// true when the attached noise would pass step index 2^31 - 1 within the next `steps` shifts
inline bool noise_exhausted(const piadmm_obca_plan_s* p, int64_t steps) {
  return p->nz.on && (int64_t)p->nz.k0 + p->fb.steps + steps > ((int64_t)1 << 31);
}

// What refuses the next `steps` MPC steps of a plan with the delay attached, or nullptr: step k since
// the attachment needs its tape row (k < cap with a tape) and a step index k0 + k below 2^31
inline const char* delay_refusal(const piadmm_obca_plan_s* p, int64_t steps) {
  if (!p->dl.on) return nullptr;
  if (p->dl.tape && (int64_t)p->dl.steps + steps > p->dl.cap) return "latency tape exhausted";
  if ((int64_t)p->dl.k0 + p->dl.steps + steps > ((int64_t)1 << 31)) return "delay step index exhausted";
  return nullptr;
}

// the launch arguments of the loop `l` on the plan's own arrays
inline loop_io loop_view(const piadmm_obca_plan_s* p, const piadmm_obca_plan_s::loop_s& l) {
  loop_io io{};
  io.plant = l.plant;  io.plant_s = l.plant_rows > 1 ? FPAR : 0;
  io.noise = (l.flags & 2) ? l.noise.get() : nullptr;  io.noise_s = l.noise_rows > 1 ? ZPAR : 0;
  io.delay = (l.flags & 4) ? l.delay.get() : nullptr;  io.delay_s = l.delay_rows > 1 ? YPAR : 0;
  io.streams = l.streams;
  io.clk = p->ck.clk;
  io.x0 = p->bar + S_INIT;
  io.ctrl = p->ctrl;
  io.next = l.next;
  io.tau = l.tau;
  io.seed_lo = (uint32_t)l.seed;  io.seed_hi = (uint32_t)(l.seed >> 32);
  io.k0 = (uint32_t)l.k0;
  return io;
}
// true when, with the loop attached, the next `steps` MPC steps would take an alive tenant's step
// index k0 + c to 2^31 (a tenant ticks at most until it retires)
inline bool loop_exhausted(const piadmm_obca_plan_s* p, int64_t steps) {
  if (!p->lp.on || !p->ck.on) return false;
  for (int s = 0; s < p->n; ++s) {
    const int* k = p->ck.host.data() + 3 * (size_t)s;
    if (!k[2]) continue;
    const int64_t ticks = std::min<int64_t>(steps, (int64_t)k[1] - 8 - k[0] + 1);
    if ((int64_t)p->lp.k0 + k[0] + ticks >= ((int64_t)1 << 31)) return true;
  }
  return false;
}

// The checks more than one call makes, each worded once; `who` is the call's name.
// list[0 .. m) (`item`: what the call names it) holds distinct scenarios below n
inline int slots_check(piadmm_obca_t h, const std::string& who, const char* item, const int32_t* list, int m, int n) {
  std::vector<char> seen((size_t)n, 0);
  for (int k = 0; k < m; ++k) {
    if (list[k] < 0 || list[k] >= n || seen[(size_t)list[k]])
      return fail(h, PIADMM_E_ARG, who + ": " + item + "[" + std::to_string(k) + "] must be a scenario below n, listed once");
    seen[(size_t)list[k]] = 1;
  }
  return 0;
}
// m, the pointers and the slots of an export, an import or a gather
inline int tenant_slots_check(piadmm_obca_t h, const piadmm_obca_plan_s* p, int m, const int32_t* slots,
                              const void* blob, const std::string& who) {
  if (m < 1 || m > p->n) return fail(h, PIADMM_E_ARG, who + ": 1 <= m <= n_scenarios");
  if (!slots || !blob) return fail(h, PIADMM_E_ARG, who + ": null argument (slots, blob)");
  return slots_check(h, who, "slots", slots, m, p->n);
}
inline int prob_check(piadmm_obca_t h, const std::string& who, const int32_t* prob, int k) {
  if (prob[k] != 0 && prob[k] != 1) return fail(h, PIADMM_E_ARG, who + ": prob[" + std::to_string(k) + "] must be 0 or 1");
  return 0;
}
inline int rows_check(piadmm_obca_t h, const std::string& who, int rows, int n) {
  if (rows != 1 && rows != n) return fail(h, PIADMM_E_ARG, who + ": rows must be 1 or n (" + std::to_string(n) + ")");
  return 0;
}
// The tail of a _get call: item `what` is `want` bytes at src, on the host (`host`) or on the device.
inline int get_finish(piadmm_obca_t h, const std::string& who, int what, const void* src, bool host, int64_t want,
                      void* out, int64_t bytes) {
  if (bytes != want)
    return fail(h, PIADMM_E_ARG, who + ": item " + std::to_string(what) + " is " + std::to_string(want) +
                " bytes, not " + std::to_string(bytes));
  if (want == 0) return 0;
  if (!out) return fail(h, PIADMM_E_ARG, who + ": out");
  if (host) {
    std::memcpy(out, src, (size_t)want);
    return 0;
  }
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipMemcpyAsync(out, src, (size_t)want, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

// csrc/piadmm_obca_plan.hip
const char* row_check(const double* row);
int stage_ensure(piadmm_obca_t h, piadmm_obca_plan_s* p, size_t bytes, int m);
// csrc/piadmm_obca_plan_attach.hip
const char* dual_row_check(const double* row);
int clock_lists(piadmm_obca_t h, piadmm_obca_plan_s* p, const int* ran, int dst, int n_alive);
int clock_shift(piadmm_obca_t h, piadmm_obca_plan_s* p);
int clock_relist(piadmm_obca_t h, piadmm_obca_plan_s* p);
// csrc/piadmm_obca_plan_feedback.hip
const char* feedback_row_check(const double* row);
void feedback_row_nominal(double* row);
const char* noise_row_check(const double* row);
// csrc/piadmm_obca_plan_delay.hip
const char* delay_row_check(const double* row);
int delay_next(piadmm_obca_t h, piadmm_obca_plan_s* p);
// csrc/piadmm_obca_plan_loop.hip
int loop_close(piadmm_obca_t h, piadmm_obca_plan_s* p);
int loop_set_init(piadmm_obca_t h, piadmm_obca_plan_s* p);
int loop_open(piadmm_obca_t h, piadmm_obca_plan_s* p, int m);
// csrc/piadmm_obca_plan_trace.hip
int trace_append(piadmm_obca_t h, piadmm_obca_plan_s* p, int row);
struct stats_out {
  piadmm_obca_stats_t* stats;
  int64_t* hist;
  double* row_min;
  int32_t *row_arg, *row_below, *worst;
};
int stats_args_check(piadmm_obca_t h, const std::string& who, int n, const double* edges, int B, int K,
                     const stats_out& o);
int stats_run(piadmm_obca_t h, int R, int n, const double* d_clear, const double* d_summary, const int* d_iters,
              const int* d_mask, const double* edges, int B, int K, const stats_out& o);
// csrc/piadmm_obca_plan_ledger.hip
const char* ledger_refusal(const piadmm_obca_plan_s* p, int64_t steps);
int ledger_step(piadmm_obca_t h, piadmm_obca_plan_s* p);
void ledger_stepped(piadmm_obca_plan_s* p, const std::vector<int>& next);
const char* ledger_replace_refusal(const piadmm_obca_plan_s* p, int m, const int32_t* slots, bool fresh_only);
int ledger_close(piadmm_obca_t h, piadmm_obca_plan_s* p, int m, const int32_t* slots, int reason, bool fresh_only);
int ledger_open(piadmm_obca_t h, piadmm_obca_plan_s* p, int m, const int32_t* slots);

}  // namespace obca_plan
