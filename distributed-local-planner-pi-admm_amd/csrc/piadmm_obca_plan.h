// piadmm_obca_plan.h -- what the units of the device-resident OBCA-ADMM consensus loop share
// (internal, not installed): the layouts, the kernel-argument structs, the owners of device memory,
// the plan and the small host helpers.  csrc/piadmm_obca_plan.hip holds the iterate and the shift and
// describes the launch sequence; csrc/piadmm_obca_plan_{attach,trace,tenant,feedback,delay,loop,ledger}.hip hold
// the attachments.  csrc/piadmm_obca_plan_draw.h, included below, holds what the closed loop (feedback,
// noise, delay, loop) shares: the plant step, the draws, their launch views and argument checks.
// Every kernel is defined in one unit; there is no relocatable device code, a unit launches another
// unit's kernel through the declaration here.
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
inline int blocks_for(int waves) { return (waves + PW - 1) / PW; }
// workgroups of 64 * PW lanes for a kernel that runs one lane per item
inline int lane_blocks(int lanes) { return (lanes + 64 * PW - 1) / (64 * PW); }
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
  // the device-side noise on top of the feedback (piadmm_obca_noise_plan): rows = 1 (shared) or n
  // noise rows; streams = the stream id of every scenario; wbuf = the disturbance rows of the step
  // that closes, n x 10, which k_plan_noise writes and k_plan_propagate reads; the step index of a
  // shift is k0 + fb.steps
  struct noise_s {
    bool on = false;
    int rows = 0, k0 = 0;
    uint64_t seed = 0;
    dbuf<double> par, wbuf;
    dbuf<long long> streams;
  } nz;
  // the communication delay of the exchange (piadmm_obca_delay_plan): rows = 1 (shared) or n
  // delay rows; streams = the stream id of every scenario; tape = cap recorded latencies per scenario
  // (nullptr: none), n x cap x 2; steps = the shifts since the attachment; tau = the open step's
  // latencies, n x 2, which k_plan_delay writes at the attachment and after every shift and
  // k_plan_exchange_stale reads; the open step's index is k0 + steps
  struct delay_s {
    bool on = false;
    int rows = 0, k0 = 0, cap = 0, steps = 0;
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

// what the closed loop shares: the plant step, the draws, their launch views and argument checks
#include "piadmm_obca_plan_draw.h"

namespace obca_plan {

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
__global__ void __launch_bounds__(64 * PW) k_plan_noise(const int* __restrict__ list, int m, draw_io io);
// csrc/piadmm_obca_plan_delay.hip
__global__ void __launch_bounds__(64 * PW) k_plan_delay(const int* __restrict__ list, int m, draw_io io);
// csrc/piadmm_obca_plan_loop.hip
__global__ void __launch_bounds__(64 * PW) k_loop_close(const int* __restrict__ list, int m, loop_io io);
__global__ void __launch_bounds__(64 * PW) k_loop_open(const int* __restrict__ list, int m, loop_io io);

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
// true when the attached feedback has a tape and the next `steps` shifts do not fit what is left of it
inline bool feedback_exhausted(const piadmm_obca_plan_s* p, int64_t steps) {
  return p->fb.on && p->fb.tape && (int64_t)p->fb.steps + steps > p->fb.cap;
}

// What refuses the next `steps` MPC steps of a plan with the delay attached, or nullptr: step k since
// the attachment needs its tape row (k < cap with a tape) and a step index k0 + k below 2^31
inline const char* delay_refusal(const piadmm_obca_plan_s* p, int64_t steps) {
  if (!p->dl.on) return nullptr;
  if (p->dl.tape && (int64_t)p->dl.steps + steps > p->dl.cap) return "latency tape exhausted";
  if ((int64_t)p->dl.k0 + p->dl.steps + steps > ((int64_t)1 << 31)) return "delay step index exhausted";
  return nullptr;
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

// What refuses the next `steps` MPC steps of the plan, or nullptr: the trace's rows, the disturbance
// tape's rows, the noise's step index k0 + fb.steps below 2^31, the loop's, the ledger's places.  The
// delay's refusal (delay_refusal) stays each call's own: piadmm_obca_plan_shift names it first,
// piadmm_obca_plan_step behind these.  It excludes the loop's and the ledger's (the delay refuses a
// clock, both need one), not the first three.
// TAPE_EXHAUSTED is the tape's refusal, one array for every unit: piadmm_obca_trace_run tells it by
// its address.
inline constexpr char TAPE_EXHAUSTED[] = "disturbance tape exhausted";
inline const char* step_refusal(const piadmm_obca_plan_s* p, int64_t steps) {
  if (p->tr.on && (int64_t)p->tr.rows + steps > p->tr.cap) return "trace full";
  if (feedback_exhausted(p, steps)) return TAPE_EXHAUSTED;
  if (p->nz.on && (int64_t)p->nz.k0 + p->fb.steps + steps > ((int64_t)1 << 31)) return "noise step index exhausted";
  if (loop_exhausted(p, steps)) return "loop step index exhausted";
  return ledger_refusal(p, steps);
}

}  // namespace obca_plan
