// piadmm_obca_plan_delay.hip -- communication delay in the exchange of the device-resident OBCA-ADMM
// plan: the latencies and the stale message alone (gfx950).  csrc/piadmm_obca_plan.hip describes the
// launch sequence; of it:
// With the communication delay attached (piadmm_obca_delay_plan) k_plan_exchange_stale runs in
// k_plan_exchange's place (what a vehicle sends is computed from its plan interpolated tau back) and
// piadmm_obca_plan_shift launches k_plan_delay last, one lane per vehicle: the latencies of the step
// that opens; without it neither is launched.
// k_plan_exchange_stale is defined next to k_plan_exchange; here are k_plan_delay, the stand-alone
// k_delay_exchange (the same device functions, stale_state of csrc/piadmm_obca_plan_draw.h and
// halfspaces of csrc/piadmm_obca_plan.h, on the caller's arrays) and the calls.

#include "piadmm_obca_plan.h"

namespace obca_plan {

// One lane per vehicle: lane g of a grid row = vehicle g & 1 of entry g >> 1 of `list` (nullptr: of
// scenario g >> 1), 2 m lanes; grid row y is step index k + y (the in-plan step launches one row).
// No LDS, no atomics, nothing shared between lanes: the counter is the lane's own, the key words and
// the step index are kernel arguments, the arithmetic 32-bit integer and fp64 in registers.  The
// lane's 4 parameters are 8-byte loads from the row; its result one 8-byte store, neighbouring lanes
// to neighbouring addresses.
__global__ void __launch_bounds__(64 * PW) k_plan_delay(const int* __restrict__ list, int m, draw_io io) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * m) return;
  const int v = g & 1;
  const size_t s = (size_t)(list ? list[g >> 1] : (g >> 1));
  const size_t y = blockIdx.y;
  const double* P = io.par + s * io.par_s;
  uint32_t t_lo, t_hi;
  stream_words(io.streams, s, t_lo, t_hi);
  const double tape = io.tape ? io.tape[s * io.tape_s + y * 2 + v] : 0.0;
  uint32_t words[4];
  io.out[s * io.out_s + y * 2 + v] = delay_draw(io.seed_lo, io.seed_hi, t_lo, t_hi, io.k + (uint32_t)y, v, P[Y_AVG + v],
                                                P[Y_STD + v], P[Y_TMAX + v], P[Y_TRUNC], tape, io.raw ? words : nullptr);
  if (io.raw) {
    uint32_t* r = io.raw + s * io.raw_s + y * 8 + v * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) r[q] = words[q];
  }
}

// One wave per scenario k of the caller's arrays; lane < 14 owns the (vehicle, slot) item lane =
// v * 7 + t, as in k_plan_exchange_stale, and runs the same two device functions: the stale state
// from X[t] and X[t + 1] under tau[k][v], then its halfspaces.  Nothing of a plan is read or written.
__global__ void __launch_bounds__(64 * PW) k_delay_exchange(int n, const double* __restrict__ X,
                                                            const int* __restrict__ prob,
                                                            const double* __restrict__ tau, double sigd,
                                                            double* __restrict__ lx, double* __restrict__ Ao,
                                                            double* __restrict__ bo) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= n || lane >= 2 * NT) return;
  const int v = lane / NT, t = lane % NT;
  const int pr = prob[k];
  const double tau0 = tau[(size_t)2 * k], tau1 = tau[(size_t)2 * k + 1];
  const double* x1 = X + (size_t)k * NX + v * 40 + (t + 1) * 5;
  double st[5], A[4][2], b[4];
  stale_state(x1 - 5, x1, v ? tau1 : tau0, st);
  halfspaces(st, pr, sigd, A, b);
  const size_t item = (size_t)k * 2 * NT + lane;
#pragma unroll
  for (int j = 0; j < 5; ++j) lx[item * 5 + j] = st[j];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    Ao[item * 8 + 2 * i] = A[i][0];
    Ao[item * 8 + 2 * i + 1] = A[i][1];
    bo[item * 4 + i] = b[i];
  }
}

// The latencies of the step that opens after the shift in flight, step dl.steps + 1 since the
// attachment, into dl.tau: one launch on the handle's stream.  Past the tape's last row or the last
// step index nothing is launched; every call that would run that step is refused (delay_refusal).
int delay_next(piadmm_obca_t h, piadmm_obca_plan_s* p) {
  const int64_t next = (int64_t)p->dl.steps + 1;
  if ((p->dl.tape && next >= p->dl.cap) || (int64_t)p->dl.k0 + next >= ((int64_t)1 << 31)) return 0;
  hipLaunchKernelGGL(k_plan_delay, dim3(lane_blocks(2 * p->n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr, p->n,
                     delay_view(p->dl, (int)next));
  OWN_HIP(h, hipGetLastError());
  return 0;
}

}  // namespace obca_plan

using namespace obca_plan;

namespace obca_plan {
// One delay row: nullptr when it is good, else what is wrong with it.
const char* delay_row_check(const double* row) {
  for (int i = 0; i < YPAR; ++i)
    if (!std::isfinite(row[i])) return "every entry finite";
  for (int v = 0; v < 2; ++v) {
    if (!(row[Y_AVG + v] >= 0.0)) return "avg >= 0";
    if (!(row[Y_STD + v] >= 0.0)) return "std >= 0";
    if (!(row[Y_TMAX + v] >= 0.0 && row[Y_TMAX + v] <= PLANT_DT)) return "0 <= tau_max <= DT";
  }
  if (!(row[Y_TRUNC] >= 0.0)) return "trunc 0 (none) or > 0";
  if (row[Y_RESERVED] != 0.0) return "the reserved entry must be 0";
  return nullptr;
}
}  // namespace obca_plan

namespace {
// rows, streams, k0 and the tape of both delay calls that draw, on the host
int delay_args_check(piadmm_obca_t h, int n, const double* par, int rows, const int64_t* streams, int32_t k0,
                     int64_t steps, const double* tape, int cap, const std::string& who) {
  if (!par) return fail(h, PIADMM_E_ARG, who + ": null argument");
  if (int rc = rows_check(h, who, "", par, rows, n, YPAR, delay_row_check)) return rc;
  if (int rc = streams_check(h, who, streams, n)) return rc;
  if (int rc = step_index_check(h, who, k0, steps)) return rc;
  return tape_finite_check(h, who, tape, n, cap, 2);
}
}  // namespace

extern "C" {

int32_t piadmm_obca_delay_tau(piadmm_obca_t h, int32_t n, int32_t cap, const double* par, int32_t rows,
                              const int64_t* streams, uint64_t seed, int32_t k0, const double* tape, double* tau_out,
                              uint32_t* raw_out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_delay_tau: 1 <= n <= 2^20");
  if (cap < 0 || cap > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_delay_tau: 0 <= cap <= 2^20");
  const size_t N = (size_t)n, C = (size_t)cap, B = sizeof(double);
  if (N * C * 2 * B >= ((size_t)1 << 31))
    return fail(h, PIADMM_E_ARG, "obca_delay_tau: n x cap x 16 bytes must stay below 2 GiB");
  if (int rc = delay_args_check(h, n, par, rows, streams, k0, cap, tape, cap, "obca_delay_tau")) return rc;
  if (cap == 0) return 0;
  if (!tau_out) return fail(h, PIADMM_E_ARG, "obca_delay_tau: null argument");
  OWN_HIP(h, hipSetDevice(h->device));
  scratch a(h);
  double *d_par = a.take<double>((size_t)rows * YPAR, false), *d_out = a.take<double>(N * C * 2, false),
         *d_tape = tape ? a.take<double>(N * C * 2, false) : nullptr;
  long long* d_str = streams ? a.take<long long>(N, false) : nullptr;
  uint32_t* d_raw = raw_out ? a.take<uint32_t>(N * C * 8, false) : nullptr;
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_par, par, (size_t)rows * YPAR * B, hipMemcpyHostToDevice, h->stream));
  if (streams) OWN_HIP(h, hipMemcpyAsync(d_str, streams, N * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  if (tape) OWN_HIP(h, hipMemcpyAsync(d_tape, tape, N * C * 2 * B, hipMemcpyHostToDevice, h->stream));
  if (int rc = draw_launch(h, k_plan_delay, draw_view(d_par, rows, YPAR, d_str, seed), n, cap, k0, 2, 8, d_out, d_tape,
                           d_raw))
    return rc;
  OWN_HIP(h, hipMemcpyAsync(tau_out, d_out, N * C * 2 * B, hipMemcpyDeviceToHost, h->stream));
  if (raw_out)
    OWN_HIP(h, hipMemcpyAsync(raw_out, d_raw, N * C * 8 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_delay_exchange(piadmm_obca_t h, int32_t n, const double* X, const int32_t* prob, const double* tau,
                                   double* lx_out, double* A_out, double* b_out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_delay_exchange: 1 <= n <= 2^20");
  if (!X || !prob || !tau || !lx_out || !A_out || !b_out)
    return fail(h, PIADMM_E_ARG, "obca_delay_exchange: null argument");
  const size_t N = (size_t)n, B = sizeof(double);
  for (int k = 0; k < n; ++k) {
    if (int rc = prob_check(h, "obca_delay_exchange", prob, k)) return rc;
    for (int i = 0; i < NX; ++i)
      if (!std::isfinite(X[(size_t)k * NX + i]))
        return fail(h, PIADMM_E_ARG, "obca_delay_exchange: X of scenario " + std::to_string(k) + " is not finite");
    for (int v = 0; v < 2; ++v)
      if (!(tau[2 * (size_t)k + v] >= 0.0 && tau[2 * (size_t)k + v] <= PLANT_DT))
        return fail(h, PIADMM_E_ARG, "obca_delay_exchange: tau of scenario " + std::to_string(k) + " must be in [0, DT]");
  }
  OWN_HIP(h, hipSetDevice(h->device));
  scratch a(h);
  double *d_X = a.take<double>(N * NX, false), *d_tau = a.take<double>(N * 2, false),
         *d_lx = a.take<double>(N * 70, true), *d_A = a.take<double>(N * 112, true), *d_b = a.take<double>(N * 56, true);
  int* d_prob = a.take<int>(N, false);
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_X, X, N * NX * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_tau, tau, N * 2 * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_prob, prob, N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_delay_exchange, dim3(blocks_for(n)), dim3(64 * PW), 0, h->stream, n, (const double*)d_X,
                     (const int*)d_prob, (const double*)d_tau, std::sqrt(0.95 / (1.0 - 0.95)), d_lx, d_A, d_b);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(lx_out, d_lx, N * 70 * B, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(A_out, d_A, N * 112 * B, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(b_out, d_b, N * 56 * B, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_delay_plan(piadmm_obca_t h, int32_t mode, const double* par, int32_t rows, const int64_t* streams,
                               uint64_t seed, int32_t k0, const double* tape, int32_t cap) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_delay_plan")) return rc;
  if (mode != 0 && mode != 1) return fail(h, PIADMM_E_ARG, "obca_delay_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  const size_t N = (size_t)n;
  if (mode == 1) {
    if (tape && (cap < 0 || cap > (1 << 20))) return fail(h, PIADMM_E_ARG, "obca_delay_plan: 0 <= cap <= 2^20");
    if (int rc = delay_args_check(h, n, par, rows, streams, k0, 0, tape, cap, "obca_delay_plan")) return rc;
    if (p->ck.on)
      return fail(h, PIADMM_E_STATE, "obca_delay_plan: a clock is attached (obca_clock_plan: the delay counts the plan's steps, not per-scenario clocks)");
  }
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_delay_plan: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (mode == 0) {
    p->dl = {};
    return 0;
  }
  // the new attachment is complete, the open step's latencies included, before it replaces the earlier one
  piadmm_obca_plan_s::delay_s nd;
  const std::vector<long long> ids = stream_ids(streams, N);
  const size_t T = tape ? N * (size_t)cap * 2 : 0;
  hipError_t e = nd.par.make((size_t)rows * YPAR);
  if (e == hipSuccess) e = nd.tau.make(N * 2);
  if (e == hipSuccess) e = nd.streams.make(N);
  if (e == hipSuccess) e = hipMemset(nd.tau, 0, N * 2 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(nd.par, par, (size_t)rows * YPAR * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(nd.streams, ids.data(), N * sizeof(long long), hipMemcpyHostToDevice);
  if (e == hipSuccess && tape) {
    // a tape without rows still counts as one: every step is then refused
    e = nd.tape.make(std::max(T, (size_t)1));
    if (e == hipSuccess && T) e = hipMemcpy(nd.tape, tape, T * sizeof(double), hipMemcpyHostToDevice);
  }
  // the fill and the copies went through the null stream, which the handle's stream does not wait for
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  nd.rows = rows;
  nd.seed = seed;
  nd.k0 = k0;
  nd.cap = tape ? cap : 0;
  nd.steps = 0;
  if (e == hipSuccess && !(tape && cap == 0)) {
    hipLaunchKernelGGL(k_plan_delay, dim3(lane_blocks(2 * n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr, n,
                       delay_view(nd, 0));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    return fail(h, PIADMM_E_HIP, std::string("obca_delay_plan: ") + hipGetErrorString(e));
  }
  nd.on = true;
  p->dl = std::move(nd);
  return 0;
}

}  // extern "C"
