// piadmm_obca_plan_feedback.hip -- the closed loop of the device-resident OBCA-ADMM plan: the plant
// step, the measurement and the device-side noise (gfx950).  csrc/piadmm_obca_plan.hip describes the
// launch sequence; of it:
// With the feedback attached (piadmm_obca_feedback_plan) piadmm_obca_plan_shift runs k_plan_propagate
// before k_plan_shift (the plant step from the closing step's init_state and first control) and
// k_plan_set_init after it (the state the vehicle reached over init_state of both copies); without
// it neither is launched.  These two run one lane per vehicle, not one wave per item.
// With the noise attached on top (piadmm_obca_noise_plan) k_plan_noise runs in front of
// k_plan_propagate and writes the step's disturbance rows, which that kernel reads in the tape's
// place; without it k_plan_noise is not launched.  One lane per vehicle as well.

#include "piadmm_obca_plan.h"

namespace obca_plan {

// ---------------------------------------------------------------------------------------------
// Closed-loop feedback (piadmm_obca_feedback_plan / _measure, piadmm_obca_propagate): the plant step
// between two MPC steps and the scatter of states over init_state.  Opt-in: without the attachment
// neither kernel is launched by piadmm_obca_plan_shift.
// ---------------------------------------------------------------------------------------------

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
  double P[FV];
  plant_row_load(io.par + s * io.par_s + v * FV, P);
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

// One lane per vehicle: lane g of a grid row = vehicle g & 1 of entry g >> 1 of `list` (nullptr: of
// scenario g >> 1), 2 m lanes; grid row y is step index k + y (the in-plan step launches one row).
// No LDS, no atomics, nothing shared between lanes: the counter is the lane's own, the arithmetic
// 32-bit integer and fp64 in registers.  The lane's 11 parameters are 8-byte loads from the row;
// its five results 8-byte stores, neighbouring lanes to neighbouring rows as in k_plan_propagate.
// With a tape the written value is tape + w, the tape term first.
__global__ void __launch_bounds__(64 * PW) k_plan_noise(const int* __restrict__ list, int m, draw_io io) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * m) return;
  const int v = g & 1;
  const size_t s = (size_t)(list ? list[g >> 1] : (g >> 1));
  const size_t y = blockIdx.y;
  const double* P = io.par + s * io.par_s;
  double S[5], B[5];
  noise_row_load(P, v, S, B);
  uint32_t t_lo, t_hi;
  stream_words(io.streams, s, t_lo, t_hi);
  uint32_t words[12];
  double w[5];
  noise_draw(io.seed_lo, io.seed_hi, t_lo, t_hi, io.k + (uint32_t)y, v, S, B, P[Z_TRUNC], w, io.raw ? words : nullptr);
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

}  // namespace obca_plan

using namespace obca_plan;

namespace obca_plan {
// One plant row of the feedback (both vehicles): nullptr when it is good, else what is wrong with it.
const char* feedback_row_check(const double* row) {
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
  for (int v = 0; v < 2; ++v) {
    double* P = row + v * FV;
    P[F_METHOD] = 0.0;  P[F_NSUB] = 1.0;  P[F_LR] = 1.0;  P[F_LF] = 1.5;
    P[F_GA] = 1.0;  P[F_GW] = 1.0;  P[F_AMAX] = 5.0;  P[F_WMAX] = 20.0;
  }
}
}  // namespace obca_plan

namespace {
// the first entry of a[0 .. count) that is not finite, or -1
int64_t first_not_finite(const double* a, size_t count) {
  for (size_t i = 0; i < count; ++i)
    if (!std::isfinite(a[i])) return (int64_t)i;
  return -1;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_propagate(piadmm_obca_t h, int32_t n, const double* states, const double* ctrl, const double* par,
                              const double* w, double* out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_propagate: 1 <= n <= 2^20");
  if (!states || !ctrl || !par || !out) return fail(h, PIADMM_E_ARG, "obca_propagate: null argument");
  const size_t N = (size_t)n;
  int64_t bad = -1;
  if ((bad = first_not_finite(states, N * 10)) >= 0)
    return fail(h, PIADMM_E_ARG, "obca_propagate: state pair " + std::to_string(bad / 10) + " is not finite");
  if ((bad = first_not_finite(ctrl, N * 4)) >= 0)
    return fail(h, PIADMM_E_ARG, "obca_propagate: ctrl of scenario " + std::to_string(bad / 4) + " is not finite");
  if (w && (bad = first_not_finite(w, N * 10)) >= 0)
    return fail(h, PIADMM_E_ARG, "obca_propagate: w of scenario " + std::to_string(bad / 10) + " is not finite");
  if (int rc = rows_check(h, "obca_propagate", "", par, n, n, FPAR, feedback_row_check)) return rc;
  OWN_HIP(h, hipSetDevice(h->device));
  const size_t B = sizeof(double);
  scratch a(h);
  double *d_st = a.take<double>(N * 10, false), *d_ct = a.take<double>(N * 4, false),
         *d_par = a.take<double>(N * FPAR, false), *d_w = w ? a.take<double>(N * 10, false) : nullptr,
         *d_out = a.take<double>(N * 10, true);
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_st, states, N * 10 * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_ct, ctrl, N * 4 * B, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_par, par, N * FPAR * B, hipMemcpyHostToDevice, h->stream));
  if (w) OWN_HIP(h, hipMemcpyAsync(d_w, w, N * 10 * B, hipMemcpyHostToDevice, h->stream));
  plant_io io{};
  io.x0 = d_st;  io.x0_s = 10;
  io.ctrl = d_ct;  io.ctrl_s = 4;  io.ctrl_v = 2;  io.ctrl_w = 1;
  io.par = d_par;  io.par_s = FPAR;
  io.w = d_w;  io.w_s = 10;
  io.out = d_out;
  hipLaunchKernelGGL(k_plan_propagate, dim3(lane_blocks(2 * n)), dim3(64 * PW), 0, h->stream, (const int*)nullptr, n,
                     io);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(out, d_out, N * 10 * B, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_feedback_plan(piadmm_obca_t h, int32_t mode, const double* par, int32_t rows, const double* tape,
                                  int32_t cap) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_feedback_plan")) return rc;
  if (mode != 0 && mode != 1) return fail(h, PIADMM_E_ARG, "obca_feedback_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  const size_t N = (size_t)n;
  double nominal[FPAR];
  feedback_row_nominal(nominal);
  if (mode == 1) {
    if (int rc = rows_check(h, "obca_feedback_plan", "", par, rows, n, FPAR, feedback_row_check)) return rc;
    if (!par) {
      par = nominal;
      rows = 1;
    }
    if (tape && (cap < 0 || cap > (1 << 20))) return fail(h, PIADMM_E_ARG, "obca_feedback_plan: 0 <= cap <= 2^20");
    if (int rc = tape_finite_check(h, "obca_feedback_plan", tape, n, cap, 10)) return rc;
    if (p->ck.on)
      return fail(h, PIADMM_E_STATE, "obca_feedback_plan: a clock is attached (obca_clock_plan: the tape has no per-scenario clocks)");
  }
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_feedback_plan: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (mode == 0) {
    p->fb = {};
    p->nz = {};    // the noise counts its steps by the feedback's: it goes whenever the feedback goes or is replaced
    return 0;
  }
  // the new attachment is complete before it replaces the earlier one
  piadmm_obca_plan_s::feedback_s nf;
  const size_t T = N * (size_t)cap * 10;
  hipError_t e = nf.par.make((size_t)rows * FPAR);
  if (e == hipSuccess) e = nf.next.make(N * 10);
  if (e == hipSuccess) e = hipMemset(nf.next, 0, N * 10 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(nf.par, par, (size_t)rows * FPAR * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess && tape) {
    // a tape without rows still counts as one: every shift is then refused
    e = nf.tape.make(std::max(T, (size_t)1));
    if (e == hipSuccess && T) e = hipMemcpy(nf.tape, tape, T * sizeof(double), hipMemcpyHostToDevice);
  }
  if (e != hipSuccess) return fail(h, PIADMM_E_HIP, std::string("obca_feedback_plan: ") + hipGetErrorString(e));
  p->fb = std::move(nf);
  p->nz = {};      // as above
  p->fb.rows = rows;
  p->fb.stride = rows > 1 ? FPAR : 0;
  p->fb.cap = tape ? cap : 0;
  p->fb.steps = 0;
  p->fb.on = true;
  return 0;
}

int32_t piadmm_obca_feedback_measure(piadmm_obca_t h, int32_t m, const int32_t* slots, const double* states) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_feedback_measure")) return rc;
  const int n = p->n;
  if (m < 1 || m > n) return fail(h, PIADMM_E_ARG, "obca_feedback_measure: 1 <= m <= n_scenarios");
  if (!slots || !states) return fail(h, PIADMM_E_ARG, "obca_feedback_measure: null argument");
  for (int k = 0; k < m; ++k)
    if (slots[k] < 0 || slots[k] >= n || (k > 0 && slots[k] <= slots[k - 1]))
      return fail(h, PIADMM_E_ARG, "obca_feedback_measure: slots[" + std::to_string(k) +
                  "] must be a scenario below n, the slots ascending and distinct");
  const int64_t bad = first_not_finite(states, (size_t)m * 10);
  if (bad >= 0)
    return fail(h, PIADMM_E_ARG, "obca_feedback_measure: state pair " + std::to_string(bad / 10) + " is not finite");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_feedback_measure: only at a step boundary (an MPC step is open)");
  if (p->tr.on)
    return fail(h, PIADMM_E_STATE, "obca_feedback_measure: a trace is attached (its last row was computed from the state being replaced)");
  OWN_HIP(h, hipSetDevice(h->device));
  // the states, then the slot numbers, through the staging buffer; one scatter launch
  const size_t body = (size_t)m * 10 * sizeof(double);
  if (int rc = stage_ensure(h, p, body, m)) return rc;
  int* d_list = reinterpret_cast<int*>(p->stg.buf + body);
  OWN_HIP(h, hipMemcpyAsync(p->stg.buf, states, body, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_set_init, dim3(lane_blocks(2 * m)), dim3(64 * PW), 0, h->stream, (const int*)d_list, m,
                     reinterpret_cast<const double*>(p->stg.buf.get()), p->bar, p->barp);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// Device-side disturbance noise (include/piadmm.h)
// ---------------------------------------------------------------------------------------------
namespace obca_plan {
// One noise row: nullptr when it is good, else what is wrong with it.
const char* noise_row_check(const double* row) {
  for (int i = 0; i < ZPAR; ++i)
    if (!std::isfinite(row[i])) return "every entry finite";
  for (int i = 0; i < 10; ++i)
    if (!(row[Z_SIGMA + i] >= 0.0)) return "sigma >= 0";
  if (!(row[Z_TRUNC] >= 0.0)) return "trunc 0 (none) or > 0";
  if (row[Z_RESERVED] != 0.0) return "the reserved entry must be 0";
  return nullptr;
}
}  // namespace obca_plan

namespace {
// rows, streams and k0 of both noise calls, on the host
int noise_args_check(piadmm_obca_t h, int n, const double* par, int rows, const int64_t* streams, int32_t k0,
                     int64_t steps, const std::string& who) {
  if (!par) return fail(h, PIADMM_E_ARG, who + ": null argument");
  if (int rc = rows_check(h, who, "", par, rows, n, ZPAR, noise_row_check)) return rc;
  if (int rc = streams_check(h, who, streams, n)) return rc;
  return step_index_check(h, who, k0, steps);
}
}  // namespace

extern "C" {

int32_t piadmm_obca_noise_tape(piadmm_obca_t h, int32_t n, int32_t cap, const double* par, int32_t rows,
                               const int64_t* streams, uint64_t seed, int32_t k0, double* tape_out, uint32_t* raw_out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_noise_tape: 1 <= n <= 2^20");
  if (cap < 0 || cap > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_noise_tape: 0 <= cap <= 2^20");
  const size_t N = (size_t)n, C = (size_t)cap, B = sizeof(double);
  if (N * C * 10 * B >= ((size_t)1 << 31))
    return fail(h, PIADMM_E_ARG, "obca_noise_tape: n x cap x 80 bytes must stay below 2 GiB");
  if (int rc = noise_args_check(h, n, par, rows, streams, k0, cap, "obca_noise_tape")) return rc;
  if (cap == 0) return 0;
  if (!tape_out) return fail(h, PIADMM_E_ARG, "obca_noise_tape: null argument");
  OWN_HIP(h, hipSetDevice(h->device));
  scratch a(h);
  double *d_par = a.take<double>((size_t)rows * ZPAR, false), *d_out = a.take<double>(N * C * 10, false);
  long long* d_str = streams ? a.take<long long>(N, false) : nullptr;
  uint32_t* d_raw = raw_out ? a.take<uint32_t>(N * C * 24, false) : nullptr;
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_par, par, (size_t)rows * ZPAR * B, hipMemcpyHostToDevice, h->stream));
  if (streams) OWN_HIP(h, hipMemcpyAsync(d_str, streams, N * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  if (int rc = draw_launch(h, k_plan_noise, draw_view(d_par, rows, ZPAR, d_str, seed), n, cap, k0, 10, 24, d_out, nullptr,
                           d_raw))
    return rc;
  OWN_HIP(h, hipMemcpyAsync(tape_out, d_out, N * C * 10 * B, hipMemcpyDeviceToHost, h->stream));
  if (raw_out)
    OWN_HIP(h, hipMemcpyAsync(raw_out, d_raw, N * C * 24 * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_noise_plan(piadmm_obca_t h, int32_t mode, const double* par, int32_t rows, const int64_t* streams,
                               uint64_t seed, int32_t k0) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_noise_plan")) return rc;
  if (mode != 0 && mode != 1) return fail(h, PIADMM_E_ARG, "obca_noise_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  const size_t N = (size_t)n;
  if (mode == 1)
    if (int rc = noise_args_check(h, n, par, rows, streams, k0, 0, "obca_noise_plan")) return rc;
  if (mode == 1 && !p->fb.on)
    return fail(h, PIADMM_E_STATE, "obca_noise_plan: no feedback attached (obca_feedback_plan: the noise enters through the plant step)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_noise_plan: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (mode == 0) {
    p->nz = {};
    return 0;
  }
  // the new attachment is complete before it replaces the earlier one
  piadmm_obca_plan_s::noise_s nz;
  const std::vector<long long> ids = stream_ids(streams, N);
  hipError_t e = nz.par.make((size_t)rows * ZPAR);
  if (e == hipSuccess) e = nz.wbuf.make(N * 10);
  if (e == hipSuccess) e = nz.streams.make(N);
  if (e == hipSuccess) e = hipMemset(nz.wbuf, 0, N * 10 * sizeof(double));
  if (e == hipSuccess) e = hipMemcpy(nz.par, par, (size_t)rows * ZPAR * sizeof(double), hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(nz.streams, ids.data(), N * sizeof(long long), hipMemcpyHostToDevice);
  if (e != hipSuccess) return fail(h, PIADMM_E_HIP, std::string("obca_noise_plan: ") + hipGetErrorString(e));
  p->nz = std::move(nz);
  p->nz.rows = rows;
  p->nz.seed = seed;
  p->nz.k0 = k0;
  p->nz.on = true;
  return 0;
}

}  // extern "C"
