// piadmm_obca_plan_loop.hip -- the loop of the device-resident OBCA-ADMM plan: the closed loop (plant,
// noise, delay) of a clocked plan, its step index each tenant's own clock (gfx950).
// csrc/piadmm_obca_plan.hip describes the launch sequence; of it:
// With the loop attached (piadmm_obca_loop_plan; a clocked plan only) piadmm_obca_plan_shift runs
// k_loop_close before k_plan_shift_list (noise at k0 + c plus the plant step of the scenarios the
// step ran) and k_plan_set_init after it (the state each reached over init_state of both copies),
// and with delay rows k_loop_open after the tick (the latencies of the alive scenarios at their new
// clocks) and every iterate k_plan_exchange_stale in k_plan_exchange's place; without it none is
// launched.  The arithmetic is plant_step, noise_draw and delay_draw of csrc/piadmm_obca_plan_draw.h, the
// functions k_plan_propagate, k_plan_noise and k_plan_delay call.

#include "piadmm_obca_plan.h"

namespace obca_plan {

// One lane per (entry of the list, vehicle): lane g = vehicle g & 1 of scenario s = list[g >> 1]
// (nullptr: g >> 1), 2 m lanes.  The disturbance row of stream streams[s] at step index k0 + clk[3 s]
// (none without noise rows) and the plant step from init_state under the first control, all in
// registers; next[g >> 1][v] = x + w, the sum k_plan_propagate forms.  No LDS, no barrier, no atomic;
// the loads are those of k_plan_noise and k_plan_propagate.
__global__ void __launch_bounds__(64 * PW) k_loop_close(const int* __restrict__ list, int m, loop_io io) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * m) return;
  const int v = g & 1;
  const size_t s = (size_t)(list ? list[g >> 1] : (g >> 1));
  double P[FV];
  plant_row_load(io.plant + s * io.plant_s + v * FV, P);
  const double* xin = io.x0 + s * STATE + v * 5;
  const double* cu = io.ctrl + s * NCTRL + v * (NCTRL / 2);
  double x[5];
#pragma unroll
  for (int i = 0; i < 5; ++i) x[i] = xin[i];
  plant_step(x, cu[0], cu[NT], P);
  double* o = io.next + (size_t)(g >> 1) * 10 + v * 5;
  if (io.noise) {
#pragma clang fp contract(off)
    const double* Z = io.noise + s * io.noise_s;
    double S[5], B[5], w[5];
    noise_row_load(Z, v, S, B);
    uint32_t t_lo, t_hi;
    stream_words(io.streams, s, t_lo, t_hi);
    noise_draw(io.seed_lo, io.seed_hi, t_lo, t_hi, io.k0 + (uint32_t)io.clk[3 * s], v, S, B, Z[Z_TRUNC], w, nullptr);
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = x[i] + w[i];
  } else {
#pragma unroll
    for (int i = 0; i < 5; ++i) o[i] = x[i];
  }
}

// One lane per (entry of the list, vehicle), as above: tau[s][v] = the latency of stream streams[s]
// at step index k0 + clk[3 s] under the scenario's delay row.  Launched only with delay rows.
__global__ void __launch_bounds__(64 * PW) k_loop_open(const int* __restrict__ list, int m, loop_io io) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * m) return;
  const int v = g & 1;
  const size_t s = (size_t)(list ? list[g >> 1] : (g >> 1));
  const double* Y = io.delay + s * io.delay_s;
  uint32_t t_lo, t_hi;
  stream_words(io.streams, s, t_lo, t_hi);
  io.tau[2 * s + v] = delay_draw(io.seed_lo, io.seed_hi, t_lo, t_hi, io.k0 + (uint32_t)io.clk[3 * s], v, Y[Y_AVG + v],
                                 Y[Y_STD + v], Y[Y_TMAX + v], Y[Y_TRUNC], 0.0, nullptr);
}

// The stand-alone draw (piadmm_obca_loop_draw): one lane per (scenario, vehicle) of the caller's
// arrays, next[s][v] = the disturbance row and tau[s][v] = the latency at step index k0 + clk[3 s];
// zeros where the kind is absent.  The same two device functions as the in-plan kernels.
__global__ void __launch_bounds__(64 * PW) k_loop_draw(int n, loop_io io) {
  const int g = blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= 2 * n) return;
  const int v = g & 1;
  const size_t s = (size_t)(g >> 1);
  uint32_t t_lo, t_hi;
  stream_words(io.streams, s, t_lo, t_hi);
  const uint32_t k = io.k0 + (uint32_t)io.clk[3 * s];
  double w[5] = {0.0, 0.0, 0.0, 0.0, 0.0}, tau = 0.0;
  if (io.noise) {
    const double* Z = io.noise + s * io.noise_s;
    double S[5], B[5];
    noise_row_load(Z, v, S, B);
    noise_draw(io.seed_lo, io.seed_hi, t_lo, t_hi, k, v, S, B, Z[Z_TRUNC], w, nullptr);
  }
  if (io.delay) {
    const double* Y = io.delay + s * io.delay_s;
    tau = delay_draw(io.seed_lo, io.seed_hi, t_lo, t_hi, k, v, Y[Y_AVG + v], Y[Y_STD + v], Y[Y_TMAX + v], Y[Y_TRUNC], 0.0,
                     nullptr);
  }
  double* o = io.next + s * 10 + v * 5;
#pragma unroll
  for (int i = 0; i < 5; ++i) o[i] = w[i];
  io.tau[2 * s + v] = tau;
}

// What clock_shift enqueues for the loop, each one launch on the handle's stream, no synchronisation.
// Before the shift: the states the scenarios of ck.list reach, into lp.next by list position.
int loop_close(piadmm_obca_t h, piadmm_obca_plan_s* p) {
  const int m = p->ck.n_list;
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_loop_close, dim3(lane_blocks(2 * m)), dim3(64 * PW), 0, h->stream, (const int*)p->ck.list, m,
                     loop_view(p, p->lp));
  OWN_HIP(h, hipGetLastError());
  return 0;
}
// After the shift, before the tick rebuilds ck.list: lp.next over init_state of both state copies.
int loop_set_init(piadmm_obca_t h, piadmm_obca_plan_s* p) {
  const int m = p->ck.n_list;
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_plan_set_init, dim3(lane_blocks(2 * m)), dim3(64 * PW), 0, h->stream, (const int*)p->ck.list, m,
                     (const double*)p->lp.next, p->bar, p->barp);
  OWN_HIP(h, hipGetLastError());
  return 0;
}
// After the lists are rebuilt (a tick, an admission): the latencies of the m scenarios now in ck.list
// at their clocks.  A retired scenario's latency stays.  A pure function of
// (seed, stream, k0 + c), so a scenario whose clock and row did not change draws what it holds.
int loop_open(piadmm_obca_t h, piadmm_obca_plan_s* p, int m) {
  if (!(p->lp.flags & 4) || m <= 0) return 0;
  hipLaunchKernelGGL(k_loop_open, dim3(lane_blocks(2 * m)), dim3(64 * PW), 0, h->stream, (const int*)p->ck.list, m,
                     loop_view(p, p->lp));
  OWN_HIP(h, hipGetLastError());
  return 0;
}

}  // namespace obca_plan

using namespace obca_plan;

namespace {
// the rows of the kinds a loop call takes (nullptr: the kind is absent) and its stream ids
int loop_args_check(piadmm_obca_t h, const std::string& who, int n, const double* plant, int plant_rows,
                    const double* noise, int noise_rows, const double* delay, int delay_rows, const int64_t* streams) {
  if (int rc = rows_check(h, who, "plant", plant, plant_rows, n, FPAR, feedback_row_check)) return rc;
  if (int rc = rows_check(h, who, "noise", noise, noise_rows, n, ZPAR, noise_row_check)) return rc;
  if (int rc = rows_check(h, who, "delay", delay, delay_rows, n, YPAR, delay_row_check)) return rc;
  return streams_check(h, who, streams, n);
}
}  // namespace

extern "C" {

int32_t piadmm_obca_loop_plan(piadmm_obca_t h, int32_t mode, const double* plant, int32_t plant_rows,
                              const double* noise, int32_t noise_rows, const double* delay, int32_t delay_rows,
                              const int64_t* streams, uint64_t seed, int32_t k0) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_loop_plan")) return rc;
  if (mode != 0 && mode != 1) return fail(h, PIADMM_E_ARG, "obca_loop_plan: mode 0 (detach) or 1 (attach)");
  const int n = p->n;
  const size_t N = (size_t)n;
  double nominal[FPAR];
  feedback_row_nominal(nominal);
  if (mode == 1) {
    const std::string who = "obca_loop_plan";
    if (!plant) {
      plant = nominal;
      plant_rows = 1;
    }
    if (int rc = loop_args_check(h, who, n, plant, plant_rows, noise, noise_rows, delay, delay_rows, streams)) return rc;
    if (k0 < 0) return fail(h, PIADMM_E_ARG, "obca_loop_plan: k0 >= 0");
    if (p->fb.on) return fail(h, PIADMM_E_STATE, "obca_loop_plan: feedback is attached (obca_feedback_plan: it counts the plan's steps; detach it)");
    if (p->dl.on) return fail(h, PIADMM_E_STATE, "obca_loop_plan: the delay is attached (obca_delay_plan: it counts the plan's steps; detach it)");
    if (!p->ck.on) return fail(h, PIADMM_E_STATE, "obca_loop_plan: no clock attached (obca_clock_plan: the loop's step index is the tenant's clock)");
  }
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_loop_plan: only at a step boundary (an MPC step is open)");
  if (mode == 1)
    for (int s = 0; s < n; ++s)
      if (p->ck.host[3 * (size_t)s + 2] && (int64_t)k0 + p->ck.host[3 * (size_t)s] >= ((int64_t)1 << 31))
        return fail(h, PIADMM_E_STATE, "obca_loop_plan: loop step index exhausted (scenario " + std::to_string(s) + ")");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (mode == 0) {
    p->lp = {};
    return 0;
  }
  // the new attachment is complete, the open step's latencies included, before it replaces the earlier one
  piadmm_obca_plan_s::loop_s nl;
  const std::vector<long long> ids = stream_ids(streams, N);
  const size_t D = sizeof(double);
  hipError_t e = nl.plant.make((size_t)plant_rows * FPAR);
  if (e == hipSuccess) e = nl.tau.make(N * 2);
  if (e == hipSuccess) e = nl.next.make(N * 10);
  if (e == hipSuccess) e = nl.streams.make(N);
  if (e == hipSuccess && noise) e = nl.noise.make((size_t)noise_rows * ZPAR);
  if (e == hipSuccess && delay) e = nl.delay.make((size_t)delay_rows * YPAR);
  if (e == hipSuccess) e = hipMemset(nl.tau, 0, N * 2 * D);
  if (e == hipSuccess) e = hipMemset(nl.next, 0, N * 10 * D);
  if (e == hipSuccess) e = hipMemcpy(nl.plant, plant, (size_t)plant_rows * FPAR * D, hipMemcpyHostToDevice);
  if (e == hipSuccess) e = hipMemcpy(nl.streams, ids.data(), N * sizeof(long long), hipMemcpyHostToDevice);
  if (e == hipSuccess && noise) e = hipMemcpy(nl.noise, noise, (size_t)noise_rows * ZPAR * D, hipMemcpyHostToDevice);
  if (e == hipSuccess && delay) e = hipMemcpy(nl.delay, delay, (size_t)delay_rows * YPAR * D, hipMemcpyHostToDevice);
  // the fills and the copies went through the null stream, which the handle's stream does not wait for
  if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
  nl.flags = 1 | (noise ? 2 : 0) | (delay ? 4 : 0);
  nl.plant_rows = plant_rows;
  nl.noise_rows = noise ? noise_rows : 0;
  nl.delay_rows = delay ? delay_rows : 0;
  nl.seed = seed;
  nl.k0 = k0;
  if (e == hipSuccess && delay && p->ck.n_list > 0) {
    hipLaunchKernelGGL(k_loop_open, dim3(lane_blocks(2 * p->ck.n_list)), dim3(64 * PW), 0, h->stream,
                       (const int*)p->ck.list, p->ck.n_list, loop_view(p, nl));
    e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(h->stream);
  }
  if (e != hipSuccess) {
    (void)hipStreamSynchronize(h->stream);
    return fail(h, PIADMM_E_HIP, std::string("obca_loop_plan: ") + hipGetErrorString(e));
  }
  nl.on = true;
  p->lp = std::move(nl);
  return 0;
}

int32_t piadmm_obca_loop_admit(piadmm_obca_t h, int32_t m, const int32_t* slots, const double* plant,
                               const double* noise, const double* delay, const int64_t* streams) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_loop_admit")) return rc;
  const int n = p->n;
  const std::string who = "obca_loop_admit";
  if (m < 1 || m > n) return fail(h, PIADMM_E_ARG, "obca_loop_admit: 1 <= m <= n_scenarios");
  if (!slots) return fail(h, PIADMM_E_ARG, "obca_loop_admit: null argument (slots)");
  if (int rc = slots_check(h, who, "slots", slots, m, n)) return rc;
  if (int rc = loop_args_check(h, who, m, plant, m, noise, m, delay, m, streams)) return rc;
  auto& l = p->lp;
  if (!l.on) return fail(h, PIADMM_E_STATE, "obca_loop_admit: no loop attached (obca_loop_plan)");
  if (p->tr.on) return fail(h, PIADMM_E_STATE, "obca_loop_admit: a trace is attached (its minima would mix two tenants)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_loop_admit: only at a step boundary (an MPC step is open)");
  if (plant && l.plant_rows != n) return fail(h, PIADMM_E_STATE, "obca_loop_admit: plant needs a loop with a plant row per scenario");
  if (noise && l.noise_rows != n) return fail(h, PIADMM_E_STATE, "obca_loop_admit: noise needs a loop with a noise row per scenario");
  if (delay && l.delay_rows != n) return fail(h, PIADMM_E_STATE, "obca_loop_admit: delay needs a loop with a delay row per scenario");
  if (const char* why = ledger_replace_refusal(p, m, slots, true)) return fail(h, PIADMM_E_STATE, who + ": " + why);
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (p->lg.on) {
    // a tenant that has closed a step leaves under its old stream id; one that has not (the second half
    // of an admission) keeps its record, opened again below under the new one
    if (int rc = ledger_close(h, p, m, slots, 2, true)) return rc;
  }
  const size_t D = sizeof(double);
  for (int k = 0; k < m; ++k) {
    const size_t s = (size_t)slots[k], K = (size_t)k;
    if (plant) OWN_HIP(h, hipMemcpy(l.plant + s * FPAR, plant + K * FPAR, FPAR * D, hipMemcpyHostToDevice));
    if (noise) OWN_HIP(h, hipMemcpy(l.noise + s * ZPAR, noise + K * ZPAR, ZPAR * D, hipMemcpyHostToDevice));
    if (delay) OWN_HIP(h, hipMemcpy(l.delay + s * YPAR, delay + K * YPAR, YPAR * D, hipMemcpyHostToDevice));
    if (streams) OWN_HIP(h, hipMemcpy(l.streams + s, streams + K, sizeof(long long), hipMemcpyHostToDevice));
  }
  OWN_HIP(h, hipStreamSynchronize(nullptr));
  if (int rc = loop_open(h, p, p->ck.n_list)) {
    (void)hipStreamSynchronize(h->stream);
    return rc;
  }
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  if (p->lg.on) {
    if (int rc = ledger_open(h, p, m, slots)) return rc;
  }
  return 0;
}

int32_t piadmm_obca_loop_draw(piadmm_obca_t h, int32_t n, const int32_t* clock, const double* noise, int32_t noise_rows,
                              const double* delay, int32_t delay_rows, const int64_t* streams, uint64_t seed, int32_t k0,
                              double* w_out, double* tau_out) {
  if (!h) return PIADMM_E_ARG;
  const std::string who = "obca_loop_draw";
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_loop_draw: 1 <= n <= 2^20");
  if (!clock || !w_out || !tau_out) return fail(h, PIADMM_E_ARG, "obca_loop_draw: null argument (clock, w_out, tau_out)");
  if (int rc = loop_args_check(h, who, n, nullptr, 0, noise, noise_rows, delay, delay_rows, streams)) return rc;
  if (k0 < 0) return fail(h, PIADMM_E_ARG, "obca_loop_draw: k0 >= 0");
  for (int s = 0; s < n; ++s) {
    const int c = clock[3 * (size_t)s];
    if (c < 0 || (int64_t)k0 + c >= ((int64_t)1 << 31))
      return fail(h, PIADMM_E_ARG, "obca_loop_draw: row " + std::to_string(s) + ": c >= 0 and the step index k0 + c below 2^31");
  }
  OWN_HIP(h, hipSetDevice(h->device));
  const size_t N = (size_t)n, D = sizeof(double);
  scratch a(h);
  int* d_clk = a.take<int>(3 * N, false);
  double *d_z = noise ? a.take<double>((size_t)noise_rows * ZPAR, false) : nullptr,
         *d_y = delay ? a.take<double>((size_t)delay_rows * YPAR, false) : nullptr,
         *d_w = a.take<double>(N * 10, false), *d_tau = a.take<double>(N * 2, false);
  long long* d_str = streams ? a.take<long long>(N, false) : nullptr;
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_clk, clock, 3 * N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  if (noise) OWN_HIP(h, hipMemcpyAsync(d_z, noise, (size_t)noise_rows * ZPAR * D, hipMemcpyHostToDevice, h->stream));
  if (delay) OWN_HIP(h, hipMemcpyAsync(d_y, delay, (size_t)delay_rows * YPAR * D, hipMemcpyHostToDevice, h->stream));
  if (streams) OWN_HIP(h, hipMemcpyAsync(d_str, streams, N * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
  loop_io io{};
  io.noise = d_z;  io.noise_s = noise_rows > 1 ? ZPAR : 0;
  io.delay = d_y;  io.delay_s = delay_rows > 1 ? YPAR : 0;
  io.streams = d_str;
  io.clk = d_clk;
  io.next = d_w;
  io.tau = d_tau;
  io.seed_lo = (uint32_t)seed;  io.seed_hi = (uint32_t)(seed >> 32);
  io.k0 = (uint32_t)k0;
  hipLaunchKernelGGL(k_loop_draw, dim3(lane_blocks(2 * n)), dim3(64 * PW), 0, h->stream, n, io);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(w_out, d_w, N * 10 * D, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipMemcpyAsync(tau_out, d_tau, N * 2 * D, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
