// piadmm_obca_plan_draw.h -- what the closed loop of the device-resident OBCA-ADMM plan shares
// (internal, not installed): the plant step, the Philox draws of the noise and the delay, the stale
// state, the launch views of their kernels and the argument checks of their calls, each stated once
// for csrc/piadmm_obca_plan_{feedback,delay,loop}.hip and the shift of csrc/piadmm_obca_plan.hip.
// csrc/piadmm_obca_plan.h includes it behind the plan (the views are built from the plan's
// attachments); nothing else does.
#pragma once

namespace obca_plan {

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

// where the arrays of one k_plan_noise or k_plan_delay launch sit, indexed by scenario: par the noise
// or delay rows (par_s = 0: one shared row), streams the stream ids (nullptr: the scenario's number),
// tape the rows added in front (nullptr: none), out the result, raw the Philox words (nullptr: not
// kept); the strides in elements per scenario, and per step index (blockIdx.y) the kernel's own
// widths of tape and out and of raw: 10 doubles and 24 words for the noise, 2 doubles and 8 words for
// the delay; k = the step index of blockIdx.y = 0
struct draw_io {
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

// ---------------------------------------------------------------------------------------------
// The device side
// ---------------------------------------------------------------------------------------------
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

// Two normals of one Philox call's four words: two uniforms in (0, 1) on 52 bits and the half, then
// Box-Muller, (zc, zs) = rad (cos, sin)(ang).  piadmm.obca.noise_uniform and _box_muller are the same
// statements on the host.
__device__ __forceinline__ void box_muller(const uint32_t c[4], double& zc, double& zs) {
#pragma clang fp contract(off)
  const unsigned long long a = ((unsigned long long)c[0] << 32) | c[1];
  const unsigned long long b = ((unsigned long long)c[2] << 32) | c[3];
  const double u1 = ((double)(a >> 12) + 0.5) * 0x1p-52;
  const double u2 = ((double)(b >> 12) + 0.5) * 0x1p-52;
  const double rad = sqrt(-2.0 * log(u1));
  const double ang = 6.283185307179586 * u2;
  zc = rad * cos(ang);
  zs = rad * sin(ang);
}

// The loads more than one kernel makes.  The plant row of one vehicle, P (8) = row[0 .. 8): 64 bytes
// on a 64-byte boundary (the base comes from hipMalloc), four 16-byte loads.
__device__ __forceinline__ void plant_row_load(const double* row, double P[FV]) {
  const double2* P2 = reinterpret_cast<const double2*>(row);
#pragma unroll
  for (int i = 0; i < FV / 2; ++i) {
    const double2 q = P2[i];
    P[2 * i] = q.x;
    P[2 * i + 1] = q.y;
  }
}
// sigma S and bias B of vehicle v of the noise row Z: 8-byte loads
__device__ __forceinline__ void noise_row_load(const double* Z, int v, double S[5], double B[5]) {
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    S[i] = Z[Z_SIGMA + v * 5 + i];
    B[i] = Z[Z_BIAS + v * 5 + i];
  }
}
// the stream id of scenario s as the counter's two words: streams[s], or s without a list
__device__ __forceinline__ void stream_words(const long long* streams, size_t s, uint32_t& t_lo, uint32_t& t_hi) {
  const unsigned long long t = streams ? (unsigned long long)streams[s] : (unsigned long long)s;
  t_lo = (uint32_t)t;
  t_hi = (uint32_t)(t >> 32);
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
// trunc: three Philox calls at counter (k, 4 v + j, t low, t high), each giving two normals
// (box_muller); the sixth normal is discarded.  raw (12 words, or nullptr) receives the calls' words.
// piadmm.obca.noise_tape is the same statements on the host; products and sums are kept apart (no
// contraction), so sigma = 0 gives the bias bit for bit.  The body of k_plan_noise (the in-plan step
// and the stand-alone tape) and of k_loop_close and k_loop_draw: the same bits.
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
    box_muller(c, z[2 * j], z[2 * j + 1]);
  }
#pragma unroll
  for (int i = 0; i < 5; ++i) {
    double zi = z[i];
    if (trunc != 0.0) zi = fmin(trunc, fmax(zi, -trunc));
    w[i] = B[i] + S[i] * zi;
  }
}

// The latency of vehicle v of stream t at step k under the row's avg, std, tau_max and trunc: one
// Philox call at counter (k, 4 v + 3, t low, t high) -- the call index the noise leaves free -- and
// the first of its two normals (box_muller); the second is discarded.  tape is the recorded latency
// added in front (0 without one).  raw (4 words, or nullptr) receives the call's words.
// piadmm.obca.delay_tau is the same statements on the host; products and sums are kept apart (no
// contraction), so std = 0 gives min(tau_max, tape + avg) bit for bit.  The body of k_plan_delay (the
// in-plan step and the stand-alone call), of k_loop_open and of k_loop_draw: the same bits.
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
  double z, unused;
  box_muller(c, z, unused);
  if (trunc != 0.0) z = fmin(trunc, fmax(z, -trunc));
  const double x = tape + (avg + sd * z);
  const double lo = x > 0.0 ? x : 0.0;
  return lo < tau_max ? lo : tau_max;
}

// ---------------------------------------------------------------------------------------------
// The host side: the launch views
// ---------------------------------------------------------------------------------------------
// what every view of a draw starts from: `rows` rows of `width` doubles at par, the stream ids, the key
inline draw_io draw_view(const double* par, int rows, int width, const long long* streams, uint64_t seed) {
  draw_io io{};
  io.par = par;  io.par_s = rows > 1 ? width : 0;
  io.streams = streams;
  io.seed_lo = (uint32_t)seed;  io.seed_hi = (uint32_t)(seed >> 32);
  return io;
}
// the plant step of the feedback `f` at its step `step` on the plan's own arrays: the tape's row as
// the disturbance (none without a tape)
inline plant_io feedback_view(const piadmm_obca_plan_s* p, const piadmm_obca_plan_s::feedback_s& f, int step) {
  plant_io io{};
  io.x0 = p->bar + S_INIT;  io.x0_s = STATE;
  io.ctrl = p->ctrl;  io.ctrl_s = NCTRL;  io.ctrl_v = NCTRL / 2;  io.ctrl_w = NT;
  io.par = f.par;  io.par_s = f.stride;
  io.w = f.tape ? f.tape + (size_t)step * 10 : nullptr;  io.w_s = (long long)f.cap * 10;
  io.out = f.next;
  return io;
}
// the disturbance rows of the noise `z` at step `step` of the feedback `f` into z.wbuf: the tape's
// row added in front
inline draw_io noise_view(const piadmm_obca_plan_s::noise_s& z, const piadmm_obca_plan_s::feedback_s& f, int step) {
  draw_io io = draw_view(z.par, z.rows, ZPAR, z.streams, z.seed);
  io.tape = f.tape ? f.tape + (size_t)step * 10 : nullptr;  io.tape_s = (long long)f.cap * 10;
  io.out = z.wbuf;  io.out_s = 10;
  io.k = (uint32_t)z.k0 + (uint32_t)step;
  return io;
}
// the latencies of the delay `d` at its step `step` into d.tau: the tape's row added in front
inline draw_io delay_view(const piadmm_obca_plan_s::delay_s& d, int step) {
  draw_io io = draw_view(d.par, d.rows, YPAR, d.streams, d.seed);
  io.tape = d.tape ? d.tape + (size_t)step * 2 : nullptr;  io.tape_s = (long long)d.cap * 2;
  io.out = d.tau;  io.out_s = 2;
  io.k = (uint32_t)d.k0 + (uint32_t)step;
  return io;
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

// The stand-alone draw of `cap` step indices from k0 for n scenarios on the caller's arrays (n x cap
// x dw doubles of out and tape, n x cap x rw words of raw; tape, raw nullptr: none): one grid row
// per step index, at most 32768 rows a launch, on the handle's stream; no synchronisation.
template <typename Kernel>
inline int draw_launch(piadmm_obca_t h, Kernel kernel, draw_io io, int n, int cap, int32_t k0, int dw, int rw,
                       double* out, const double* tape, uint32_t* raw) {
  io.tape_s = io.out_s = (long long)cap * dw;
  io.raw_s = (long long)cap * rw;
  for (int at = 0; at < cap; at += 32768) {
    const int ny = std::min(cap - at, 32768);
    io.out = out + (size_t)at * dw;
    io.tape = tape ? tape + (size_t)at * dw : nullptr;
    io.raw = raw ? raw + (size_t)at * rw : nullptr;
    io.k = (uint32_t)k0 + (uint32_t)at;
    hipLaunchKernelGGL(kernel, dim3(lane_blocks(2 * n), ny), dim3(64 * PW), 0, h->stream, (const int*)nullptr, n, io);
    OWN_HIP(h, hipGetLastError());
  }
  return 0;
}

// ---------------------------------------------------------------------------------------------
// The host side: the checks of the calls' arguments, each worded once; `who` is the call's name
// ---------------------------------------------------------------------------------------------
// `rows` rows of `width` doubles at par (nullptr: the kind is absent, nothing to check): 1 or n of
// them, every row through its kind's own check.  `kind` names the rows in a call that takes more
// than one kind ("plant", "noise", "delay"), else it is empty.
inline int rows_check(piadmm_obca_t h, const std::string& who, const char* kind, const double* par, int rows, int n,
                      int width, const char* (*check)(const double*)) {
  if (!par) return 0;
  const std::string item = who + ": " + kind + (*kind ? " " : "");
  if (rows != 1 && rows != n) return fail(h, PIADMM_E_ARG, item + "rows must be 1 or n (" + std::to_string(n) + ")");
  for (int k = 0; k < rows; ++k)
    if (const char* why = check(par + (size_t)k * width))
      return fail(h, PIADMM_E_ARG, item + "row " + std::to_string(k) + ": " + why);
  return 0;
}
// the stream ids (nullptr: the scenarios' numbers)
inline int streams_check(piadmm_obca_t h, const std::string& who, const int64_t* streams, int count) {
  if (streams)
    for (int k = 0; k < count; ++k)
      if (streams[k] < 0) return fail(h, PIADMM_E_ARG, who + ": streams[" + std::to_string(k) + "] must be >= 0");
  return 0;
}
// the step indices k0 .. k0 + steps - 1 of a noise or a delay
inline int step_index_check(piadmm_obca_t h, const std::string& who, int32_t k0, int64_t steps) {
  if (k0 < 0 || (int64_t)k0 + steps > ((int64_t)1 << 31))
    return fail(h, PIADMM_E_ARG, who + ": k0 >= 0 and every step index below 2^31");
  return 0;
}
// a tape of n x cap rows of `width` doubles (nullptr: none)
inline int tape_finite_check(piadmm_obca_t h, const std::string& who, const double* tape, int n, int cap, int width) {
  if (!tape) return 0;
  const size_t C = (size_t)cap, W = (size_t)width, T = (size_t)n * C * W;
  for (size_t i = 0; i < T; ++i)
    if (!std::isfinite(tape[i]))
      return fail(h, PIADMM_E_ARG, who + ": the tape of scenario " + std::to_string(i / (C * W)) +
                  " is not finite (step " + std::to_string(i / W % C) + ")");
  return 0;
}
// what an attachment uploads as its stream ids: the caller's, or 0 .. n - 1 without any
inline std::vector<long long> stream_ids(const int64_t* streams, size_t n) {
  std::vector<long long> ids(n);
  for (size_t k = 0; k < n; ++k) ids[k] = streams ? (long long)streams[k] : (long long)k;
  return ids;
}

}  // namespace obca_plan
