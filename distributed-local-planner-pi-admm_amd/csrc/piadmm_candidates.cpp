// piadmm_candidates.cpp -- candidate pairs on a uniform grid hash (C-ABI of libpiadmm, piadmm_ctx.h).
#include "piadmm_ctx.h"

namespace {
// the events around the two phases (ms_out)
struct four_events {
  hipEvent_t e[4] = {};
  four_events() {
    for (auto& x : e) (void)hipEventCreate(&x);
  }
  four_events(const four_events&) = delete;
  four_events& operator=(const four_events&) = delete;
  ~four_events() {
    for (auto& x : e) (void)hipEventDestroy(x);
  }
};
}  // namespace

extern "C" {

// Candidate pairs on a uniform grid hash (piadmm_detect.hip; casadi/main.py:110-113 at O(N)).
int32_t piadmm_candidate_pairs(piadmm_handle_t h, const double* xy, const double* radius, int32_t n,
                               int32_t* pairs_out, int32_t max_pairs, int32_t* n_pairs_out, float* ms_out) {
  if (!h || !n_pairs_out || (n > 0 && (!xy || !radius))) return fail(h, PIADMM_E_ARG, "null argument");
  if (n < 0 || n > (1 << 25)) return fail(h, PIADMM_E_ARG, "n must be in [0, 2^25]");
  if (max_pairs < 0 || (max_pairs > 0 && !pairs_out)) return fail(h, PIADMM_E_ARG, "bad pairs_out / max_pairs");
  *n_pairs_out = 0;
  if (ms_out) *ms_out = 0.0f;
  if (n == 0) return PIADMM_OK;
  (void)hipGetLastError();   // a stale error of an earlier runtime call is not this call's
  double rmax = 0.0;
  for (int i = 0; i < n; ++i) {
    if (!std::isfinite(xy[2 * i]) || !std::isfinite(xy[2 * i + 1]) || !std::isfinite(radius[i]) || radius[i] < 0)
      return fail(h, PIADMM_E_ARG, "positions and radii must be finite, radii >= 0");
    rmax = std::max(rmax, radius[i]);
  }
  // cell size >= 2 max r (a candidate pair is in the same or an adjacent cell), with margin for
  // the rounding of x / cs; buckets: a power of two >= 2n
  const double cs = rmax > 0 ? 2.0 * rmax * (1.0 + 1e-9) : 1.0;
  unsigned T = 1024;
  while (T < 2u * (unsigned)n) T <<= 1;
  HIPCHK(h, hipSetDevice(h->cfg.device));
  hipStream_t s = h->stream;
  // the events, then the arrays: when the call leaves, on whichever path, the arena synchronises the
  // stream and frees the arrays, and then the events go
  four_events ev;
  pd_own::arena<piadmm_ctx> tmp(h);
  double* d_xy = tmp.take<double>((size_t)n * 2, false);
  double* d_r = tmp.take<double>((size_t)n, false);
  unsigned* d_key = tmp.take<unsigned>((size_t)n, false);
  int* d_cnt = tmp.take<int>((size_t)T, false);
  int* d_fill = tmp.take<int>((size_t)T, false);
  int* d_start = tmp.take<int>((size_t)T + 1, false);
  int* d_order = tmp.take<int>((size_t)n, false);
  int* d_pcnt = tmp.take<int>((size_t)n, false);
  int* d_off = tmp.take<int>((size_t)n + 1, false);
  long long* d_total = tmp.take<long long>(1, false);
  long long* d_bsum = tmp.take<long long>((size_t)T / pd::DETECT_SCAN_B + 2, false);   // T >= n: the larger scan
  double* d_xs = tmp.take<double>((size_t)n * 2, false);                     // bucket-ordered copies
  double* d_rs = tmp.take<double>((size_t)n, false);
  if (tmp.rc) return fail(h, PIADMM_E_HIP, "hipMalloc failed (candidate pairs)");
  hipEvent_t* e = ev.e;
  int rc = 0;
  long long total = 0;
  rc |= hipMemcpyAsync(d_xy, xy, (size_t)n * 2 * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess;
  rc |= hipMemcpyAsync(d_r, radius, (size_t)n * sizeof(double), hipMemcpyHostToDevice, s) != hipSuccess;
  rc |= hipEventRecord(e[0], s) != hipSuccess;
  rc |= pd::launch_detect_count(d_xy, d_r, n, 1.0 / cs, T, d_key, d_cnt, d_start, d_fill, d_order, d_pcnt, d_off,
                                d_total, d_bsum, d_xs, d_rs, s) != 0;
  rc |= hipEventRecord(e[1], s) != hipSuccess;
  rc |= hipMemcpyAsync(&total, d_total, sizeof(long long), hipMemcpyDeviceToHost, s) != hipSuccess;
  rc |= hipStreamSynchronize(s) != hipSuccess;
  if (rc) return fail(h, PIADMM_E_HIP, "candidate pairs: count phase failed");
  if (total > 0x7fffffffll / 2) return fail(h, PIADMM_E_ARG, "candidate pairs: more than 2^30 pairs");
  int* d_out = tmp.take<int>((size_t)total * 2, false);
  if (!d_out) return fail(h, PIADMM_E_HIP, "hipMalloc failed (candidate pairs output)");
  rc |= hipEventRecord(e[2], s) != hipSuccess;
  rc |= pd::launch_detect_emit(d_xs, d_rs, n, 1.0 / cs, T, d_start, d_order, d_off, d_out, s) != 0;
  rc |= hipEventRecord(e[3], s) != hipSuccess;
  const long long ncopy = std::min<long long>(total, max_pairs);
  if (ncopy > 0)
    rc |= hipMemcpyAsync(pairs_out, d_out, (size_t)ncopy * 2 * sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess;
  rc |= hipStreamSynchronize(s) != hipSuccess;
  float m1 = 0.0f, m2 = 0.0f;
  if (!rc && ms_out && hipEventElapsedTime(&m1, e[0], e[1]) == hipSuccess &&
      hipEventElapsedTime(&m2, e[2], e[3]) == hipSuccess)
    *ms_out = m1 + m2;
  if (rc) return fail(h, PIADMM_E_HIP, "candidate pairs: emit phase failed");
  *n_pairs_out = (int32_t)total;
  return PIADMM_OK;
}

}  // extern "C"
