// piadmm_obca_plan_trace.hip -- what reads the device-resident OBCA-ADMM plan without changing it: the
// run record ("trace"), the clearance, the fleet statistics and the gather (gfx950).
// csrc/piadmm_obca_plan.hip describes the launch sequence; of it:
// With a trace attached (piadmm_obca_trace_begin) k_plan_trace and k_plan_clearance append the
// step's row to the device-side run record after k_plan_shift has closed an MPC step.
// The statistics of a run record (piadmm_obca_fleet_stats / _stats_trace: k_stats_fleet, k_stats_rows,
// k_stats_worst and their merges) and k_trace_gather are launched by those calls alone and write
// nothing of the plan or the trace.

#include "piadmm_obca_plan.h"

namespace obca_plan {

// ---------------------------------------------------------------------------------------------
// The run record ("trace") of an open plan: k_plan_trace copies a closed step's row, and
// k_plan_clearance measures how close the two vehicles are at the states the row holds.
// ---------------------------------------------------------------------------------------------

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

// One wave per scenario: clearance_pair (csrc/piadmm_obca_plan.h) at the state pair st[2][5] = states +
// s * stride, the plain and the tightened clearance into out[s].  With `summary`, lane 0 keeps the
// scenario's running minima: row 0 starts them, a later row replaces the plain minimum only when it
// is smaller, so the row kept is the first at which the minimum was reached.
__global__ void __launch_bounds__(64 * PW) k_plan_clearance(int n, const double* __restrict__ states, int stride,
                                                            const int* __restrict__ prob, double sigd, int row,
                                                            double* __restrict__ out,
                                                            double* __restrict__ summary) {
  const int lane = threadIdx.x & 63;
  const int s = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (s >= n) return;
  double plain, tight;
  clearance_pair(states + (size_t)s * stride, prob[s], sigd, lane, plain, tight);
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

using namespace obca_plan;

namespace obca_plan {
// Enqueues row `row` of the attached trace (0: the state it is attached at; rows + 1: the step
// k_plan_shift has just closed, on the same stream): the copies, then the clearances of the row's
// own states.  No synchronisation.
int trace_append(piadmm_obca_t h, piadmm_obca_plan_s* p, int row) {
  auto& t = p->tr;
  const size_t N = (size_t)p->n;
  hipLaunchKernelGGL(k_plan_trace, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->n, row, p->bar, p->iters,
                     p->mask, p->primal, p->dual, p->lamb, t.states, t.iters, t.mask, t.primal, t.dual, t.lamb,
                     t.summary);
  OWN_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_plan_clearance, dim3(blocks_for(p->n)), dim3(64 * PW), 0, h->stream, p->n,
                     t.states + (size_t)row * N * 10, 10, p->prob, p->sigd, row, t.clear + (size_t)row * N * 2,
                     t.summary);
  OWN_HIP(h, hipGetLastError());
  return 0;
}
}  // namespace obca_plan

namespace {
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }
}  // namespace

namespace obca_plan {
// what every statistics call checks of its arguments, before any device call
int stats_args_check(piadmm_obca_t h, const std::string& who, int n, const double* edges, int B, int K,
                     const stats_out& o) {
  if (B < 1 || B > PIADMM_OBCA_STATS_EDGES) return fail(h, PIADMM_E_ARG, who + ": 1 <= B <= 64");
  if (K < 1 || K > PIADMM_OBCA_STATS_WORST || K > n) return fail(h, PIADMM_E_ARG, who + ": 1 <= K <= min(64, n)");
  if (!edges || !o.stats || !o.hist || !o.row_min || !o.row_arg || !o.row_below || !o.worst)
    return fail(h, PIADMM_E_ARG, who + ": null argument");
  for (int k = 0; k < B; ++k) {
    if (!std::isfinite(edges[k])) return fail(h, PIADMM_E_ARG, who + ": edge " + std::to_string(k) + ": not finite");
    if (k > 0 && !(edges[k] > edges[k - 1]))
      return fail(h, PIADMM_E_ARG, who + ": edge " + std::to_string(k) + ": the edges must be strictly ascending");
  }
  return 0;
}

// The reductions over device arrays (clear (R + 1) x n x 2, summary n x 4, iters R x n, mask
// R x n x 2; the last two are not read for R = 0), on the handle's stream: one workspace for the
// edges, the partial records and the results, one copy of the results back, then into `o`.
int stats_run(piadmm_obca_t h, int R, int n, const double* d_clear, const double* d_summary, const int* d_iters,
              const int* d_mask, const double* edges, int B, int K, const stats_out& o) {
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
  std::vector<char> back(res_bytes);
  scratch sc(h);
  char* ws = sc.take<char>(total, false);
  if (sc.rc) return sc.rc;
  auto D = [&](size_t off) { return reinterpret_cast<double*>(ws + off); };
  auto I = [&](size_t off) { return reinterpret_cast<int*>(ws + off); };
  OWN_HIP(h, hipMemcpyAsync(ws + o_edges, edges, Bz * 8, hipMemcpyHostToDevice, h->stream));
  const stat_parts FP{D(f_min), I(f_arg), I(f_fin), I(f_bel)}, RP{D(r_min), I(r_arg), I(r_fin), I(r_bel)};
  const fleet_parts FF{reinterpret_cast<long long*>(ws + f_sum), I(f_max), I(f_or), I(f_flag)};
  hipLaunchKernelGGL(k_stats_fleet, dim3((unsigned)G), dim3(ST), 0, h->stream, n, R, d_summary, d_iters, d_mask,
                     (const double*)D(o_edges), B, FP, FF);
  OWN_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_stats_fleet_merge, dim3(1), dim3(ST), 0, h->stream, n, R, (int)G, B, FP, FF,
                     reinterpret_cast<piadmm_obca_stats_t*>(ws + o_res), reinterpret_cast<long long*>(ws + o_hist));
  OWN_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_stats_rows, dim3((unsigned)rows, (unsigned)G), dim3(ST), 0, h->stream, n, d_clear,
                     (const double*)D(o_edges), B, RP);
  OWN_HIP(h, hipGetLastError());
  hipLaunchKernelGGL(k_stats_rows_merge, dim3((unsigned)rows), dim3(ST), 0, h->stream, (int)G, B, RP, D(o_rmin),
                     I(o_rarg), I(o_rbel));
  OWN_HIP(h, hipGetLastError());
  // the first level reads the summary's plain minima once, ST a workgroup; every further level
  // merges WCAND / K lists a workgroup until one is left
  hipLaunchKernelGGL(k_stats_worst, dim3((unsigned)G), dim3(ST), 0, h->stream, d_summary, (int)TSUM,
                     (const int*)nullptr, n, (int)ST, K, D(w_v[0]), I(w_s[0]));
  OWN_HIP(h, hipGetLastError());
  int cur = 0;
  const int per_lists = WCAND / K;
  for (size_t lists = G; lists > 1; cur ^= 1) {
    const size_t next = (lists + per_lists - 1) / per_lists;
    hipLaunchKernelGGL(k_stats_worst, dim3((unsigned)next), dim3(ST), 0, h->stream, (const double*)D(w_v[cur]), 1,
                       (const int*)I(w_s[cur]), (int)(lists * Kz), per_lists * K, K, D(w_v[cur ^ 1]), I(w_s[cur ^ 1]));
    OWN_HIP(h, hipGetLastError());
    lists = next;
  }
  OWN_HIP(h, hipMemcpyAsync(ws + o_worst, ws + w_s[cur], Kz * 4, hipMemcpyDeviceToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(back.data(), ws, res_bytes, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  std::memcpy(o.stats, back.data() + o_res, sizeof(piadmm_obca_stats_t));
  std::memcpy(o.hist, back.data() + o_hist, 2 * (Bz + 1) * 8);
  std::memcpy(o.row_min, back.data() + o_rmin, rows * 2 * 8);
  std::memcpy(o.row_arg, back.data() + o_rarg, rows * 2 * 4);
  std::memcpy(o.row_below, back.data() + o_rbel, rows * 2 * Bz * 4);
  std::memcpy(o.worst, back.data() + o_worst, Kz * 4);
  return 0;
}
}  // namespace obca_plan

namespace {
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

int32_t piadmm_obca_clearance(piadmm_obca_t h, int32_t n, const double* states, const int32_t* prob, double* out) {
  if (!h) return PIADMM_E_ARG;
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_clearance: 1 <= n <= 2^20");
  if (!states || !prob || !out) return fail(h, PIADMM_E_ARG, "obca_clearance: null argument");
  for (int k = 0; k < n; ++k) {
    if (int rc = prob_check(h, "obca_clearance", prob, k)) return rc;
    for (int i = 0; i < 10; ++i)
      if (!std::isfinite(states[(size_t)k * 10 + i]))
        return fail(h, PIADMM_E_ARG, "obca_clearance: state pair " + std::to_string(k) + " is not finite");
  }
  OWN_HIP(h, hipSetDevice(h->device));
  const size_t N = (size_t)n;
  scratch a(h);
  double *d_st = a.take<double>(N * 10, false), *d_out = a.take<double>(N * 2, true);
  int* d_pr = a.take<int>(N, false);
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(d_st, states, N * 10 * sizeof(double), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(d_pr, prob, N * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_plan_clearance, dim3(blocks_for(n)), dim3(64 * PW), 0, h->stream, n, d_st, 10, d_pr,
                     std::sqrt(0.95 / (1.0 - 0.95)), 0, d_out, (double*)nullptr);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(out, d_out, N * 2 * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

int32_t piadmm_obca_trace_begin(piadmm_obca_t h, int32_t cap_steps, int32_t flags) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_trace_begin")) return rc;
  if (cap_steps < 1 || cap_steps > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_trace_begin: 1 <= cap_steps <= 2^20");
  if (flags & ~PIADMM_OBCA_TRACE_LAMBDA) return fail(h, PIADMM_E_ARG, "obca_trace_begin: unknown flag bits");
  if (p->lg.on) return fail(h, PIADMM_E_STATE, "obca_trace_begin: a ledger is attached (obca_ledger_end: the two do not record together)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_trace_begin: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  // the earlier record goes before the new one is built, not after it: the plan never holds two
  // records (peak device memory; a trace can be large), and a failure below leaves none attached
  p->tr = {};
  piadmm_obca_plan_s::trace_s t;
  const size_t N = (size_t)p->n, C = (size_t)cap_steps;
  int rc = 0;
  if ((rc = t.states.alloc(h, (C + 1) * N * 10, false)) || (rc = t.clear.alloc(h, (C + 1) * N * 2, false)) ||
      (rc = t.iters.alloc(h, C * N, false)) || (rc = t.mask.alloc(h, C * N * 2, false)) ||
      (rc = t.primal.alloc(h, C * N, false)) || (rc = t.dual.alloc(h, C * N, false)) ||
      (rc = t.summary.alloc(h, N * TSUM, true)) ||
      ((flags & PIADMM_OBCA_TRACE_LAMBDA) && (rc = t.lamb.alloc(h, C * N * 126, false))))
    return rc;
  t.cap = cap_steps;
  t.rows = 0;
  t.flags = flags;
  p->tr = std::move(t);      // not yet on: row 0 is written through the plan
  if ((rc = trace_append(h, p, 0))) {
    (void)hipStreamSynchronize(h->stream);
    p->tr = {};
    return rc;
  }
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  p->tr.on = true;
  return 0;
}

int32_t piadmm_obca_trace_run(piadmm_obca_t h, int32_t n_steps, int32_t* steps_done) {
  piadmm_obca_plan_s* p = nullptr;
  if (steps_done) *steps_done = 0;
  if (int rc = open_trace(h, &p, "obca_trace_run")) return rc;
  if (n_steps < 1) return fail(h, PIADMM_E_ARG, "obca_trace_run: n_steps >= 1");
  if ((int64_t)p->tr.rows + n_steps > p->tr.cap)
    return fail(h, PIADMM_E_STATE, "obca_trace_run: " + std::to_string(n_steps) + " steps do not fit the trace (" +
                std::to_string(p->tr.rows) + " of " + std::to_string(p->tr.cap) + " rows used)");
  // the steps fit the trace (above) and a trace excludes a ledger, so step_refusal names the tape, the
  // noise or the loop here; the delay excludes the loop, so its place behind them names what it named
  const char* why = step_refusal(p, n_steps);
  if (!why) why = delay_refusal(p, n_steps);
  if (why)
    return fail(h, PIADMM_E_STATE, std::string("obca_trace_run: ") + why + " before " + std::to_string(n_steps) + " steps" +
                (why == TAPE_EXHAUSTED
                     ? " (" + std::to_string(p->fb.steps) + " of " + std::to_string(p->fb.cap) + " rows used)"
                     : std::string()));
  if (p->ck.on) {
    // the steps the longest-lived scenario has left
    int left = 0;
    for (int s = 0; s < p->n; ++s)
      if (p->ck.host[3 * (size_t)s + 2])
        left = std::max(left, p->ck.host[3 * (size_t)s + 1] - 8 - p->ck.host[3 * (size_t)s] + 1);
    if (left == 0) return fail(h, PIADMM_E_STATE, "obca_trace_run: no scenario alive");
    if (n_steps > left)
      return fail(h, PIADMM_E_STATE, "obca_trace_run: every reference ends before " + std::to_string(n_steps) +
                  " steps (" + std::to_string(left) + " left)");
  } else if ((int64_t)p->t_step + n_steps - 1 + 8 > p->cfg.n_ref)
    return fail(h, PIADMM_E_STATE, "obca_trace_run: the reference ends before " + std::to_string(n_steps) + " steps");
  // a host loop of the plan's bounded launches: every step ends in piadmm_obca_plan_shift, which appends its row
  for (int k = 0; k < n_steps; ++k) {
    if (int rc = piadmm_obca_plan_step(h, nullptr)) return rc;
    if (steps_done) *steps_done = k + 1;
  }
  return 0;
}

int32_t piadmm_obca_trace_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes) {
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
      if (!t.lamb) return fail(h, PIADMM_E_STATE, "obca_trace_get: the trace keeps no lamb_bar (PIADMM_OBCA_TRACE_LAMBDA)");
      src = t.lamb; want = R * n * 126 * D; break;
    case PIADMM_OBCA_TRACE_GET_SUMMARY: src = t.summary; want = n * TSUM * D; break;
    case PIADMM_OBCA_TRACE_GET_ROWS: src = &t.rows; want = I; break;
    default: return fail(h, PIADMM_E_ARG, "obca_trace_get: unknown item " + std::to_string(what));
  }
  return get_finish(h, "obca_trace_get", what, src, what == PIADMM_OBCA_TRACE_GET_ROWS, want, out, bytes);
}

int32_t piadmm_obca_trace_end(piadmm_obca_t h) {
  if (!h) return PIADMM_E_ARG;
  if (!h->plan || !h->plan->tr.on) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->plan->tr = {};
  return 0;
}

int32_t piadmm_obca_stats_size(void) { return (int32_t)sizeof(piadmm_obca_stats_t); }

int32_t piadmm_obca_fleet_stats(piadmm_obca_t h, int32_t rows_R, int32_t n, const double* clear, const double* summary,
                                const int32_t* iters, const int32_t* mask, const double* edges, int32_t B, int32_t K,
                                piadmm_obca_stats_t* stats, int64_t* hist, double* row_min, int32_t* row_arg,
                                int32_t* row_below, int32_t* worst) {
  if (!h) return PIADMM_E_ARG;
  const std::string who = "obca_fleet_stats";
  if (n < 1 || n > (1 << 20)) return fail(h, PIADMM_E_ARG, who + ": 1 <= n <= 2^20");
  if (rows_R < 0 || rows_R > (1 << 20)) return fail(h, PIADMM_E_ARG, who + ": 0 <= rows_R <= 2^20");
  if (!clear || !summary || (rows_R > 0 && (!iters || !mask))) return fail(h, PIADMM_E_ARG, who + ": null argument");
  const stats_out o{stats, hist, row_min, row_arg, row_below, worst};
  if (int rc = stats_args_check(h, who, n, edges, B, K, o)) return rc;
  for (int k = 0; k < n; ++k) {
    const double v = summary[(size_t)k * TSUM + 3];
    if (!(v >= 0.0 && v <= 1099511627776.0 && v == std::floor(v)))
      return fail(h, PIADMM_E_ARG, who + ": row " + std::to_string(k) + ": the sum of iterates must be an integer in [0, 2^40]");
  }
  OWN_HIP(h, hipSetDevice(h->device));
  const size_t N = (size_t)n, R = (size_t)rows_R;
  const size_t b_clear = (R + 1) * N * 2 * 8, b_sum = N * TSUM * 8, b_it = R * N * 4, b_mask = R * N * 2 * 4;
  const size_t o_sum = up256(b_clear), o_it = o_sum + up256(b_sum), o_mask = o_it + up256(b_it);
  scratch a(h);
  char* in = a.take<char>(o_mask + up256(b_mask) + 256, false);
  if (a.rc) return a.rc;
  OWN_HIP(h, hipMemcpyAsync(in, clear, b_clear, hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(in + o_sum, summary, b_sum, hipMemcpyHostToDevice, h->stream));
  if (R) {
    OWN_HIP(h, hipMemcpyAsync(in + o_it, iters, b_it, hipMemcpyHostToDevice, h->stream));
    OWN_HIP(h, hipMemcpyAsync(in + o_mask, mask, b_mask, hipMemcpyHostToDevice, h->stream));
  }
  return stats_run(h, rows_R, n, reinterpret_cast<const double*>(in), reinterpret_cast<const double*>(in + o_sum),
                   reinterpret_cast<const int*>(in + o_it), reinterpret_cast<const int*>(in + o_mask), edges, B, K, o);
}

int32_t piadmm_obca_stats_trace(piadmm_obca_t h, const double* edges, int32_t B, int32_t K, piadmm_obca_stats_t* stats,
                                int64_t* hist, double* row_min, int32_t* row_arg, int32_t* row_below, int32_t* worst) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_trace(h, &p, "obca_stats_trace")) return rc;
  const stats_out o{stats, hist, row_min, row_arg, row_below, worst};
  if (int rc = stats_args_check(h, "obca_stats_trace", p->n, edges, B, K, o)) return rc;
  OWN_HIP(h, hipSetDevice(h->device));
  const auto& t = p->tr;
  return stats_run(h, t.rows, p->n, t.clear, t.summary, t.iters, t.mask, edges, B, K, o);
}

int32_t piadmm_obca_gather_trace_bytes(piadmm_obca_t h, int32_t m, int64_t* bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_trace(h, &p, "obca_gather_trace_bytes")) return rc;
  if (m < 1 || m > p->n) return fail(h, PIADMM_E_ARG, "obca_gather_trace_bytes: 1 <= m <= n_scenarios");
  if (!bytes) return fail(h, PIADMM_E_ARG, "obca_gather_trace_bytes: null argument");
  *bytes = gather_offsets(p->tr.rows, m, p->tr.lamb != nullptr).bytes;
  return 0;
}

int32_t piadmm_obca_gather_trace(piadmm_obca_t h, int32_t m, const int32_t* slots, void* blob, int64_t bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_trace(h, &p, "obca_gather_trace")) return rc;
  if (int rc = tenant_slots_check(h, p, m, slots, blob, "obca_gather_trace")) return rc;
  const auto& t = p->tr;
  const gather_layout g = gather_offsets(t.rows, m, t.lamb != nullptr);
  if (bytes != g.bytes)
    return fail(h, PIADMM_E_ARG, "obca_gather_trace: the blob is " + std::to_string(g.bytes) + " bytes, not " +
                std::to_string(bytes));
  const int64_t waves = ((int64_t)t.rows + 1) * m, blocks = (waves + PW - 1) / PW;
  if (blocks > INT_MAX) return fail(h, PIADMM_E_ARG, "obca_gather_trace: (rows + 1) m must stay below 2^33");
  OWN_HIP(h, hipSetDevice(h->device));
  if (int rc = stage_ensure(h, p, (size_t)g.bytes, m)) return rc;
  char* st = p->stg.buf;
  int* d_list = reinterpret_cast<int*>(st + g.bytes);
  auto D = [&](int64_t off) { return reinterpret_cast<double*>(st + off); };
  const gather_src a{t.states, t.clear, t.primal, t.dual, t.lamb, t.summary, t.iters, t.mask};
  const gather_dst d{D(g.states), D(g.clear), D(g.primal), D(g.dual), D(g.summary), D(g.lamb),
                     reinterpret_cast<int*>(st + g.iters), reinterpret_cast<int*>(st + g.mask)};
  OWN_HIP(h, hipMemcpyAsync(d_list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  // the pad word between STATUS_MASK and LAMBDA has no writer: it goes out as 0
  if (g.lamb != g.mask + 8 * (int64_t)t.rows * m) OWN_HIP(h, hipMemsetAsync(st + g.lamb - 4, 0, 4, h->stream));
  hipLaunchKernelGGL(k_trace_gather, dim3((unsigned)blocks), dim3(64 * PW), 0, h->stream, (const int*)d_list, m, p->n,
                     t.rows + 1, a, d);
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipMemcpyAsync(blob, st, (size_t)g.bytes, hipMemcpyDeviceToHost, h->stream));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"
