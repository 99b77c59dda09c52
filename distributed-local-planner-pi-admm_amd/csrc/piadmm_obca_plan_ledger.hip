// piadmm_obca_plan_ledger.hip -- the tenant ledger of the device-resident OBCA-ADMM plan: one risk record
// per tenant, kept on the device while the tenant runs and appended when it leaves its slot (gfx950).
// csrc/piadmm_obca_plan.hip describes the launch sequence; of it:
// With a ledger attached (piadmm_obca_ledger_begin; a clocked plan only) piadmm_obca_plan_shift runs
// k_ledger_step on the scenarios the step ran, after the shift (and, under the loop, after
// k_plan_set_init) and before the tick: the update of their open records and the append of the ones
// the tick retires.  piadmm_obca_clock_admit, _loop_admit and _tenant_import run k_ledger_close before
// they overwrite a slot and k_ledger_open after it; piadmm_obca_ledger_stats runs k_ledger_view and the
// statistics' kernels.  Without a ledger none is launched.
//
// A record is LREC = 22 words of 8 bytes (include/piadmm.h).  Where the clearance is computed one wave
// serves one scenario in the lane layout of k_plan_clearance (clearance_pair, csrc/piadmm_obca_plan.h);
// lane w < 22 then owns word w of the scenario's record, the open one and the appended one alike, so
// every word has one writer.  No LDS, no atomic, no wait for another workgroup: a position in the
// ledger is the host's count plus the number of retirees before the scenario in the ascending list the
// step ran, counted by the wave itself, or a number the host uploads (an admission).

#include "piadmm_obca_plan.h"

namespace obca_plan {

__device__ __forceinline__ long long pack2(int lo, int hi) {
  return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ int lo32(long long w) { return (int)(unsigned)((unsigned long long)w & 0xffffffffull); }
__device__ __forceinline__ int hi32(long long w) { return (int)(unsigned)((unsigned long long)w >> 32); }

// One wave per entry k of `list`: a fresh open record of slot list[k] for the tenant ids[k], at the
// slot's clock and init_state, whose two clearances start the minima.  ids[k] < 0: the slot holds no
// tenant (id -1, the other words as a record without a step).  streams nullptr: no loop, stream -1.
__global__ void __launch_bounds__(64 * PW) k_ledger_open(const int* __restrict__ list,
                                                         const long long* __restrict__ ids, int m,
                                                         const double* __restrict__ bar, const int* __restrict__ prob,
                                                         double sigd, const int* __restrict__ clk,
                                                         const long long* __restrict__ streams,
                                                         long long* __restrict__ run) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= m) return;
  const int s = __builtin_amdgcn_readfirstlane(list[k]);
  const double* st = bar + (size_t)s * STATE + S_INIT;
  double plain, tight;
  clearance_pair(st, prob[s], sigd, lane, plain, tight);
  if (lane >= LREC) return;
  const long long id = ids[k];
  const int c = clk[3 * (size_t)s];
  long long w = 0;
  if (lane == L_ID) w = id < 0 ? -1 : id;
  else if (lane == L_STREAM) w = streams ? streams[s] : -1;
  else if (lane == L_SLOT) w = pack2(s, 0);
  else if (lane == L_FIRST) w = pack2(c, 0);
  else if (lane == L_PLAIN) w = __double_as_longlong(plain);
  else if (lane == L_TIGHT) w = __double_as_longlong(tight);
  else if (lane == L_CMIN) w = pack2(c, 0);
  else if (lane == L_PRIMAL || lane == L_DUAL) w = __double_as_longlong(0.0);
  else if (lane == L_TSTEP) w = pack2(-1, 0);
  else if (lane >= L_STATE) w = __double_as_longlong(st[lane - L_STATE]);
  run[(size_t)s * LREC + lane] = w;
}

// true when the tick that follows retires a scenario at clock c with len rows: k_plan_clock's rule at c + 1
__device__ __forceinline__ bool retires(int c, int len) { return c + 1 > len - 8; }

// One wave per entry k of `list`, the scenarios the closing step ran, ascending, before the tick: the
// open record of scenario s takes the step -- steps + 1, the new init_state and its two clearances (the
// plain minimum replaced only by a smaller one, with the clock c + 1 of that state: the first at which
// it was reached), the stop iterate into the largest and the sum, both masks into the ORs, the stopping
// iterate's residuals, the stream id it runs under.  A scenario the tick retires is appended to `rec`
// with reason 1 and the plan's step t_step, and its slot's open record says "no tenant" (id -1).  Its
// position is base + the number of retirees before it in the list, which the wave counts over the
// entries in front of it (ballot and popcount, uniform): ascending by slot, whatever order the waves run in.
__global__ void __launch_bounds__(64 * PW) k_ledger_step(const int* __restrict__ list, int m,
                                                         const double* __restrict__ bar, const int* __restrict__ prob,
                                                         double sigd, const int* __restrict__ clk,
                                                         const long long* __restrict__ streams,
                                                         const int* __restrict__ iters, const int* __restrict__ mask,
                                                         const double* __restrict__ primal,
                                                         const double* __restrict__ dual, int base, int cap, int t_step,
                                                         long long* run, long long* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= m) return;
  const int s = __builtin_amdgcn_readfirstlane(list[k]);
  const double* st = bar + (size_t)s * STATE + S_INIT;
  double plain, tight;
  clearance_pair(st, prob[s], sigd, lane, plain, tight);
  const int c1 = __builtin_amdgcn_readfirstlane(clk[3 * (size_t)s]) + 1;
  const bool out = retires(c1 - 1, __builtin_amdgcn_readfirstlane(clk[3 * (size_t)s + 1]));
  int pos = base;
  if (out) {
    for (int start = 0; start < k; start += 64) {
      const int j = start + lane;
      bool f = false;
      if (j < k) {
        const size_t q = (size_t)list[j];
        f = retires(clk[3 * q], clk[3 * q + 1]);
      }
      pos += __popcll(__ballot(f));
    }
  }
  // every lane is here again; lane w owns word w.  The old plain minimum decides word L_CMIN as well
  long long* R = run + (size_t)s * LREC;
  const long long old = lane < LREC ? R[lane] : 0;
  const double old_plain = __longlong_as_double(__shfl(old, L_PLAIN, 64));
  if (lane >= LREC) return;
  const int it = iters[s];
  long long w = old;
  if (lane == L_STREAM) w = streams ? streams[s] : -1;
  else if (lane == L_FIRST) w = pack2(lo32(old), hi32(old) + 1);
  else if (lane == L_PLAIN) w = plain < old_plain ? __double_as_longlong(plain) : old;
  else if (lane == L_TIGHT) w = tight < __longlong_as_double(old) ? __double_as_longlong(tight) : old;
  else if (lane == L_CMIN) w = pack2(plain < old_plain ? c1 : lo32(old), max(hi32(old), it));
  else if (lane == L_SUM) w = old + (long long)it;
  else if (lane == L_MASK) w = pack2(lo32(old) | mask[2 * (size_t)s], hi32(old) | mask[2 * (size_t)s + 1]);
  else if (lane == L_PRIMAL) w = __double_as_longlong(primal[s]);
  else if (lane == L_DUAL) w = __double_as_longlong(dual[s]);
  else if (lane >= L_STATE) w = __double_as_longlong(st[lane - L_STATE]);
  if (out && pos >= 0 && pos < cap) {
    long long a = w;
    if (lane == L_SLOT) a = pack2(s, 1);
    else if (lane == L_TSTEP) a = pack2(t_step, 0);
    rec[(size_t)pos * LREC + lane] = a;
  }
  R[lane] = (out && lane == L_ID) ? -1 : w;
}

// One wave per entry k of `list`, before an admission or an import overwrites the slots: pos[k] >= 0
// appends the open record of slot list[k] at that position (the host's mirror chose it) with `reason`,
// the plan's step and the stream id the tenant ran under, and the slot then holds no tenant.
__global__ void __launch_bounds__(64 * PW) k_ledger_close(const int* __restrict__ list, const int* __restrict__ pos,
                                                          int m, int cap, int reason, int t_step,
                                                          const long long* __restrict__ streams, long long* run,
                                                          long long* __restrict__ rec) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * PW + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (k >= m) return;
  const int s = __builtin_amdgcn_readfirstlane(list[k]);
  const int at = __builtin_amdgcn_readfirstlane(pos[k]);
  if (at < 0 || at >= cap || lane >= LREC) return;
  long long* R = run + (size_t)s * LREC;
  long long w = R[lane];
  if (lane == L_STREAM) w = streams ? streams[s] : -1;
  else if (lane == L_SLOT) w = pack2(s, reason);
  else if (lane == L_TSTEP) w = pack2(t_step, 0);
  rec[(size_t)at * LREC + lane] = w;
  if (lane == L_ID) R[lane] = -1;
}

// One lane per (record r, word j) of the statistics' view of `count` appended records, R = 1: summary
// (count x 4: min plain, c_min, min tight, the iterate sum), clear (2 x count x 2: both rows the
// minima), iters (1 x count: the largest stop iterate), mask (1 x count x 2: the two ORs).
__global__ void __launch_bounds__(64 * PW) k_ledger_view(const long long* __restrict__ rec, int count,
                                                         double* __restrict__ summary, double* __restrict__ clear,
                                                         int* __restrict__ iters, int* __restrict__ mask) {
  const long long g = (long long)blockIdx.x * (64 * PW) + threadIdx.x;
  if (g >= (long long)count * LVIEW) return;
  const size_t r = (size_t)(g / LVIEW), C = (size_t)count;
  const int j = (int)(g % LVIEW);
  const long long* R = rec + r * LREC;
  if (j == 0) summary[r * TSUM] = __longlong_as_double(R[L_PLAIN]);
  else if (j == 1) summary[r * TSUM + 1] = (double)lo32(R[L_CMIN]);
  else if (j == 2) summary[r * TSUM + 2] = __longlong_as_double(R[L_TIGHT]);
  else if (j == 3) summary[r * TSUM + 3] = (double)R[L_SUM];
  else if (j < 8) {
    const int row = (j - 4) >> 1, kk = (j - 4) & 1;
    clear[(row * C + r) * 2 + kk] = __longlong_as_double(R[kk ? L_TIGHT : L_PLAIN]);
  } else if (j == 8) iters[r] = hi32(R[L_CMIN]);
  else mask[2 * r + (j - 9)] = j == 9 ? lo32(R[L_MASK]) : hi32(R[L_MASK]);
}

}  // namespace obca_plan

using namespace obca_plan;

namespace obca_plan {

// the tenants the next `steps` MPC steps retire, by the mirror of the clocks
static int ledger_retirees(const piadmm_obca_plan_s* p, int64_t steps) {
  int r = 0;
  for (int s = 0; s < p->n; ++s) {
    const int* k = p->ck.host.data() + 3 * (size_t)s;
    if (k[2] && (int64_t)k[1] - 8 - k[0] + 1 <= steps) r += 1;
  }
  return r;
}

// What refuses the next `steps` MPC steps of a plan with a ledger, or nullptr: every tenant they retire
// needs a place
const char* ledger_refusal(const piadmm_obca_plan_s* p, int64_t steps) {
  if (!p->lg.on || !p->ck.on) return nullptr;
  return (int64_t)p->lg.count + ledger_retirees(p, steps) > p->lg.cap ? "ledger full" : nullptr;
}

static const long long* ledger_streams(const piadmm_obca_plan_s* p) {
  return p->lp.on ? (const long long*)p->lp.streams : nullptr;
}

// What clock_shift enqueues for the ledger, after the shift has written the new init_state (under the
// loop: after k_plan_set_init) and before the tick: one launch over ck.list, no synchronisation.
int ledger_step(piadmm_obca_t h, piadmm_obca_plan_s* p) {
  const int m = p->ck.n_list;
  if (m <= 0) return 0;
  auto& l = p->lg;
  hipLaunchKernelGGL(k_ledger_step, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, (const int*)p->ck.list, m,
                     (const double*)p->bar, (const int*)p->prob, p->sigd, (const int*)p->ck.clk, ledger_streams(p),
                     (const int*)p->iters, (const int*)p->mask, (const double*)p->primal, (const double*)p->dual,
                     l.count, l.cap, p->t_step, l.run.get(), l.rec.get());
  OWN_HIP(h, hipGetLastError());
  return 0;
}

// The mirror after that shift: `next` is the clocks' mirror after the tick (ck.host still the one before)
void ledger_stepped(piadmm_obca_plan_s* p, const std::vector<int>& next) {
  auto& l = p->lg;
  for (int s = 0; s < p->n; ++s)
    if (p->ck.host[3 * (size_t)s + 2] && !next[3 * (size_t)s + 2]) {
      l.count += 1;
      l.id[(size_t)s] = -1;
    }
}

// true when the call appends the tenant of slot s before it overwrites the slot: it is alive, and with
// keep_fresh (piadmm_obca_loop_admit: the second half of an admission) it has closed a step
static bool ledger_closes(const piadmm_obca_plan_s* p, int s, bool keep_fresh) {
  const int* k = p->ck.host.data() + 3 * (size_t)s;
  if (p->lg.id[(size_t)s] < 0 || !k[2]) return false;
  return !keep_fresh || k[0] != p->lg.c_first[(size_t)s];
}

// What refuses an admission or an import into `slots` of a plan with a ledger, or nullptr
const char* ledger_replace_refusal(const piadmm_obca_plan_s* p, int m, const int32_t* slots, bool keep_fresh) {
  if (!p->lg.on || !p->ck.on) return nullptr;
  int64_t closed = 0;
  for (int k = 0; k < m; ++k) closed += ledger_closes(p, slots[k], keep_fresh) ? 1 : 0;
  return (int64_t)p->lg.count + closed > p->lg.cap ? "ledger full" : nullptr;
}

// Before the slots are overwritten: the alive tenants' open records appended with `reason`, in the
// order of `slots` (ledger_replace_refusal has passed).  Synchronises: the caller's copies go through
// the null stream.
int ledger_close(piadmm_obca_t h, piadmm_obca_plan_s* p, int m, const int32_t* slots, int reason, bool keep_fresh) {
  auto& l = p->lg;
  std::vector<int> pos((size_t)m, -1);
  int at = l.count;
  for (int k = 0; k < m; ++k)
    if (ledger_closes(p, slots[k], keep_fresh)) pos[(size_t)k] = at++;
  if (at == l.count) return 0;
  OWN_HIP(h, hipMemcpyAsync(l.list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(l.pos, pos.data(), (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_ledger_close, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, (const int*)l.list,
                     (const int*)l.pos, m, l.cap, reason, p->t_step, ledger_streams(p), l.run.get(), l.rec.get());
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < m; ++k)
    if (pos[(size_t)k] >= 0) l.id[(size_t)slots[k]] = -1;
  l.count = at;
  return 0;
}

// After the slots hold their new tenants and the clocks' mirror is up to date: a fresh open record for
// every alive one, in the order of `slots`; a tenant ledger_close kept keeps its id, every other takes
// the next.  A slot that is not alive holds no tenant.  Synchronises.
int ledger_open(piadmm_obca_t h, piadmm_obca_plan_s* p, int m, const int32_t* slots) {
  auto& l = p->lg;
  std::vector<long long> ids((size_t)m, -1);
  long long next = l.next_id;
  for (int k = 0; k < m; ++k) {
    const size_t s = (size_t)slots[k];
    if (p->ck.host[3 * s + 2]) ids[(size_t)k] = l.id[s] >= 0 ? l.id[s] : next++;
  }
  OWN_HIP(h, hipMemcpyAsync(l.list, slots, (size_t)m * sizeof(int), hipMemcpyHostToDevice, h->stream));
  OWN_HIP(h, hipMemcpyAsync(l.ids, ids.data(), (size_t)m * sizeof(long long), hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_ledger_open, dim3(blocks_for(m)), dim3(64 * PW), 0, h->stream, (const int*)l.list,
                     (const long long*)l.ids, m, (const double*)p->bar, (const int*)p->prob, p->sigd,
                     (const int*)p->ck.clk, ledger_streams(p), l.run.get());
  OWN_HIP(h, hipGetLastError());
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  for (int k = 0; k < m; ++k) {
    const size_t s = (size_t)slots[k];
    l.id[s] = ids[(size_t)k];
    l.c_first[s] = p->ck.host[3 * s];
  }
  l.next_id = next;
  return 0;
}

}  // namespace obca_plan

namespace {
size_t up256(size_t v) { return (v + 255) & ~(size_t)255; }

int open_ledger(piadmm_obca_t h, piadmm_obca_plan_s** out, const char* who) {
  if (int rc = open_plan(h, out, who)) return rc;
  if (!(*out)->lg.on) return fail(h, PIADMM_E_STATE, std::string(who) + ": no ledger attached (obca_ledger_begin)");
  return 0;
}
}  // namespace

extern "C" {

int32_t piadmm_obca_ledger_begin(piadmm_obca_t h, int32_t cap_tenants, int32_t flags) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_plan(h, &p, "obca_ledger_begin")) return rc;
  if (cap_tenants < 1 || cap_tenants > (1 << 20)) return fail(h, PIADMM_E_ARG, "obca_ledger_begin: 1 <= cap_tenants <= 2^20");
  if (flags != 0) return fail(h, PIADMM_E_ARG, "obca_ledger_begin: flags must be 0");
  if (!p->ck.on) return fail(h, PIADMM_E_STATE, "obca_ledger_begin: no clock attached (obca_clock_plan: a record opens and closes by the tenant's clock)");
  if (p->tr.on) return fail(h, PIADMM_E_STATE, "obca_ledger_begin: a trace is attached (obca_trace_end: the two do not record together)");
  if (p->i_iter != 0) return fail(h, PIADMM_E_STATE, "obca_ledger_begin: only at a step boundary (an MPC step is open)");
  OWN_HIP(h, hipSetDevice(h->device));
  OWN_HIP(h, hipStreamSynchronize(h->stream));
  // the new ledger is built and its open records written before the earlier one goes: a failure on the
  // way leaves the earlier one attached, as it was
  piadmm_obca_plan_s::ledger_s l;
  const size_t N = (size_t)p->n;
  int rc = 0;
  if ((rc = l.rec.alloc(h, (size_t)cap_tenants * LREC, false)) || (rc = l.run.alloc(h, N * LREC, false)) ||
      (rc = l.ids.alloc(h, N, false)) || (rc = l.list.alloc(h, N, false)) || (rc = l.pos.alloc(h, N, false)))
    return rc;
  piadmm_obca_plan_s::ledger_s earlier = std::move(p->lg);
  l.cap = cap_tenants;
  l.count = 0;
  l.next_id = (long long)p->n;
  l.id.assign(N, -1);
  l.c_first.assign(N, 0);
  p->lg = std::move(l);      // not yet on: the open records are written through the plan
  // every alive slot's tenant takes its slot number, every other slot holds none
  for (size_t s = 0; s < N; ++s)
    if (p->ck.host[3 * s + 2]) p->lg.id[s] = (long long)s;
  const std::vector<int> ident = identity_list(N);
  if ((rc = ledger_open(h, p, p->n, ident.data()))) {
    (void)hipStreamSynchronize(h->stream);
    p->lg = std::move(earlier);
    return rc;
  }
  p->lg.next_id = (long long)p->n;
  p->lg.on = true;
  return 0;
}

int32_t piadmm_obca_ledger_get(piadmm_obca_t h, int32_t what, void* out, int64_t bytes) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_ledger(h, &p, "obca_ledger_get")) return rc;
  const auto& l = p->lg;
  const int32_t count = l.count;
  const int64_t next_id = l.next_id;
  const void* src = nullptr;
  int64_t want = -1;
  bool host = false;
  switch (what) {
    case PIADMM_OBCA_LEDGER_GET_COUNT: src = &count; want = sizeof(int32_t); host = true; break;
    case PIADMM_OBCA_LEDGER_GET_RECORDS: src = l.rec; want = (int64_t)l.count * PIADMM_OBCA_LEDGER_REC; break;
    case PIADMM_OBCA_LEDGER_GET_RUNNING: src = l.run; want = (int64_t)p->n * PIADMM_OBCA_LEDGER_REC; break;
    case PIADMM_OBCA_LEDGER_GET_NEXT_ID: src = &next_id; want = sizeof(int64_t); host = true; break;
    default: return fail(h, PIADMM_E_ARG, "obca_ledger_get: unknown item " + std::to_string(what));
  }
  return get_finish(h, "obca_ledger_get", what, src, host, want, out, bytes);
}

int32_t piadmm_obca_ledger_clear(piadmm_obca_t h) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_ledger(h, &p, "obca_ledger_clear")) return rc;
  p->lg.count = 0;
  return 0;
}

int32_t piadmm_obca_ledger_stats(piadmm_obca_t h, const double* edges, int32_t B, int32_t K, piadmm_obca_stats_t* stats,
                                 int64_t* hist, int32_t* worst) {
  piadmm_obca_plan_s* p = nullptr;
  if (int rc = open_ledger(h, &p, "obca_ledger_stats")) return rc;
  auto& l = p->lg;
  if (l.count == 0) return fail(h, PIADMM_E_STATE, "obca_ledger_stats: the ledger holds no record");
  // the rows' results of the R = 1 view say nothing the minima do not: they stay here
  const size_t Bz = B > 0 ? (size_t)B : 1;
  std::vector<double> row_min(4);
  std::vector<int32_t> row_arg(4), row_below(4 * Bz);
  const stats_out o{stats, hist, row_min.data(), row_arg.data(), row_below.data(), worst};
  if (int rc = stats_args_check(h, "obca_ledger_stats", l.count, edges, B, K, o)) return rc;
  OWN_HIP(h, hipSetDevice(h->device));
  const size_t C = (size_t)l.count;
  const size_t o_clear = up256(C * TSUM * 8), o_it = o_clear + up256(2 * C * 2 * 8), o_mask = o_it + up256(C * 4),
               need = o_mask + up256(C * 2 * 4);
  if (l.view_cap < need) {
    OWN_HIP(h, hipStreamSynchronize(h->stream));
    l.view = {};
    l.view_cap = 0;
    if (int rc = l.view.alloc(h, need, false)) return rc;
    l.view_cap = need;
  }
  char* v = l.view;
  double* d_sum = reinterpret_cast<double*>(v);
  double* d_clear = reinterpret_cast<double*>(v + o_clear);
  int* d_it = reinterpret_cast<int*>(v + o_it);
  int* d_mask = reinterpret_cast<int*>(v + o_mask);
  hipLaunchKernelGGL(k_ledger_view, dim3((unsigned)((C * LVIEW + 64 * PW - 1) / (64 * PW))), dim3(64 * PW), 0, h->stream,
                     (const long long*)l.rec, l.count, d_sum, d_clear, d_it, d_mask);
  OWN_HIP(h, hipGetLastError());
  return stats_run(h, 1, l.count, d_clear, d_sum, d_it, d_mask, edges, B, K, o);
}

int32_t piadmm_obca_ledger_end(piadmm_obca_t h) {
  if (!h) return PIADMM_E_ARG;
  if (!h->plan || !h->plan->lg.on) return 0;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  h->plan->lg = {};
  return 0;
}

}  // extern "C"
