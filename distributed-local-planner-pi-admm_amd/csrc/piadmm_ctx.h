// piadmm_ctx.h -- what the units of the planner's C-ABI share (internal, not installed): the handle,
// the error helpers, the environment knobs and the functions one unit calls in another.
//   piadmm_capi.cpp        version / build info, create / destroy, state up and down, counters, ties
//   piadmm_scenario.cpp    set_scenario: check -> partition (pd_partition.h) -> allocate -> upload
//   piadmm_steps.cpp       the launches of MPC steps and their termination, the communicator
//   piadmm_candidates.cpp  candidate pairs on the grid hash
#pragma once

#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "pd_owners.h"
#include "piadmm_internal.h"

// The handle.  Everything it holds on the device or pinned has an owner here: the scenario's arrays
// are the arena's (d_part and d_xrecv are two of them), the pinned buffers are dev_bufs, and the
// destructor lets the communicator, the events and the stream go, so `delete` releases a handle
// that was only part made like a whole one.
struct piadmm_ctx {
  piadmm_ctx() = default;
  piadmm_ctx(const piadmm_ctx&) = delete;
  piadmm_ctx& operator=(const piadmm_ctx&) = delete;
  ~piadmm_ctx() {
    scn.release();                 // (synchronises the stream first)
    if (comm) (void)ncclCommDestroy(comm);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    if (stream) (void)hipStreamDestroy(stream);
    stream = nullptr;              // (the members' destructors run after this one)
  }
  // the scenario goes: its arrays, and the pointers into them that live outside DevArgs
  void release_scenario() {
    scn.release();
    d_part = d_xrecv = nullptr;
    have_scn = false;
  }
  piadmm_config_t cfg{};
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  bool have_scn = false;
  int N = 0, E = 0, C = 0, T = 0;
  std::vector<int> comp_ptr, comp_edge;
  pd_own::arena<piadmm_ctx> scn{this};
  pd::DevArgs a{};
  std::string err;
  // term_global: RCCL communicator (null = single rank), device partials, pinned host copy
  ncclComm_t comm = nullptr;
  int nranks = 1, rank = 0;
  double* d_part = nullptr;      // max_outer x 5 partials, or max_outer x 2 residual history
  pd_own::dev_buf<double, true> h_part;
  std::vector<double> ghist;     // global (rk, sk) history of the last step
  int giters = 0;
  int step_cap = 1;              // MPC steps per persistent launch (resid slots)
  bool coop = false;             // term_global natural termination decided in-kernel (one rank)
  std::vector<double> rho_init;  // host staging of the initial ADMM penalties (outlives the async copy)
  std::vector<double> rho_pi_init;   // host staging of the global-PI pair penalties
  std::vector<std::vector<int>> graph_host;   // graph-mode index arrays (host staging)
  std::vector<unsigned char> shard_host;      // owned | counted (host staging)
  // sharded graph (piadmm_set_scenario_shard): ghost agents fed by one all-reduce of the
  // boundary exchange buffer per outer iteration
  bool xchg = false;
  int n_slots = 0;
  // a connected component larger than the workgroup block (term_global) split over several
  // workgroups: the graph kernel's X and Z phases as separate launches (like a sharded job's,
  // without the exchange: every agent's positions are in this handle's memory)
  bool split = false;
  double* d_xrecv = nullptr;
  // host all-reduce transport (piadmm_set_allreduce): used when there is no RCCL communicator
  piadmm_allreduce_fn xfn = nullptr;
  void* xctx = nullptr;
  pd_own::dev_buf<double, true> h_x;   // pinned staging of the host transport
  size_t h_x_n = 0;
  // host-stepped MPC step (piadmm_outer_iter / piadmm_step_finish): the open step, the next
  // outer iteration, and the host-decided stop state of the global scope
  bool step_open = false;
  // the MPC step the receding-horizon sequence continues with (-1: a fresh sequence, any t).  A
  // step run at any other t (the same t again, a jump) must not resume a pair's stored dual active
  // set: its S^-1 and Y columns were built for another step's geometry (pd_qp.h gi_snap_restore)
  int t_next = -1;
  int step_t = -1, step_it = 0, step_flag = 0, step_nanlast = 0, step_stop = 0;
  // device-decided global termination (F_DEVSTOP): pinned copy of the stop state, iterations
  // enqueued per chunk (the last step's count), PIADMM_HOST_DECIDE=1 keeps one host decision
  // per outer iteration
  pd_own::dev_buf<int, true> h_ctl;
  int chunk_guess = 2;
  bool host_decide = false;
  // near-tie log (piadmm_get_near_ties): tolerance, and the ties of stop decisions the host takes
  double tie_tol = 0.0;         // 0: the log is off (piadmm_set_tie_tolerance turns it on)
  std::vector<piadmm_near_tie_t> host_ties;
  unsigned long long host_tie_cnt[PIADMM_TIE_KINDS] = {};
  // MPC steps per persistent launch agreed over the job's ranks (the fixed-iteration residual
  // history is all-reduced once per launch: every rank must cut the steps into the same launches)
  bool cap_synced = false;
};

// h->err (h may be null) and the thread's message (piadmm_last_error(nullptr)); returns code
int fail(piadmm_ctx* h, int code, const std::string& msg);
template <>
inline int pd_own::own_fail<piadmm_ctx>(piadmm_ctx* h, int code, const std::string& msg) {
  return fail(h, code, msg);
}

#define HIPCHK(h, expr)                                                              \
  do {                                                                               \
    hipError_t _e = (expr);                                                          \
    if (_e != hipSuccess)                                                            \
      return fail((h), PIADMM_E_HIP, std::string(#expr ": ") + hipGetErrorString(_e)); \
  } while (0)
#define LAUNCH(h, expr)                                                                       \
  do {                                                                                        \
    if ((expr) != 0)                                                                          \
      return fail((h), PIADMM_E_HIP, std::string("kernel launch " #expr ": ") + hipGetErrorString(pd::g_launch_err)); \
  } while (0)
#define NCCLCHK(h, expr)                                                                      \
  do {                                                                                        \
    ncclResult_t _r = (expr);                                                                 \
    if (_r != ncclSuccess) return fail((h), PIADMM_E_HIP, std::string(#expr ": ") + ncclGetErrorString(_r)); \
  } while (0)

// The environment knobs, each read at one moment.  Tests change them between scenarios of one
// process, so the moments are part of the behaviour.
inline bool env_is(const char* name, char c) {
  const char* v = std::getenv(name);
  return v && v[0] == c;
}
// at piadmm_create: PIADMM_HOST_DECIDE=1 keeps one host stop decision per outer iteration
inline bool knob_host_decide() { return env_is("PIADMM_HOST_DECIDE", '1'); }
// once per process: PIADMM_NO_ZX=1 runs a sharded job's fixed iterations as separate X and Z
// launches (A/B check)
inline bool knob_no_zx() {
  static const bool v = env_is("PIADMM_NO_ZX", '1');
  return v;
}
// at every set_scenario
struct scenario_knobs {
  bool force_graph;   // PIADMM_GRAPH=1: graph mode whatever the graph (tests)
  int block;          // PIADMM_GRAPH_BLOCK: agents per workgroup block of a split component (default 4; 0: never)
  int pair_gi;        // PIADMM_PAIR_SOLVER=admm (0): pair QPs skip the dual active set and take the ADMM +
                      // PDAS path (the fallback), so that tests can check both solvers against each other
  int pair_warm;      // PIADMM_PAIR_WARM=0: the pair's dual active set starts cold
  int x_gi;           // PIADMM_X_SOLVER (below)
  int no_spec;        // PIADMM_NO_SPEC=1: the fused kernel's plain loop shape instead of the speculative
                      // one (the two shapes' equality test)
  bool pair_snap;     // PIADMM_PAIR_SNAP=0: a pair's rows are appended again instead of restored (pd_qp.h)
  bool no_coop;       // PIADMM_NO_COOP=1: the host-decided path where the in-kernel stop test would fit
};
inline scenario_knobs read_scenario_knobs() {
  scenario_knobs k{};
  k.force_graph = env_is("PIADMM_GRAPH", '1');
  const char* gb = std::getenv("PIADMM_GRAPH_BLOCK");
  k.block = gb ? std::atoi(gb) : 4;
  const char* ps = std::getenv("PIADMM_PAIR_SOLVER");
  k.pair_gi = (ps && std::strcmp(ps, "admm") == 0) ? 0 : 1;
  k.pair_warm = env_is("PIADMM_PAIR_WARM", '0') ? 0 : 1;
  // PIADMM_X_SOLVER: "pdas" = one-step label moves + ADMM only; "gi" = the dual active set
  // warm-started from the labels after a failed reduced solve of them; "gi_warm" = the same,
  // except that an MPC step's first x-QP skips that reduced solve (a table rebuild, ~20 us,
  // that rarely certifies); default ("gi_cold") = that first x-QP's dual active set starts
  // cold (from the unconstrained minimiser: cheaper on a wave than appending and dropping the
  // previous step's shifted rows); "gi_cold_all" = every x-step dual active set starts cold
  const char* xs = std::getenv("PIADMM_X_SOLVER");
  const std::string x = xs ? xs : "";
  k.x_gi = x == "pdas" ? 0 : x == "gi" ? 1 : x == "gi_warm" ? 2 : x == "gi_cold_all" ? 4 : 3;
  k.no_spec = env_is("PIADMM_NO_SPEC", '1') ? 1 : 0;
  k.pair_snap = !env_is("PIADMM_PAIR_SNAP", '0');
  k.no_coop = env_is("PIADMM_NO_COOP", '1');
  return k;
}

// n elements of device array src to the host's dst on the handle's stream; a null dst (an output
// the caller did not ask for) or n == 0 copies nothing.  The caller synchronises.
template <typename T>
int download(piadmm_ctx* h, T* dst, const T* src, size_t n) {
  if (dst && n) HIPCHK(h, hipMemcpyAsync(dst, src, n * sizeof(T), hipMemcpyDeviceToHost, h->stream));
  return 0;
}

// piadmm_capi.cpp
int reset_penalties(piadmm_ctx* h);
