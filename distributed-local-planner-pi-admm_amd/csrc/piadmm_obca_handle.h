// piadmm_obca_handle.h -- the piadmm_obca_t handle, shared by the local batch
// (csrc/piadmm_obca.hip), the edge step (csrc/piadmm_obca_edge.hip) and the device-resident
// consensus loop (csrc/piadmm_obca_plan.hip and the csrc/piadmm_obca_plan_*.hip units of its attachments).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "pd_owners.h"
#include "piadmm.h"

struct piadmm_obca_plan_s;      // csrc/piadmm_obca_plan.h

// Every device array is owned by its member; the destructor lets the events and the stream go, so a
// handle that was only part made is released by `delete` like a whole one (piadmm_obca_create).
struct piadmm_obca_s {
  template <typename T>
  using dbuf = pd_own::dev_buf<T>;
  piadmm_obca_s() = default;
  piadmm_obca_s(const piadmm_obca_s&) = delete;
  piadmm_obca_s& operator=(const piadmm_obca_s&) = delete;
  ~piadmm_obca_s() {
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    if (stream) (void)hipStreamDestroy(stream);
  }
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  dbuf<double> d_rec, d_out;
  dbuf<int> d_ist;
  dbuf<char> d_qg;              // per-problem linearisation blocks (obca::WsG, HBM)
  dbuf<unsigned long long> d_stamps;
  dbuf<int> d_order;            // the launch's problem order (longest first; cap ints)
  std::vector<int> order;       // host copy of the order
  std::vector<int> cost;        // the last solve's status / SQP iterations / QP steps per problem
  int cost_n = 0;               // batch size of the last solve (0: none yet)
  int cap = 0, n = 0;
  // the edge step's own buffers (csrc/piadmm_obca_edge.hip): an edge call never touches the
  // resident local batch above or its longest-first history
  dbuf<double> e_rec, e_out;
  dbuf<int> e_ist;
  int e_cap = 0;
  // the consensus loop (csrc/piadmm_obca_plan.hip).  piadmm_obca_plan_begin takes the local and
  // edge buffers over: plan_taken stays set (piadmm_obca_run / _time / _download: PIADMM_E_STATE)
  // until the next piadmm_obca_upload, which also ends the plan.
  piadmm_obca_plan_s* plan = nullptr;
  bool plan_taken = false;
  std::string err;
};

// The error path of every OBCA unit: the message into the handle, the code back.  A failed runtime
// call goes through OWN_HIP (pd_owners.h), which words it "<the call as written>: <HIP's text>".
inline int fail(piadmm_obca_t h, int code, const std::string& msg) { return pd_own::own_fail(h, code, msg); }

// The plan path's view of the two solves: grow the handle's buffers to n local problems / n pairs,
// and enqueue one launch over the first n records already in d_rec (problem order d_order[0..n))
// or e_rec on the handle's stream.  No copy, no synchronisation.
int piadmm_obca_local_ensure(piadmm_obca_t h, int n);
int piadmm_obca_local_launch(piadmm_obca_t h, int n);
int piadmm_obca_edge_ensure(piadmm_obca_t h, int n);
int piadmm_obca_edge_launch(piadmm_obca_t h, int n);

// an upload into the handle's buffers ends an open plan (its records would be overwritten);
// frees the plan's state (piadmm_obca_destroy)
void piadmm_obca_plan_release(piadmm_obca_t h);
void piadmm_obca_plan_free(piadmm_obca_t h);
