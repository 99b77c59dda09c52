// piadmm_obca_handle.h -- the piadmm_obca_t handle, shared by the local batch
// (csrc/piadmm_obca.hip), the edge step (csrc/piadmm_obca_edge.hip) and the device-resident
// consensus loop (csrc/piadmm_obca_plan.hip and the csrc/piadmm_obca_plan_*.hip units of its attachments).
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "piadmm.h"

struct piadmm_obca_plan_s;      // csrc/piadmm_obca_plan.h

struct piadmm_obca_s {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  double* d_rec = nullptr;
  double* d_out = nullptr;
  int* d_ist = nullptr;
  void* d_qg = nullptr;         // per-problem linearisation blocks (obca::WsG, HBM)
  unsigned long long* d_stamps = nullptr;
  int* d_order = nullptr;       // the launch's problem order (longest first; cap ints)
  std::vector<int> order;       // host copy of the order
  std::vector<int> cost;        // the last solve's status / SQP iterations / QP steps per problem
  int cost_n = 0;               // batch size of the last solve (0: none yet)
  int cap = 0, n = 0;
  // the edge step's own buffers (csrc/piadmm_obca_edge.hip): an edge call never touches the
  // resident local batch above or its longest-first history
  double* e_rec = nullptr;
  double* e_out = nullptr;
  int* e_ist = nullptr;
  int e_cap = 0;
  // the consensus loop (csrc/piadmm_obca_plan.hip).  piadmm_obca_plan_begin takes the local and
  // edge buffers over: plan_taken stays set (piadmm_obca_run / _time / _download: PIADMM_E_STATE)
  // until the next piadmm_obca_upload, which also ends the plan.
  piadmm_obca_plan_s* plan = nullptr;
  bool plan_taken = false;
  std::string err;
};

// frees the edge buffers (piadmm_obca_destroy)
void piadmm_obca_edge_free(piadmm_obca_t h);

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
