// pd_partition.h -- the graph work of a scenario (piadmm_scenario.cpp), host only: what refuses a
// candidate graph, which kernel takes it, its components, their workgroup blocks, the neighbour
// CSR and the residual-sum order.  No HIP here: tools/partition_dump.cpp prints the arrays for
// tests/test_partition_host.py.  The device reads every array as it is built here.
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <vector>

namespace pd {

// Why the arguments of a set_scenario call are refused (the checks that need no device), or
// nullptr.  owned == nullptr: not a sharded job (slot, n_slots and counted are not read).
inline const char* check_graph_args(int N, const int32_t* edges, int n_edges, const uint8_t* owned,
                                    const int32_t* slot, int n_slots, const uint8_t* counted, bool term_global,
                                    const double* spd, const double* xt0) {
  for (int e = 0; e < n_edges; ++e) {
    const int v1 = edges[2 * e], v2 = edges[2 * e + 1];
    if (v1 < 0 || v2 >= N || v1 >= v2) return "edge must satisfy 0 <= v1 < v2 < N";
  }
  {
    // a pair listed twice would add its AL term twice to both x-steps and solve its QP twice
    std::vector<long long> key((size_t)n_edges);
    for (int e = 0; e < n_edges; ++e) key[e] = (long long)edges[2 * e] * N + edges[2 * e + 1];
    std::sort(key.begin(), key.end());
    if (std::adjacent_find(key.begin(), key.end()) != key.end())
      return "duplicate candidate pair (the same (v1, v2) twice)";
  }
  if (owned) {
    if (!slot || !counted || n_slots < 0) return "shard: null array or n_slots < 0";
    bool ghosts = false;
    for (int i = 0; i < N; ++i) {
      if (owned[i] > 1 || slot[i] < -1 || slot[i] >= n_slots) return "shard: owned must be 0/1 and slot in [-1, n_slots)";
      if (!owned[i] && slot[i] < 0) return "shard: a ghost agent needs an exchange slot";
      ghosts |= !owned[i];
    }
    for (int e = 0; e < n_edges; ++e) {
      if (counted[e] > 1) return "shard: counted must be 0/1";
      if (!owned[edges[2 * e]] && !owned[edges[2 * e + 1]])
        return "shard: a pair of two ghost agents (it belongs to another rank)";
    }
    if (ghosts && n_slots == 0) return "shard: ghost agents without an exchange buffer";
    if (n_slots > 0 && !term_global) return "shard: pairs across ranks need term_global (one stop for the whole job)";
  }
  for (int i = 0; i < N; ++i)
    if (!std::isfinite(spd[i]) || !std::isfinite(xt0[3 * i]) || !std::isfinite(xt0[3 * i + 1]) ||
        !std::isfinite(xt0[3 * i + 2]))
      return "non-finite speed or state";
  return nullptr;
}

struct Partition {
  bool simple = true;     // the fused kernel takes the graph (else the graph kernel)
  bool split = false;     // a component spans several workgroup blocks
  int C = 0;              // components (split: blocks)
  std::vector<int> comp_ptr, comp_edge, nbr;
  // graph mode: agent / pair lists per component (split: per block), neighbour CSR
  std::vector<int> aptr, alist, eptr, elist, nptr, nedge, ndir;
  // split: pairs per original component, each pair's position in that sum order, its block
  std::vector<int> sum_cptr, sum_pos, pair_block;
};

// Components of more than `block` agents (PIADMM_GRAPH_BLOCK, default 4; 0: never) span
// several workgroups under the global scope: blocks of `block` consecutive agents (in index
// order, numbered by first agent), the component's pairs dealt round-robin over its blocks.  The x-step
// of an agent reads the hat / lam of pairs other blocks own and a pair reads positions of
// agents other blocks own, so the X and Z phases run as separate launches (the kernel boundary
// orders them); the stop test sums the blocks' partials (one job-wide decision).
// comp (the component of each agent) becomes the block of each agent, C the block count.
inline void cut_blocks(Partition& P, int N, const int32_t* edges, int n_edges, int block, std::vector<int>& comp,
                       int& C) {
  // the original components' pair lists (pairs in increasing index): k_graph_partials sums
  // the residual terms in this order, the reference's (casadi/main.py:165-173)
  P.sum_cptr.assign(C + 1, 0);
  for (int e = 0; e < n_edges; ++e) ++P.sum_cptr[comp[edges[2 * e]] + 1];
  for (int k = 0; k < C; ++k) P.sum_cptr[k + 1] += P.sum_cptr[k];
  P.sum_pos.resize(n_edges);
  {
    std::vector<int> fill(P.sum_cptr.begin(), P.sum_cptr.end() - 1);
    for (int e = 0; e < n_edges; ++e) P.sum_pos[e] = fill[comp[edges[2 * e]]]++;
  }
  const std::vector<int> ocomp = comp;      // original component of each agent
  std::vector<int> seen(C, 0), cur(C, -1);
  std::vector<std::vector<int>> blocks_of(C);
  int NB = 0;
  for (int a = 0; a < N; ++a) {
    const int k = comp[a];
    if (seen[k] % block == 0) {                  // a new block of component k
      cur[k] = NB++;
      blocks_of[k].push_back(cur[k]);
    }
    ++seen[k];
    comp[a] = cur[k];
  }
  // pairs dealt round-robin over the component's blocks (in pair order), so the pair QPs of
  // a densely coupled component -- an all-pairs crossing: 6 pairs of 4 agents -- run on
  // several workgroups at once instead of queueing on the first agents' blocks
  P.pair_block.assign(n_edges, 0);
  {
    std::vector<int> dealt(C, 0);
    for (int e = 0; e < n_edges; ++e) {
      const int k = ocomp[edges[2 * e]];
      P.pair_block[e] = blocks_of[k][dealt[k]++ % blocks_of[k].size()];
    }
  }
  C = NB;
  P.split = true;
}

// The fused kernel (piadmm_device.hip) takes components of one agent or one pair (v, v+1);
// any other candidate graph -- components of more agents, agents in several pairs -- runs
// on the graph kernel (piadmm_graph.hip), and so does
//   force_graph: PIADMM_GRAPH=1 (tests);
//   global_pi / no_gate / dual_init: the global PI law (adaptive per-pair penalties), the
//     collision gate off, a nonzero initial pair state (the adaptive-gain script's 1e-4);
//   exchange: a sharded job with a boundary exchange (its X / Z phases are split launches around
//     the all-reduce).
// sharded: the job has shard arrays at all (it never splits).  block: PIADMM_GRAPH_BLOCK.
inline Partition partition(int N, const int32_t* edges, int n_edges, bool sharded, bool exchange, bool global_pi,
                           bool no_gate, bool dual_init, bool term_global, bool force_graph, int block) {
  Partition P;
  std::vector<int> pair_of(N, -1);
  for (int e = 0; e < n_edges && P.simple; ++e) {
    const int v1 = edges[2 * e], v2 = edges[2 * e + 1];
    if (v2 != v1 + 1 || pair_of[v1] >= 0 || pair_of[v2] >= 0) P.simple = false;
    else pair_of[v1] = pair_of[v2] = e;
  }
  if (force_graph || global_pi || no_gate || dual_init || exchange) P.simple = false;
  P.comp_ptr.assign(1, 0);
  P.nbr.assign(N, 0);
  if (P.simple) {
    for (int a = 0; a < N;) {
      const int e = pair_of[a];
      if (e >= 0) {
        P.comp_edge.push_back(e);
        P.nbr[a] = P.nbr[a + 1] = 1;
        a += 2;
      } else {
        P.comp_edge.push_back(-1);
        a += 1;
      }
      P.comp_ptr.push_back(a);
    }
    P.C = (int)P.comp_edge.size();
    return P;
  }
  // graph mode: connected components labelled in order of their first agent (the oracle's
  // Scenario.components()), agent / pair lists per component, neighbour CSR sorted by
  // neighbour id (the order of the x-step's consensus sum)
  std::vector<int> parent(N);
  for (int a = 0; a < N; ++a) parent[a] = a;
  auto find = [&](int a) {
    while (parent[a] != a) a = parent[a] = parent[parent[a]];
    return a;
  };
  for (int e = 0; e < n_edges; ++e) {
    const int ra = find(edges[2 * e]), rb = find(edges[2 * e + 1]);
    if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
  }
  std::vector<int> comp(N), id_of(N, -1);
  int C = 0;
  for (int a = 0; a < N; ++a) {
    const int r = find(a);
    if (id_of[r] < 0) id_of[r] = C++;
    comp[a] = id_of[r];
  }
  if (term_global && !sharded && block > 0) {
    std::vector<int> csize(C, 0);
    for (int a = 0; a < N; ++a) ++csize[comp[a]];
    bool any = false;
    for (int k = 0; k < C; ++k) any |= csize[k] > block;
    if (any) cut_blocks(P, N, edges, n_edges, block, comp, C);
  }
  P.aptr.assign(C + 1, 0);
  P.eptr.assign(C + 1, 0);
  for (int a = 0; a < N; ++a) ++P.aptr[comp[a] + 1];
  auto owner = [&](int e) { return P.split ? P.pair_block[e] : comp[edges[2 * e]]; };
  for (int e = 0; e < n_edges; ++e) ++P.eptr[owner(e) + 1];
  for (int k = 0; k < C; ++k) {
    P.aptr[k + 1] += P.aptr[k];
    P.eptr[k + 1] += P.eptr[k];
  }
  P.alist.resize(N);
  P.elist.resize(n_edges);
  {
    std::vector<int> fa(P.aptr.begin(), P.aptr.end() - 1), fe(P.eptr.begin(), P.eptr.end() - 1);
    for (int a = 0; a < N; ++a) P.alist[fa[comp[a]]++] = a;
    for (int e = 0; e < n_edges; ++e) P.elist[fe[owner(e)]++] = e;
  }
  std::vector<std::vector<std::array<int, 3>>> adj(N);
  for (int e = 0; e < n_edges; ++e) {
    const int v1 = edges[2 * e], v2 = edges[2 * e + 1];
    adj[v1].push_back({v2, e, 0});
    adj[v2].push_back({v1, e, 1});
  }
  P.nptr.assign(N + 1, 0);
  for (int a = 0; a < N; ++a) {
    std::sort(adj[a].begin(), adj[a].end());
    P.nbr[a] = (int)adj[a].size();
    P.nptr[a + 1] = P.nptr[a] + P.nbr[a];
    for (const auto& x : adj[a]) {
      P.nedge.push_back(x[1]);
      P.ndir.push_back(x[2]);
    }
  }
  P.comp_ptr = P.aptr;                    // (sizes only: agents of a component need not be contiguous)
  P.comp_edge.assign(C, -1);
  P.C = C;
  return P;
}

}  // namespace pd
