// partition_dump.cpp -- prints what csrc/pd_partition.h makes of candidate graphs, for
// tests/test_partition_host.py.  Host only:
//   g++ -std=c++17 -I distributed-local-planner-pi-admm_amd/csrc tools/partition_dump.cpp -o partition_dump
//
// stdin, whitespace separated, any number of cases:
//   N E term_global global_pi no_gate dual_init force_graph block sharded n_slots nonfinite
//   v1 v2            (E pairs)
//   owned[N] slot[N] counted[E]        (only when sharded = 1)
// nonfinite: -1, or 4 * agent + k to make the agent's speed (k = 0) or state entry k - 1 a NaN.
// stdout, per case: "refused: <text>" or one line per array of the result, then "end".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "pd_partition.h"

static void line(const char* name, const std::vector<int>& v) {
  std::printf("%s:", name);
  for (int x : v) std::printf(" %d", x);
  std::printf("\n");
}

int main() {
  int N, E, term_global, global_pi, no_gate, dual_init, force_graph, block, sharded, n_slots, nonfinite;
  while (std::scanf("%d %d %d %d %d %d %d %d %d %d %d", &N, &E, &term_global, &global_pi, &no_gate, &dual_init,
                    &force_graph, &block, &sharded, &n_slots, &nonfinite) == 11) {
    if (N < 1 || E < 0) return 2;
    std::vector<int32_t> edges(2 * (size_t)E), slot;
    std::vector<uint8_t> owned, counted;
    for (auto& v : edges)
      if (std::scanf("%d", &v) != 1) return 2;
    if (sharded) {
      int x;
      for (int i = 0; i < N; ++i) {
        if (std::scanf("%d", &x) != 1) return 2;
        owned.push_back((uint8_t)x);
      }
      for (int i = 0; i < N; ++i) {
        if (std::scanf("%d", &x) != 1) return 2;
        slot.push_back(x);
      }
      for (int e = 0; e < E; ++e) {
        if (std::scanf("%d", &x) != 1) return 2;
        counted.push_back((uint8_t)x);
      }
      counted.push_back(0);      // (never read: keeps data() non-null when E = 0)
    }
    std::vector<double> spd((size_t)N, 1.0), xt0(3 * (size_t)N, 0.0);
    if (nonfinite >= 0) {
      if (nonfinite >= 4 * N) return 2;
      (nonfinite % 4 == 0 ? spd[nonfinite / 4] : xt0[3 * (size_t)(nonfinite / 4) + nonfinite % 4 - 1]) = NAN;
    }
    if (const char* why = pd::check_graph_args(N, edges.data(), E, sharded ? owned.data() : nullptr, slot.data(),
                                               n_slots, counted.data(), term_global != 0, spd.data(), xt0.data())) {
      std::printf("refused: %s\nend\n", why);
      continue;
    }
    const pd::Partition P = pd::partition(N, edges.data(), E, sharded != 0, sharded && n_slots > 0, global_pi != 0,
                                          no_gate != 0, dual_init != 0, term_global != 0, force_graph != 0, block);
    std::printf("simple: %d\nsplit: %d\nC: %d\n", (int)P.simple, (int)P.split, P.C);
    line("comp_ptr", P.comp_ptr);
    line("comp_edge", P.comp_edge);
    line("nbr", P.nbr);
    line("aptr", P.aptr);
    line("alist", P.alist);
    line("eptr", P.eptr);
    line("elist", P.elist);
    line("nptr", P.nptr);
    line("nedge", P.nedge);
    line("ndir", P.ndir);
    line("sum_cptr", P.sum_cptr);
    line("sum_pos", P.sum_pos);
    line("pair_block", P.pair_block);
    std::printf("end\n");
  }
  return 0;
}
