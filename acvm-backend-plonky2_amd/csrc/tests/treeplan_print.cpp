// treeplan_print.cpp -- prints the launch schedule of treeplan.hpp for every tree shape, in the format of
// tests/golden/tree_schedule.txt.gz (recorded from the launch code the plan replaced: profiles/merkle_refactor.md).  Per case one
// line per launch: profile name, grid x, grid y, block, nodes per coset of the input level, levels, profile bytes; then whether
// the cap level is mirrored to host memory.
//   g++ -O2 -std=c++17 -o treeplan_print treeplan_print.cpp && ./treeplan_print
#include <cstdio>
#include "../treeplan.hpp"

int main() {
  for (int hasher = 0; hasher < 2; hasher++)
    for (uint32_t cosets = 1; cosets <= 8; cosets *= 2)
      for (uint32_t lg = 0; lg <= 24; lg++)
        for (uint32_t cap = 1; cap <= 16; cap *= 2)
          for (uint32_t done = 0; done <= 2; done += 2) {  // levels the leaf launch has built
            const uint32_t m0 = 1u << lg;
            if (done && m0 < 4 * cap) continue;  // (a tree of fewer than three levels)
            std::printf("# hasher %d cosets %u nodes %u cap %u done %u\n", hasher, cosets, m0, cap, done);
            const p2::TreePlan p = p2::tree_plan(hasher, cosets, m0 >> done, cap);
            for (uint32_t i = 0; i < p.count; i++) {
              const p2::TreeStep &s = p.step[i];
              std::printf("%s %u %u %u %u %u %.0f\n", p2::tree_kernel_name(s.kernel), s.grid_x, s.grid_y, s.block, s.m, s.levels, s.bytes(cosets));
            }
            std::printf("mirrored %d\n", p.cap_from_coop_keccak() ? 1 : 0);  // (a mirror buffer exists whenever the tree has a level to build)
          }
  return 0;
}
