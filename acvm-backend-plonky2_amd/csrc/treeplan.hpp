// treeplan.hpp -- which launches build a Merkle tree above its leaf digests.  Host-only and free of HIP, so that the schedule of
// every tree shape can be printed and compared without a GPU (tests/treeplan_print.cpp, tests/golden/tree_schedule.txt.gz);
// merkle.hip's tree_levels is the one place that turns a step into a launch.
#pragma once
#include <cstddef>
#include <cstdint>

namespace p2 {

// Thresholds, in nodes of a step's first OUTPUT level, all cosets together.
// One wave per SIMD on the chip (1024 SIMDs * 64 lanes): from here down a Keccak level is latency-bound, and up to three of
// them share a launch.
constexpr size_t TREE_ONE_WAVE_PER_SIMD = (size_t)1024 * 64;
// Two waves per SIMD: from here up a single Keccak level takes the throughput placement of the permutation's code (<1>);
// below, a SIMD sees a lone wave (<0>).
constexpr size_t TREE_TWO_WAVES_PER_SIMD = (size_t)2 * 1024 * 64;
// Keccak: a level with more than 2 048 nodes (two per wave: one wave per SIMD) is still cheaper one lane per node (7.5 us);
// at or below, the 25-lane form wins (3.5-5 us per level), four levels per launch.
constexpr size_t TREE_KECCAK_COOP_MAX = 2048;
// Poseidon: at or below this, twelve lanes per node pay up to four waves per SIMD (~27 vs ~75 us per level).
constexpr size_t TREE_POSEIDON_COOP_MAX = 16384;

enum class TreeKernel : uint8_t {
  LevelPoseidon,    // merkle_level_kernel<1>: one lane per node, one level
  LevelKfMany,      // merkle_level_kf_kernel<1>
  LevelKfLone,      // merkle_level_kf_kernel<0>
  LevelsKf,         // merkle_levels_kf_kernel: one lane per node, two or three levels
  CoopKeccak,       // merkle_coop_kernel: 25 lanes per node, up to four levels; the only kernel that can mirror the cap
  CoopPoseidon,     // merkle_coop_poseidon_kernel: 12 lanes per node, up to five levels
};
// the profile name of a step's kernel: the symbol rocprofv3 shows, so the bench line and profiles/ agree
inline const char *tree_kernel_name(TreeKernel k) {
  switch (k) {
    case TreeKernel::LevelPoseidon: return "merkle_level_kernel<1>";
    case TreeKernel::LevelKfMany: return "merkle_level_kf_kernel<1>";
    case TreeKernel::LevelKfLone: return "merkle_level_kf_kernel<0>";
    case TreeKernel::LevelsKf: return "merkle_levels_kf_kernel";
    case TreeKernel::CoopKeccak: return "merkle_coop_kernel";
    default: return "merkle_coop_poseidon_kernel";
  }
}

// one launch: the levels with m/2 ... m >> levels nodes per coset from the one with m
struct TreeStep {
  TreeKernel kernel;
  uint32_t m, levels;
  uint32_t grid_x, grid_y, block;
  double bytes(uint32_t cosets) const { return 96.0 * cosets * (double)(m - (m >> levels)); }  // (profile: two digests in, one out)
};
struct TreePlan {
  TreeStep step[24];  // a tree of 2^24 leaves built one level per launch
  uint32_t count = 0;
  // the cap level comes out of merkle_coop_kernel (a cap so wide that the tree ends on a single-lane level does not)
  bool cap_from_coop_keccak() const { return count != 0 && step[count - 1].kernel == TreeKernel::CoopKeccak; }
};

// hasher: 0 KeccakHash<25>, 1 PoseidonHash.  m: nodes per coset of the lowest level in place (a power of two); the plan ends at
// cap_per nodes per coset and is empty when m <= cap_per.  cosets <= 8 (rate_bits <= 3).
inline TreePlan tree_plan(int hasher, uint32_t cosets, uint32_t m, uint32_t cap_per) {
  TreePlan p;
  while (m > cap_per) {
    const uint32_t half = m >> 1;
    const size_t out = (size_t)cosets * half;
    TreeStep s{TreeKernel::LevelPoseidon, m, 1, 0, 1, 256};
    // (a Keccak level of fewer than 256 nodes per coset takes the 25-lane form whatever the cosets add up to)
    if (hasher == 1 ? out <= TREE_POSEIDON_COOP_MAX : (out <= TREE_KECCAK_COOP_MAX || half < 256)) {
      s.kernel = hasher == 1 ? TreeKernel::CoopPoseidon : TreeKernel::CoopKeccak;
      const uint32_t max_levels = hasher == 1 ? 5 : 4;
      while (s.levels < max_levels && (m >> s.levels) > cap_per) s.levels++;
      s.grid_x = cosets * (m >> s.levels);  // a block per node of the step's last level
    } else {
      // one lane per node
      if (hasher == 0) {
        s.kernel = out >= TREE_TWO_WAVES_PER_SIMD ? TreeKernel::LevelKfMany : TreeKernel::LevelKfLone;
        // latency-bound: one launch also takes the next level, and the one after it, while they are single-lane levels too and
        // not above the cap
        auto fusable = [&](uint32_t mo) { return (size_t)cosets * mo > TREE_KECCAK_COOP_MAX && mo >= 256 && mo >= cap_per; };
        if (out <= TREE_ONE_WAVE_PER_SIMD)
          while (s.levels < 3 && fusable(m >> (s.levels + 1))) s.levels++;
      }
      if (s.levels == 1) {
        s.block = half >= 256 ? 256 : 64;
        s.grid_x = (half + s.block - 1) / s.block;
        s.grid_y = cosets;
      } else {
        s.kernel = TreeKernel::LevelsKf;
        s.grid_x = cosets * ((m >> s.levels) >> 6);  // a block per 64 nodes of the step's last level
      }
    }
    p.step[p.count++] = s;
    m >>= s.levels;
  }
  return p;
}

}  // namespace p2
