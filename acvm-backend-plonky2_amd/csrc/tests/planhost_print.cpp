// planhost_print.cpp -- the host plan compiler of planhost.hpp on a circuit blob, without the library and without a GPU
// (tests/test_witness_plan_host.py compares what it prints with the plans recorded from p2gpu_witness_plan_create:
// profiles/witness_refactor.md).
//   g++ -O2 -std=c++17 -Wall -Werror -o planhost_print planhost_print.cpp && ./planhost_print BLOB SEEDS > OUT
// BLOB: a circuit blob without a stored cap (header word 25 == 0); the five tables are taken from it at the offsets
// tests/device_build_inputs.py decompose() documents: the gate table at 256, k_is behind it, the constant columns (selectors
// first), sigma.  SEEDS: (row, col) pairs of 32-bit words.  OUT: one text line, then for a plan the three arrays as they are:
//   plan <ops> <levels> <widest> <slots> <seeds>\n   cell_slot [R][n] u32, ops [ops] u64, level_off [levels + 1] u32
//   refused <p2gpu_last_error's text>\n
// With a third argument GENERATORS -- the generators that are no gate's own, p2gpu_generator records of nine 32-bit words
// (kind, then four (row, col) pairs) -- the plan's generator table [generators][4] u32 follows level_off.
// With four arguments, GENERATORS_V CELLS -- p2gpu_generator_v records of five 32-bit words (kind, shape[4]) and the flat list
// of their cells, (row, col) pairs of 32-bit words -- the offsets [generators + 1] u32 and then the table, one word per cell,
// follow level_off.
#include <cstdio>
#include <cstring>
#include "../planhost.hpp"

using namespace p2;

static_assert(sizeof(GateDesc) == 48, "the blob's gate record");

static std::vector<uint8_t> read_file(const char *path) {
  std::vector<uint8_t> out;
  FILE *f = std::fopen(path, "rb");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", path); std::exit(2); }
  uint8_t buf[1 << 16];
  for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + k);
  std::fclose(f);
  return out;
}

template <class T> static std::vector<T> words(const std::vector<uint8_t> &b, size_t off, size_t count) {
  if (off > b.size() || count > (b.size() - off) / sizeof(T)) { std::fprintf(stderr, "blob too short\n"); std::exit(2); }
  std::vector<T> out(count);
  if (count) std::memcpy(out.data(), b.data() + off, count * sizeof(T));
  return out;
}

int main(int argc, char **argv) {
  if (argc < 3 || argc > 5) { std::fprintf(stderr, "usage: planhost_print BLOB SEEDS [GENERATORS | GENERATORS_V CELLS]\n"); return 2; }
  const std::vector<uint8_t> blob = read_file(argv[1]), seed_bytes = read_file(argv[2]);
  const std::vector<uint32_t> h = words<uint32_t>(blob, 0, 64);
  const uint32_t d = h[2], W = h[3], R = h[4], NC = h[5], nsel = h[6], ng = h[23];
  if (h[25] != 0 || d > 24 || nsel > NC || R > W || seed_bytes.size() % 8) { std::fprintf(stderr, "unsupported blob or seed file\n"); return 2; }
  const size_t n = (size_t)1 << d;
  size_t off = 256;
  const std::vector<GateDesc> gates = words<GateDesc>(blob, off, ng);
  off += 48 * (size_t)ng;
  const std::vector<gl_t> k_is = words<gl_t>(blob, off, R);
  off += 8 * (size_t)R;
  const std::vector<gl_t> consts = words<gl_t>(blob, off, (size_t)NC * n);
  off += 8 * (size_t)NC * n;
  const std::vector<gl_t> sigma = words<gl_t>(blob, off, (size_t)R * n);
  // row -> gate: the one selector column that is not 2^32 - 1 holds the index
  std::vector<uint8_t> row_gate(n, 0);
  for (size_t row = 0; row < n; row++) {
    uint32_t gi = 0;
    for (uint32_t s = 0; s < nsel; s++) {
      const gl_t v = consts[(size_t)s * n + row];
      if (nsel == 1 || v != 0xFFFFFFFFull) gi = (uint32_t)v;
    }
    if (gi >= ng) { std::fprintf(stderr, "selector column holds an unknown gate index\n"); return 2; }
    row_gate[row] = (uint8_t)gi;
  }
  const std::vector<uint32_t> seed_words = words<uint32_t>(seed_bytes, 0, seed_bytes.size() / 4);
  const PlanInput in{d, R, W, NC - nsel, sigma.data(), consts.data() + (size_t)nsel * n, row_gate.data(), gates.data(), k_is.data()};
  static_assert(sizeof(PlanGenerator) == 36, "nine words");
  static_assert(sizeof(PlanGeneratorV) == 20, "five words");
  std::vector<PlanGenerator> gen_records;
  std::vector<PlanGeneratorV> genv_records;
  std::vector<uint32_t> genv_cells;
  PlanGenList gens;
  if (argc == 5) {
    const std::vector<uint8_t> gen_bytes = read_file(argv[3]), cell_bytes = read_file(argv[4]);
    if (gen_bytes.size() % sizeof(PlanGeneratorV) || cell_bytes.size() % 8) { std::fprintf(stderr, "unsupported generator file\n"); return 2; }
    genv_records = words<PlanGeneratorV>(gen_bytes, 0, gen_bytes.size() / sizeof(PlanGeneratorV));
    genv_cells = words<uint32_t>(cell_bytes, 0, cell_bytes.size() / 4);
  }
  if (argc == 4) {
    const std::vector<uint8_t> gen_bytes = read_file(argv[3]);
    if (gen_bytes.size() % sizeof(PlanGenerator)) { std::fprintf(stderr, "unsupported generator file\n"); return 2; }
    gen_records = words<PlanGenerator>(gen_bytes, 0, gen_bytes.size() / sizeof(PlanGenerator));
  }
  std::vector<PlanSeed> seeds;
  HostPlan plan;
  PlanRefusal r = plan_seeds(d, W, seed_words.data(), seed_words.size() / 2, seeds);
  if (!r)
    r = argc == 5 ? plan_generators_v(d, R, genv_records.data(), genv_records.size(), genv_cells.data(), genv_cells.size() / 2, gens)
                  : plan_generators(d, R, gen_records.data(), gen_records.size(), gens);
  if (!r) r = plan_compile_host(in, seeds, gens, plan);
  if (r) {
    std::printf("refused %s\n", plan_refusal_text(r, d, W, R).c_str());
    return 0;
  }
  std::printf("plan %zu %u %u %u %zu\n", plan.ops.size(), plan.levels, plan.widest, plan.slots, seeds.size());
  std::fwrite(plan.cell_slot.data(), 4, plan.cell_slot.size(), stdout);
  std::fwrite(plan.ops.data(), 8, plan.ops.size(), stdout);
  std::fwrite(plan.level_off.data(), 4, plan.level_off.size(), stdout);
  if (argc == 5) std::fwrite(plan.gen_off.data(), 4, plan.gen_off.size(), stdout);
  if (!plan.gen_table.empty()) std::fwrite(plan.gen_table.data(), 4, plan.gen_table.size(), stdout);
  return std::fflush(stdout) == 0 ? 0 : 2;
}
