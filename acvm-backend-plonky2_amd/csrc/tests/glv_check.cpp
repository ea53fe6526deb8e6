// glv_check.cpp -- the GLV decomposition of glv.hpp on a file of scalars, without the library and without a GPU
// (tests/test_glv_host.py compares what it prints with Python's integers).
//   g++ -O2 -std=c++17 -Wall -Werror -o glv_check glv_check.cpp && ./glv_check CASES > OUT
// CASES: one scalar per line, "lk" and then lk limbs in hexadecimal, up to 64 bits each (a limb >= 2^32 carries), least
// significant first; the scalar is their fold reduced modulo N.  OUT: per scalar "<k1> <k2> <k1_neg> <k2_neg>", the magnitudes in
// hexadecimal, assembled from all eight words the arithmetic leaves (the generator's targets have four limbs: more is its refusal).
#include <cinttypes>
#include <cstdio>
#include <string>
#include "../glv.hpp"

using namespace p2;

static std::string hex(const uint32_t *w) {
  std::string s;
  char buf[16];
  bool lead = true;
  for (uint32_t i = NN_LIMBS; i-- > 0;) {
    if (lead && !w[i]) continue;
    std::snprintf(buf, sizeof buf, lead ? "%x" : "%08x", w[i]);
    s += buf;
    lead = false;
  }
  return lead ? "0" : s;
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: glv_check CASES\n"); return 2; }
  FILE *f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint32_t lk;
  while (std::fscanf(f, "%u", &lk) == 1) {
    if (lk > NN_MAX_OPERAND) { std::fprintf(stderr, "unsupported case %u\n", lk); return 2; }
    Glv g;
    uint32_t k[NN_LIMBS];
    uint64_t limb;
    for (uint32_t i = 0; i < lk; i++) {
      if (std::fscanf(f, "%" SCNx64, &limb) != 1) { std::fprintf(stderr, "a limb is missing\n"); return 2; }
      g.f.push(i, limb);
    }
    g.f.reduce(lk, k);
    g.decompose(k);
    std::printf("%s %s %d %d\n", hex(g.k1).c_str(), hex(g.k2).c_str(), g.k1_neg ? 1 : 0, g.k2_neg ? 1 : 0);
  }
  std::fclose(f);
  return std::fflush(stdout) == 0 ? 0 : 2;
}
