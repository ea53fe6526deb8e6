// bigdiv_check.cpp -- the long division of bigdiv.hpp on a file of cases, without the library and without a GPU
// (tests/test_bigdiv_host.py compares what it prints with Python's divmod).
//   g++ -O2 -std=c++17 -Wall -Werror -o bigdiv_check bigdiv_check.cpp && ./bigdiv_check CASES > OUT
// CASES: one case per line, "la lb" and then la + lb limbs in hexadecimal, up to 64 bits each (a limb >= 2^32 carries), least
// significant first.  OUT: per case "zero" (the divisor is zero) or "ok <add-back steps> <quotient> <remainder>", the two numbers
// in hexadecimal, assembled from the words the generator would write.
#include <cinttypes>
#include <cstdio>
#include <string>
#include "../bigdiv.hpp"

using namespace p2;

// the words w(0) .. w(count - 1), least significant first, as one hexadecimal number
template <class F> static std::string hex(uint32_t count, F &&w) {
  std::string s;
  char buf[16];
  bool lead = true;
  for (uint32_t i = count; i-- > 0;) {
    if (lead && !w(i)) continue;
    std::snprintf(buf, sizeof buf, lead ? "%x" : "%08x", w(i));
    s += buf;
    lead = false;
  }
  return lead ? "0" : s;
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: bigdiv_check CASES\n"); return 2; }
  FILE *f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  uint32_t la, lb;
  while (std::fscanf(f, "%u %u", &la, &lb) == 2) {
    if (la < 1 || la > BIGDIV_MAX_A || lb < 1 || lb > BIGDIV_MAX_B) { std::fprintf(stderr, "unsupported shape %u / %u\n", la, lb); return 2; }
    BigDiv w;
    uint64_t limb;
    for (uint32_t i = 0; i < la; i++) {
      if (std::fscanf(f, "%" SCNx64, &limb) != 1) { std::fprintf(stderr, "a limb is missing\n"); return 2; }
      w.push_a(i, limb);
    }
    w.finish_a(la);
    for (uint32_t i = 0; i < lb; i++) {
      if (std::fscanf(f, "%" SCNx64, &limb) != 1) { std::fprintf(stderr, "a limb is missing\n"); return 2; }
      w.push_b(i, limb);
    }
    w.finish_b(lb);
    uint32_t add_backs = 0;
    if (!w.divide(&add_backs)) {
      std::printf("zero\n");
      continue;
    }
    std::printf("ok %u %s %s\n", add_backs, hex(w.nq, [&](uint32_t i) { return w.quotient_word(i); }).c_str(),
                hex(w.nv, [&](uint32_t i) { return w.remainder_word(i); }).c_str());
  }
  std::fclose(f);
  return std::fflush(stdout) == 0 ? 0 : 2;
}
