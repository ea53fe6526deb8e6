// nonnative_check.cpp -- the modular arithmetic of nonnative.hpp on a file of cases, without the library and without a GPU
// (tests/test_nonnative_host.py compares what it prints with Python's %, divmod and pow(x, -1, M)).
//   g++ -O2 -std=c++17 -Wall -Werror -o nonnative_check nonnative_check.cpp && ./nonnative_check CASES > OUT
// CASES: one case per line, "op field la lb" (op: add, sub, mul, inv; inv has lb = 0) and then la + lb limbs in hexadecimal, up
// to 64 bits each (a limb >= 2^32 carries), least significant first.  OUT: per case "zero" (the inverse of zero) or "ok <first>
// <second>", the two numbers the generator of that name sets, in hexadecimal, assembled from the words it would write: sum and
// overflow, diff and overflow, prod and overflow, inv and div.
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <string>
#include "../nonnative.hpp"

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

static bool load(FILE *f, NonNative &n, uint32_t count, uint32_t *out) {
  uint64_t limb;
  for (uint32_t i = 0; i < count; i++) {
    if (std::fscanf(f, "%" SCNx64, &limb) != 1) return false;
    n.push(i, limb);
  }
  n.reduce(count, out);
  return true;
}

int main(int argc, char **argv) {
  if (argc != 2) { std::fprintf(stderr, "usage: nonnative_check CASES\n"); return 2; }
  FILE *f = std::fopen(argv[1], "r");
  if (!f) { std::fprintf(stderr, "cannot open %s\n", argv[1]); return 2; }
  char op[8];
  uint32_t field, la, lb;
  while (std::fscanf(f, "%7s %u %u %u", op, &field, &la, &lb) == 4) {
    const bool inv = !std::strcmp(op, "inv");
    if (field >= NN_FIELDS || la > NN_MAX_OPERAND || lb > NN_MAX_OPERAND || (inv && lb)) { std::fprintf(stderr, "unsupported case %s %u %u %u\n", op, field, la, lb); return 2; }
    NonNative n(field);
    uint32_t x[NN_LIMBS], y[NN_LIMBS];
    if (!load(f, n, la, x) || !load(f, n, lb, y)) { std::fprintf(stderr, "a limb is missing\n"); return 2; }
    auto words = [](const uint32_t *w) { return [w](uint32_t i) { return w[i]; }; };
    if (!std::strcmp(op, "add")) {
      const bool over = n.add_once(x, y);
      std::printf("ok %s %d\n", hex(NN_LIMBS, words(x)).c_str(), over ? 1 : 0);
    } else if (!std::strcmp(op, "sub")) {
      const bool over = n.sub_once(x, y);
      std::printf("ok %s %d\n", hex(NN_LIMBS, words(x)).c_str(), over ? 1 : 0);
    } else if (!std::strcmp(op, "mul")) {
      n.mul_divmod(x, y);
      std::printf("ok %s %s\n", hex(NN_LIMBS, [&](uint32_t i) { return n.w.remainder_word(i); }).c_str(),
                  hex(n.w.nq, [&](uint32_t i) { return n.w.quotient_word(i); }).c_str());
    } else if (inv) {
      uint32_t r[NN_LIMBS];
      if (!n.invert(x, r)) {
        std::printf("zero\n");
        continue;
      }
      n.mul_divmod(x, r);
      std::printf("ok %s %s\n", hex(NN_LIMBS, words(r)).c_str(), hex(n.w.nq, [&](uint32_t i) { return n.w.quotient_word(i); }).c_str());
    } else {
      std::fprintf(stderr, "unknown operation %s\n", op);
      return 2;
    }
  }
  std::fclose(f);
  return std::fflush(stdout) == 0 ? 0 : 2;
}
