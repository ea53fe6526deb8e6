// genops.hpp -- the closed registry of witness-generator operations: which ops a gate row holds and which columns
// each of them reads and sets.  ONE enumerator, called by the host plan compiler (planhost.hpp) and by the device one
// (genplan.hip); the bodies that run the ops are generators.hpp's.  Plain C++ besides P2_HD: g++ compiles it.
#pragma once
#include "gates.hpp"

namespace p2 {

enum : uint32_t {
  OP_SEED = 0, OP_CONSTANT, OP_ARITHMETIC, OP_BASE_SPLIT, OP_BASE_JOIN, OP_RA_COPY, OP_RA_CONSTS, OP_POSEIDON, OP_U32_ARITHMETIC,
  OP_U32_ADD_MANY, OP_U32_SUBTRACTION, OP_U32_RANGE_CHECK, OP_COMPARISON,
  // the generators that are no gate's own (planhost.hpp): no row holds them and row_op does not list them; their cells come
  // from the plan's generator table
  OP_EQUALITY, OP_BIGUINT_DIVREM,
  // the four nonnative generators: their record keeps the field where a row op keeps its operation index (code | field << 8)
  OP_NONNATIVE_ADD, OP_NONNATIVE_SUB, OP_NONNATIVE_MUL, OP_NONNATIVE_INV,
  // the GLV decomposition generator of `decompose_secp256k1_scalar`: no field (its field is the secp256k1 scalar field)
  OP_GLV_DECOMPOSE
};
static_assert(OP_EQUALITY == 13 && OP_BIGUINT_DIVREM == 14 && OP_NONNATIVE_ADD == 15 && OP_NONNATIVE_SUB == 16 && OP_NONNATIVE_MUL == 17 &&
                  OP_NONNATIVE_INV == 18 && OP_GLV_DECOMPOSE == 19,
              "appended: the recorded plans keep their codes");
// an op whose record names a generator of the plan's list, not a row
P2_HD bool op_is_listed_generator(uint32_t code) { return code >= OP_EQUALITY && code <= OP_GLV_DECOMPOSE; }
// one of the generators whose word arrays live in private memory: the walk kernel's form with those arms runs them (genwit.hip)
P2_HD bool op_is_bigint_generator(uint32_t code) { return code >= OP_BIGUINT_DIVREM && code <= OP_GLV_DECOMPOSE; }

// The columns of one op: `in` then `out`, each the concatenation of two half-open ranges [a0, b0) ++ [a1, b1) in the order the
// schedule lists them (an empty range has a == b).  Columns >= R are gate-internal: the compilers skip them.
struct OpCols {
  uint32_t code, sub;
  uint32_t in[4], out[4];
};

// ops a row of gate g holds, in creation order (a BaseSum row: the split, then its twin the join)
P2_HD uint32_t row_num_ops(const GateDesc &g) {
  switch (g.kind) {
  case G_CONSTANT: case G_POSEIDON: case G_U32_RANGE_CHECK: case G_COMPARISON: return 1;
  case G_ARITHMETIC: case G_U32_ARITHMETIC: case G_U32_SUBTRACTION: return g.p[0];
  case G_BASE_SUM: return 2;
  case G_RANDOM_ACCESS: return g.p[1] + (g.p[2] ? 1u : 0u);
  case G_U32_ADD_MANY: return g.p[1];
  default: return 0;
  }
}

// op k < row_num_ops(g) of the row; c0, c1: the row's gate constants 0 and 1 (an ArithmeticGate operation reads the
// multiplicands only when c0 != 0 and the addend only when c1 != 0)
P2_HD OpCols row_op(const GateDesc &g, uint32_t k, gl_t c0, gl_t c1) {
  OpCols o = {OP_SEED, 0, {0, 0, 0, 0}, {0, 0, 0, 0}};
  auto in = [&](uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1) { o.in[0] = a0; o.in[1] = b0; o.in[2] = a1; o.in[3] = b1; };
  auto out = [&](uint32_t a0, uint32_t b0, uint32_t a1, uint32_t b1) { o.out[0] = a0; o.out[1] = b0; o.out[2] = a1; o.out[3] = b1; };
  switch (g.kind) {
  case G_CONSTANT:
    o.code = OP_CONSTANT;
    out(0, g.p[0], 0, 0);
    break;
  case G_ARITHMETIC:
    o.code = OP_ARITHMETIC; o.sub = k;
    in(4 * k, c0 ? 4 * k + 2 : 4 * k, 4 * k + 2, c1 ? 4 * k + 3 : 4 * k + 2);
    out(4 * k + 3, 4 * k + 4, 0, 0);
    break;
  case G_BASE_SUM:
    if (k == 0) {
      o.code = OP_BASE_SPLIT;
      in(0, 1, 0, 0);
      out(1, 1 + g.p[1], 0, 0);
    } else {
      o.code = OP_BASE_JOIN;
      in(1, 1 + g.p[1], 0, 0);
      out(0, 1, 0, 0);
    }
    break;
  case G_RANDOM_ACCESS: {
    const uint32_t bits = g.p[0], copies = g.p[1], extra = g.p[2], vec = 1u << bits, routed = (2 + vec) * copies + extra;
    if (k < copies) {
      const uint32_t base = (2 + vec) * k;
      o.code = OP_RA_COPY; o.sub = k;
      in(base, base + 1, base + 2, base + 2 + vec);
      out(base + 1, base + 2, routed + k * bits, routed + (k + 1) * bits);
    } else {
      o.code = OP_RA_CONSTS;
      out((2 + vec) * copies, (2 + vec) * copies + extra, 0, 0);
    }
    break;
  }
  case G_POSEIDON:
    o.code = OP_POSEIDON;
    in(0, 12, 24, 25);
    out(12, 24, 25, 135);
    break;
  case G_U32_ARITHMETIC:
    o.code = OP_U32_ARITHMETIC; o.sub = k;
    in(6 * k, 6 * k + 3, 0, 0);
    out(6 * k + 3, 6 * k + 6, 6 * g.p[0] + 32 * k, 6 * g.p[0] + 32 * k + 32);
    break;
  case G_U32_ADD_MANY: {
    const uint32_t na = g.p[0], nops = g.p[1], b = (na + 3) * k;
    o.code = OP_U32_ADD_MANY; o.sub = k;
    in(b, b + na + 1, 0, 0);
    out(b + na + 1, b + na + 3, (na + 3) * nops + 18 * k, (na + 3) * nops + 18 * k + 18);
    break;
  }
  case G_U32_SUBTRACTION:
    o.code = OP_U32_SUBTRACTION; o.sub = k;
    in(5 * k, 5 * k + 3, 0, 0);
    out(5 * k + 3, 5 * k + 5, 5 * g.p[0] + 16 * k, 5 * g.p[0] + 16 * k + 16);
    break;
  case G_U32_RANGE_CHECK:
    o.code = OP_U32_RANGE_CHECK;
    in(0, g.p[0], 0, 0);
    out(g.p[0], 17 * g.p[0], 0, 0);
    break;
  case G_COMPARISON: {
    const uint32_t nc = g.p[1], cb = (g.p[0] + nc - 1) / nc;
    o.code = OP_COMPARISON;
    in(0, 2, 0, 0);
    out(2, 4 + 5 * nc + cb + 1, 0, 0);
    break;
  }
  default: break;
  }
  return o;
}

// the k of an op record (code, sub) inside its row: the inverse of row_op's numbering
P2_HD uint32_t op_index_in_row(const GateDesc &g, uint32_t code, uint32_t sub) {
  if (code == OP_BASE_JOIN) return 1;
  if (code == OP_RA_CONSTS) return g.p[1];
  return sub;
}

// f(col) over the two ranges of an OpCols list
template <class F>
P2_HD void for_cols(const uint32_t r[4], F &&f) {
  for (uint32_t col = r[0]; col < r[1]; col++) f(col);
  for (uint32_t col = r[2]; col < r[3]; col++) f(col);
}

}  // namespace p2
