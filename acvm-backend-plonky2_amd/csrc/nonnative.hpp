// nonnative.hpp -- the arithmetic behind the four nonnative generators (plonky2_ecdsa/biguint/gadgets/nonnative.rs:446-715:
// NonNativeAddition / Subtraction / Multiplication / InverseGenerator), on 32-bit words, one lane's worth of state in NonNative.
// Plain C++ besides P2_HD, as bigdiv.hpp is: g++ compiles it (csrc/tests/nonnative_check.cpp, tests/test_nonnative_host.py) and
// the level walk runs the same text (generators.hpp gen_nonnative_*).
//   fields  the two `FF` the reference instantiates (curve.rs, glv.rs): id 0 the secp256k1 base field, id 1 its scalar field;
//           a field element is NN_LIMBS = 8 words, least significant first.
//   fold    an operand's limbs are canonical field elements of up to 64 bits: BigDiv::push / finish fold them as the div-rem
//           generator does (a limb >= 2^32 carries into the next), and the folded integer is reduced modulo M by BigDiv::divide
//           -- upstream's FF::from_noncanonical_biguint.  Up to NN_MAX_OPERAND = 16 limbs, hence 18 words, in BigDiv's 35.
//   mul     the 8 x 8 -> 16-word product (32 x 32 + 32 + 32-bit steps) is built in BigDiv's dividend and divided by M:
//           quotient and remainder stay where BigDiv leaves them (quotient_word / remainder_word).
//   invert  the binary extended Euclidean algorithm (HAC 14.61 for an odd modulus): u = X, v = M, x1 = 1, x2 = 0; halve the even
//           one of u, v together with its coefficient (which takes + M first when it is odd: a 257-bit sum, the carry is shifted
//           back in), subtract the smaller from the larger and the coefficients modulo M, until u or v is 1.  At most 2 * 256
//           halvings, each a pass or two over eight words: a few hundred word-level passes where Fermat's exponentiation costs
//           about 380 modular products with a long division each.  The inverse is unique: the algorithm changes no byte.
#pragma once
#include "bigdiv.hpp"

namespace p2 {

constexpr uint32_t NN_LIMBS = 8, NN_MAX_OPERAND = 16, NN_FIELDS = 2;
constexpr uint32_t NN_FIELD_SECP256K1_BASE = 0, NN_FIELD_SECP256K1_SCALAR = 1;  // p2gpu.h P2GPU_FIELD_*
static_assert(NN_MAX_OPERAND + 2 <= BIGDIV_MAX_A + 3 && 2 * NN_LIMBS <= BIGDIV_MAX_A && NN_LIMBS <= BIGDIV_MAX_B, "BigDiv's arrays hold an operand and a product");

// word i of the modulus of field `field` < NN_FIELDS
P2_HD uint32_t nn_modulus_word(uint32_t field, uint32_t i) {
  // 2^256 - 2^32 - 977; 0xFFFFFFFF FFFFFFFF FFFFFFFF FFFFFFFE BAAEDCE6 AF48A03B BFD25E8C D0364141
  const uint32_t table[NN_FIELDS][NN_LIMBS] = {
      {0xFFFFFC2Fu, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu},
      {0xD0364141u, 0xBFD25E8Cu, 0xAF48A03Bu, 0xBAAEDCE6u, 0xFFFFFFFEu, 0xFFFFFFFFu, 0xFFFFFFFFu, 0xFFFFFFFFu}};
  return table[field][i];
}

// ---- eight words ----
P2_HD int nn_cmp(const uint32_t *x, const uint32_t *y) {  // -1, 0, 1
  for (uint32_t i = NN_LIMBS; i-- > 0;)
    if (x[i] != y[i]) return x[i] < y[i] ? -1 : 1;
  return 0;
}
P2_HD uint32_t nn_add(uint32_t *r, const uint32_t *x, const uint32_t *y) {  // r = x + y; returns the carry
  uint64_t c = 0;
  for (uint32_t i = 0; i < NN_LIMBS; i++) {
    c += (uint64_t)x[i] + y[i];
    r[i] = (uint32_t)c;
    c >>= 32;
  }
  return (uint32_t)c;
}
P2_HD uint32_t nn_sub(uint32_t *r, const uint32_t *x, const uint32_t *y) {  // r = x - y; returns the borrow
  uint64_t b = 0;
  for (uint32_t i = 0; i < NN_LIMBS; i++) {
    const uint64_t t = (uint64_t)x[i] - y[i] - b;
    r[i] = (uint32_t)t;
    b = (t >> 32) & 1;
  }
  return (uint32_t)b;
}
P2_HD bool nn_is_zero(const uint32_t *x) {
  uint32_t any = 0;
  for (uint32_t i = 0; i < NN_LIMBS; i++) any |= x[i];
  return any == 0;
}
P2_HD bool nn_is_one(const uint32_t *x) {
  uint32_t any = x[0] ^ 1u;
  for (uint32_t i = 1; i < NN_LIMBS; i++) any |= x[i];
  return any == 0;
}
// x = (top * 2^256 + x) / 2
P2_HD void nn_halve(uint32_t *x, uint32_t top) {
  for (uint32_t i = 0; i + 1 < NN_LIMBS; i++) x[i] = (x[i] >> 1) | (x[i + 1] << 31);
  x[NN_LIMBS - 1] = (x[NN_LIMBS - 1] >> 1) | (top << 31);
}

struct NonNative {
  BigDiv w;
  uint32_t m[NN_LIMBS];  // the modulus
  uint32_t field;

  P2_HD explicit NonNative(uint32_t f) : field(f) {
    for (uint32_t i = 0; i < NN_LIMBS; i++) m[i] = nn_modulus_word(f, i);
  }
  // the divisor of w: the modulus (divide() keeps it as it is: its top bit is set, nothing is shifted)
  P2_HD void load_modulus() {
    for (uint32_t i = 0; i < NN_LIMBS; i++) w.v[i] = m[i];
    w.nv = NN_LIMBS;
  }
  // out = fold(the `count` <= NN_MAX_OPERAND limbs given to push(0, ..) .. push(count - 1, ..)) mod M
  P2_HD void push(uint32_t i, uint64_t limb) { w.push_a(i, limb); }
  P2_HD void reduce(uint32_t count, uint32_t *out) {
    w.finish_a(count);
    load_modulus();
    w.divide();
    for (uint32_t i = 0; i < NN_LIMBS; i++) out[i] = w.remainder_word(i);
  }
  // (Q, R) = divmod(x * y, M): afterwards w.quotient_word(i), i < w.nq, and w.remainder_word(i), i < NN_LIMBS
  P2_HD void mul_divmod(const uint32_t *x, const uint32_t *y) {
    uint32_t *p = w.u;
    for (uint32_t i = 0; i < 2 * NN_LIMBS; i++) p[i] = 0;
    for (uint32_t i = 0; i < NN_LIMBS; i++) {
      uint64_t c = 0;
      for (uint32_t j = 0; j < NN_LIMBS; j++) {
        c += (uint64_t)x[i] * y[j] + p[i + j];  // (32 x 32 + 32 + 32 bits: no overflow)
        p[i + j] = (uint32_t)c;
        c >>= 32;
      }
      p[i + NN_LIMBS] = (uint32_t)c;
    }
    uint32_t n = 2 * NN_LIMBS;
    while (n && !p[n - 1]) n--;
    w.nu = n;
    load_modulus();
    w.divide();
  }
  // NonNativeAdditionGenerator's sum for x, y < M: x += y, less M when the sum is above M -- strictly, as upstream compares: x + y
  // = M stays M.  Returns that overflow
  P2_HD bool add_once(uint32_t *x, const uint32_t *y) {
    const uint32_t c = nn_add(x, x, y);
    const bool over = c || nn_cmp(x, m) > 0;
    if (over) nn_sub(x, x, m);
    return over;
  }
  // NonNativeSubtractionGenerator's difference for x, y < M: x -= y, plus M when x < y.  Returns that overflow
  P2_HD bool sub_once(uint32_t *x, const uint32_t *y) {
    const bool over = nn_sub(x, x, y) != 0;
    if (over) nn_add(x, x, m);
    return over;
  }
  // r = x - y mod M for x, y < M
  P2_HD void sub_mod(uint32_t *r, const uint32_t *x, const uint32_t *y) {
    if (nn_sub(r, x, y)) nn_add(r, r, m);
  }
  // x = x / 2 mod M for x < M (M is odd)
  P2_HD void halve_mod(uint32_t *x) {
    uint32_t c = 0;
    if (x[0] & 1) c = nn_add(x, x, m);
    nn_halve(x, c);
  }
  // out = x^-1 mod M for 0 < x < M; false: x = 0
  P2_HD bool invert(const uint32_t *x, uint32_t *out) {
    if (nn_is_zero(x)) return false;
    uint32_t u[NN_LIMBS], v[NN_LIMBS], x1[NN_LIMBS], x2[NN_LIMBS];
    for (uint32_t i = 0; i < NN_LIMBS; i++) u[i] = x[i], v[i] = m[i], x1[i] = i == 0, x2[i] = 0;
    // invariants: x1 * x = u, x2 * x = v (mod M); gcd(u, v) = 1
    while (!nn_is_one(u) && !nn_is_one(v)) {
      while (!(u[0] & 1)) {
        nn_halve(u, 0);
        halve_mod(x1);
      }
      while (!(v[0] & 1)) {
        nn_halve(v, 0);
        halve_mod(x2);
      }
      if (nn_cmp(u, v) >= 0) {
        nn_sub(u, u, v);
        sub_mod(x1, x1, x2);
      } else {
        nn_sub(v, v, u);
        sub_mod(x2, x2, x1);
      }
    }
    const uint32_t *r = nn_is_one(u) ? x1 : x2;
    for (uint32_t i = 0; i < NN_LIMBS; i++) out[i] = r[i];
    return true;
  }
};

}  // namespace p2
