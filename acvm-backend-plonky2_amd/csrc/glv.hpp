// glv.hpp -- the arithmetic behind the GLVDecompositionGenerator (plonky2_ecdsa/curve/gadgets/glv.rs:50-88 decompose_secp256k1_scalar,
// :258-285 the generator): Algorithm 15.41 of the Handbook of Elliptic and Hyperelliptic Curve Cryptography on the secp256k1
// scalar field, on 32-bit words, built on nonnative.hpp.  Plain C++ besides P2_HD, as nonnative.hpp is: g++ compiles it
// (csrc/tests/glv_check.cpp, tests/test_glv_host.py) and the level walk runs the same text (generators.hpp gen_glv_decompose).
//   k       fold(k's limbs) mod N, as the nonnative generators reduce an operand (upstream's from_noncanonical_biguint).
//   c1, c2  round(B2 k / N), round(MINUS_B1 k / N): the 128 x 256-bit product in BigDiv's dividend, divided by N; the quotient
//           takes one more when 2 rem > N, which is rem > (N - 1) / 2 -- N is odd, a tie does not exist.  Both are below 2^128 + 1.
//   k1_raw  k - c1 A1 - c2 A2 mod N;  k2_raw = c1 MINUS_B1 - c2 B2 mod N  (k1_raw + GLV_S k2_raw = k).
//   signs   a raw value above (N - 1) / 2 is negative: its magnitude N - raw is what is kept.
#pragma once
#include "nonnative.hpp"

namespace p2 {

constexpr uint32_t GLV_LIMBS = 4;  // the limbs `decompose_secp256k1_scalar` gives k1 and k2 (glv.rs:126-127)
enum : uint32_t { GLV_A1 = 0, GLV_MINUS_B1, GLV_A2, GLV_B2, GLV_CONSTANTS };

// word i < NN_LIMBS of constant c < GLV_CONSTANTS (glv.rs:37-44)
P2_HD uint32_t glv_constant_word(uint32_t c, uint32_t i) {
  // 0x3086D221 A7D46BCD E86C90E4 9284EB15; 0xE4437ED6 010E8828 6F547FA9 0ABFE4C3; 0x1 14CA50F7 A8E2F3F6 57C1108D 9D44CFD8; B2 = A1
  const uint32_t table[GLV_CONSTANTS][5] = {{0x9284EB15u, 0xE86C90E4u, 0xA7D46BCDu, 0x3086D221u, 0u},
                                            {0x0ABFE4C3u, 0x6F547FA9u, 0x010E8828u, 0xE4437ED6u, 0u},
                                            {0x9D44CFD8u, 0x57C1108Du, 0xA8E2F3F6u, 0x14CA50F7u, 1u},
                                            {0x9284EB15u, 0xE86C90E4u, 0xA7D46BCDu, 0x3086D221u, 0u}};
  return i < 5 ? table[c][i] : 0u;
}

struct Glv {
  NonNative f;
  uint32_t k1[NN_LIMBS], k2[NN_LIMBS];  // the magnitudes
  bool k1_neg = false, k2_neg = false;

  P2_HD Glv() : f(NN_FIELD_SECP256K1_SCALAR) {}

  P2_HD void constant(uint32_t c, uint32_t *out) const {
    for (uint32_t i = 0; i < NN_LIMBS; i++) out[i] = glv_constant_word(c, i);
  }
  // out = round(constant c * k / N) for k < N
  P2_HD void rounded_quotient(uint32_t c, const uint32_t *k, const uint32_t *half, uint32_t *out) {
    uint32_t t[NN_LIMBS];
    constant(c, t);
    f.mul_divmod(t, k);
    for (uint32_t i = 0; i < NN_LIMBS; i++) out[i] = f.w.quotient_word(i), t[i] = f.w.remainder_word(i);
    if (nn_cmp(t, half) > 0) {  // 2 rem > N
      uint64_t carry = 1;
      for (uint32_t i = 0; i < NN_LIMBS; i++) {
        carry += out[i];
        out[i] = (uint32_t)carry;
        carry >>= 32;
      }
    }
  }
  // r = r - constant c * x mod N for r, x < N
  P2_HD void sub_product(uint32_t *r, uint32_t c, const uint32_t *x) {
    uint32_t t[NN_LIMBS];
    constant(c, t);
    f.mul_divmod(t, x);
    for (uint32_t i = 0; i < NN_LIMBS; i++) t[i] = f.w.remainder_word(i);
    f.sub_mod(r, r, t);
  }
  // raw > (N - 1) / 2: raw = N - raw; returns that sign
  P2_HD bool magnitude(uint32_t *raw, const uint32_t *half) const {
    const bool neg = nn_cmp(raw, half) > 0;
    if (neg) nn_sub(raw, f.m, raw);
    return neg;
  }
  // k < N, eight words: k1, k2 and the signs
  P2_HD void decompose(const uint32_t *k) {
    uint32_t half[NN_LIMBS], c1[NN_LIMBS], c2[NN_LIMBS];
    for (uint32_t i = 0; i < NN_LIMBS; i++) half[i] = f.m[i];
    nn_halve(half, 0);  // (N - 1) / 2
    rounded_quotient(GLV_B2, k, half, c1);
    rounded_quotient(GLV_MINUS_B1, k, half, c2);
    for (uint32_t i = 0; i < NN_LIMBS; i++) k1[i] = k[i], k2[i] = 0;
    sub_product(k1, GLV_A1, c1);
    sub_product(k1, GLV_A2, c2);
    // k2 = 0 - c2 B2 - (0 - c1 MINUS_B1)
    sub_product(k2, GLV_B2, c2);
    for (uint32_t i = 0; i < NN_LIMBS; i++) c2[i] = 0;
    sub_product(c2, GLV_MINUS_B1, c1);
    f.sub_mod(k2, k2, c2);
    k1_neg = magnitude(k1, half);
    k2_neg = magnitude(k2, half);
  }
};

}  // namespace p2
