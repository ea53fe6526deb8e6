// bigdiv.hpp -- the long division behind BigUintDivRemGenerator (plonky2_ecdsa/biguint/biguint.rs:337-344: a.div_rem(&b) on
// the limbs' integers), on 32-bit words: Knuth's algorithm D (TAOCP 4.3.1), one lane's worth of state in BigDiv.  Plain C++
// besides P2_HD, as genops.hpp is: g++ compiles it (csrc/tests/bigdiv_check.cpp, tests/test_bigdiv_host.py) and the level walk
// runs the same text (generators.hpp gen_biguint_divrem).
//   limbs   a limb is a canonical field element, so up to 64 bits: push() adds limb_i * 2^(32 i) with carries, as
//           `get_biguint_target` folds them; `count` limbs give at most count + 2 words.
//   divide  leading zero words of both are dropped; a one-word divisor takes the short path; otherwise both are shifted by
//           the divisor's leading zeros, every quotient word is estimated from the top two words of the running remainder,
//           corrected against the third, multiplied and subtracted, and added back when the subtraction went negative.
//           The quotient word of position j is stored in u[j + nv], the word the subtraction has just cleared: after divide()
//           the remainder is u[0 .. nv) and the quotient u[nv .. nv + nq).
#pragma once
#include "gl.hpp"

namespace p2 {

constexpr uint32_t BIGDIV_MAX_A = 32, BIGDIV_MAX_B = 16;  // limbs of the dividend and of the divisor (p2gpu.h)

struct BigDiv {
  uint32_t u[BIGDIV_MAX_A + 3];  // the dividend's words, one more for the shift; then remainder and quotient
  uint32_t v[BIGDIV_MAX_B + 2];  // the divisor's words
  uint32_t nu = 0, nv = 0, nq = 0;
  uint64_t carry = 0;            // of push(): < 2^33

  // word `i` of the number that is being loaded into `w`, from limb i
  P2_HD void push(uint32_t *w, uint32_t i, uint64_t limb) {
    const uint64_t s = (limb & 0xFFFFFFFFull) + (carry & 0xFFFFFFFFull);
    w[i] = (uint32_t)s;
    carry = (limb >> 32) + (carry >> 32) + (s >> 32);  // <= 2^32 - 1 + 1 + 1
  }
  // the two words behind the last limb; returns the number of words without the leading zeros
  P2_HD uint32_t finish(uint32_t *w, uint32_t count) {
    w[count] = (uint32_t)carry;
    w[count + 1] = (uint32_t)(carry >> 32);
    carry = 0;
    uint32_t m = count + 2;
    while (m && !w[m - 1]) m--;
    return m;
  }
  P2_HD void push_a(uint32_t i, uint64_t limb) { push(u, i, limb); }
  P2_HD void push_b(uint32_t i, uint64_t limb) { push(v, i, limb); }
  P2_HD void finish_a(uint32_t la) { nu = finish(u, la); }
  P2_HD void finish_b(uint32_t lb) { nv = finish(v, lb); }

  P2_HD uint32_t quotient_word(uint32_t i) const { return i < nq ? u[nv + i] : 0u; }
  P2_HD uint32_t remainder_word(uint32_t i) const { return i < nv ? u[i] : 0u; }

  // false: the divisor is zero.  add_backs (may be null): counts the add-back steps, for the host test
  P2_HD bool divide(uint32_t *add_backs = nullptr) {
    const uint32_t m = nu, n = nv;
    if (n == 0) return false;
    if (m < n) {  // the quotient is zero, the remainder the dividend
      for (uint32_t i = m; i < n; i++) u[i] = 0;
      nq = 0;
      return true;
    }
    nq = m - n + 1;
    if (n == 1) {
      const uint32_t d = v[0];
      uint64_t rem = 0;
      for (uint32_t j = m; j-- > 0;) {
        const uint64_t cur = (rem << 32) | u[j];
        u[j + 1] = (uint32_t)(cur / d);
        rem = cur % d;
      }
      u[0] = (uint32_t)rem;
      return true;
    }
    // normalise: the divisor's top bit set
    uint32_t s = 0;
    for (uint32_t t = v[n - 1]; !(t & 0x80000000u); t <<= 1) s++;
    if (s) {
      for (uint32_t i = n - 1; i > 0; i--) v[i] = (v[i] << s) | (v[i - 1] >> (32 - s));
      v[0] <<= s;
      u[m] = u[m - 1] >> (32 - s);
      for (uint32_t i = m - 1; i > 0; i--) u[i] = (u[i] << s) | (u[i - 1] >> (32 - s));
      u[0] <<= s;
    } else {
      u[m] = 0;
    }
    const uint64_t vt = v[n - 1], vs = v[n - 2];
    for (uint32_t j = m - n + 1; j-- > 0;) {
      const uint64_t num = ((uint64_t)u[j + n] << 32) | u[j + n - 1];
      uint64_t qhat = num / vt, rhat = num % vt;
      while (qhat >> 32 || qhat * vs > ((rhat << 32) | u[j + n - 2])) {
        qhat--;
        rhat += vt;
        if (rhat >> 32) break;
      }
      // u[j .. j + n] -= qhat * v
      uint64_t carry_mul = 0;
      int64_t t, borrow = 0;
      for (uint32_t i = 0; i < n; i++) {
        const uint64_t p = qhat * v[i] + carry_mul;  // (32 x 32 + 32 bits)
        carry_mul = p >> 32;
        t = (int64_t)u[i + j] - (int64_t)(p & 0xFFFFFFFFull) - borrow;
        u[i + j] = (uint32_t)t;
        borrow = t < 0 ? 1 : 0;
      }
      t = (int64_t)u[j + n] - (int64_t)carry_mul - borrow;
      if (t < 0) {  // one too many: add the divisor back
        qhat--;
        if (add_backs) ++*add_backs;
        uint64_t c = 0;
        for (uint32_t i = 0; i < n; i++) {
          const uint64_t sum = (uint64_t)u[i + j] + v[i] + c;
          u[i + j] = (uint32_t)sum;
          c = sum >> 32;
        }
      }
      u[j + n] = (uint32_t)qhat;  // (the running remainder's word here is zero from now on)
    }
    // the remainder, shifted back; u[n] is the quotient's already
    if (s) {
      for (uint32_t i = 0; i + 1 < n; i++) u[i] = (u[i] >> s) | (u[i + 1] << (32 - s));
      u[n - 1] >>= s;
    }
    return true;
  }
};

}  // namespace p2
