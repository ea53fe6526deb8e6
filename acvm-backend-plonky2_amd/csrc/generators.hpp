// generators.hpp -- the gates' witness generators, one body each, shared by the two kernels that run them:
//   fill_witness_kernel (witness.hip)  one lane per row, straight on the wire matrix;
//   genwit_walk_kernel  (genwit.hip)   one lane per scheduled op and witness of the batch, on that witness's class values.
// A body sees its row through an accessor A:
//   gl_t get(col)            the wire's value
//   void set(col, gl_t v)    a derived wire (the level walk compares instead when the wire's class already has a value)
//   gl_t lc(i)               gate constant i of the row
//   void reject(col)         the inputs admit no value for `col` (fill_witness: nothing -- it derives, it does not judge)
// Restated generators: witness.hip's header lists their sources.  gen_base_sum_join is the one le_sum adds
// (gadgets/split_join.rs: the sum is computed from the bits), every other body is what fill_witness_kernel always ran.
#pragma once
#include "bigdiv.hpp"
#include "glv.hpp"
#include "internal.hpp"
#include "nonnative.hpp"
#include "poseidon.hpp"

namespace p2 {

template <class A>
__device__ __forceinline__ void gen_constant(A &a, const GateDesc &g) {
  for (uint32_t i = 0; i < g.p[0]; i++) a.set(i, a.lc(i));
}

template <class A>
__device__ __forceinline__ void gen_arithmetic_op(A &a, uint32_t i, gl_t c0, gl_t c1) {
  a.set(4 * i + 3, gl_add(gl_mul(gl_mul(a.get(4 * i), a.get(4 * i + 1)), c0), gl_mul(a.get(4 * i + 2), c1)));
}

// BaseSplitGenerator: sum -> limbs
template <class A>
__device__ __forceinline__ void gen_base_sum_split(A &a, const GateDesc &g) {
  uint64_t v = a.get(0);
  const uint32_t B = g.p[0];
  for (uint32_t i = 0; i < g.p[1]; i++) {
    a.set(1 + i, v % B);
    v /= B;
  }
  if (v) a.reject(0);  // the sum does not fit the limbs
}

// limbs -> sum (Horner from the top limb)
template <class A>
__device__ __forceinline__ void gen_base_sum_join(A &a, const GateDesc &g) {
  const uint32_t B = g.p[0];
  gl_t s = 0;
  for (uint32_t i = g.p[1]; i-- > 0;) {
    const gl_t l = a.get(1 + i);
    if (l >= B) a.reject(1 + i);
    s = gl_add(gl_mul(s, B), l);
  }
  a.set(0, s);
}

template <class A>
__device__ __forceinline__ void gen_random_access_copy(A &a, const GateDesc &g, uint32_t cp) {
  const uint32_t bits = g.p[0], copies = g.p[1], extra = g.p[2], vec = 1u << bits;
  const uint32_t routed = (2 + vec) * copies + extra, base = (2 + vec) * cp;
  const uint64_t idx = a.get(base);
  a.set(base + 1, a.get(base + 2 + (uint32_t)(idx & (vec - 1))));
  for (uint32_t k = 0; k < bits; k++) a.set(routed + cp * bits + k, (idx >> k) & 1);
}

template <class A>
__device__ __forceinline__ void gen_random_access_consts(A &a, const GateDesc &g) {
  const uint32_t copies = g.p[1], extra = g.p[2], vec = 1u << g.p[0];
  for (uint32_t i = 0; i < extra; i++) a.set((2 + vec) * copies + i, a.lc(i));
}

// EqualityGenerator (gadgets/arithmetic.rs `is_equal`): no gate's own -- its accessor numbers the generator's four cells
// x, y, equal, inv instead of a row's columns.  gl_inv(0) = 0 is the equal case.
template <class A>
__device__ __forceinline__ void gen_equality(A &a) {
  const gl_t diff = gl_sub(a.get(0), a.get(1));
  a.set(2, diff == 0 ? 1 : 0);
  a.set(3, gl_inv(diff));
}

// BigUintDivRemGenerator (plonky2_ecdsa/biguint/biguint.rs:317-344, registered by `div_rem_biguint` :246): no gate's own either.
// Its accessor numbers the cells a[0 .. la), b[0 .. lb) (read), div[0 .. ld), rem[0 .. lr) (set), least significant limb first;
// shape = {la, lb, ld, lr} as the plan checked it (la <= 32, lb <= 16).  The limbs are folded as `get_biguint_target` folds them
// (a limb >= 2^32 carries), divided by bigdiv.hpp, and written as 32-bit digits.  Where upstream panics the walk rejects: b = 0
// on b's first cell; a quotient or remainder with more digits than its target has limbs on that target's top limb (the
// quotient of a target without limbs: on a's first cell).  Not forced inline: its word arrays live in private memory, and the
// caller keeps them out of the other generators' frames (genwit.hip).
template <class A>
__device__ void gen_biguint_divrem(A &a, const uint32_t shape[4]) {
  const uint32_t la = shape[0], lb = shape[1], ld = shape[2], lr = shape[3];
  BigDiv w;
  for (uint32_t i = 0; i < la; i++) w.push_a(i, a.get(i));
  w.finish_a(la);
  for (uint32_t i = 0; i < lb; i++) w.push_b(i, a.get(la + i));
  w.finish_b(lb);
  if (!w.divide()) {
    a.reject(la);
    return;
  }
  for (uint32_t i = 0; i < ld; i++) a.set(la + lb + i, w.quotient_word(i));
  for (uint32_t i = 0; i < lr; i++) a.set(la + lb + ld + i, w.remainder_word(i));
  bool q_over = false, r_over = false;
  for (uint32_t i = ld; i < w.nq; i++) q_over |= w.quotient_word(i) != 0;
  for (uint32_t i = lr; i < w.nv; i++) r_over |= w.remainder_word(i) != 0;
  if (q_over) a.reject(ld ? la + lb + ld - 1 : 0);
  if (r_over) a.reject(la + lb + ld + lr - 1);
}

// The four nonnative generators (plonky2_ecdsa/biguint/gadgets/nonnative.rs, registered by `add_nonnative` :193, `sub_nonnative`
// :292, `mul_nonnative` :323, `inv_nonnative` :370): no gate's own.  Their accessor numbers the cells a[0 .. la), b[0 .. lb) (read)
// and then the two targets they set, least significant limb first; shape as the plan checked it (la, lb <= 16), field < NN_FIELDS
// from the op record.  M is the field's modulus, A = fold(a) mod M, B = fold(b) mod M (nonnative.hpp: upstream's
// FF::from_noncanonical_biguint); what is set are 32-bit digits, zeros in the limbs beyond them.  Where upstream panics the walk
// rejects, by the div-rem generator's rule: a value with more digits than its target has limbs on that target's top limb (on
// the generator's first cell when the target has no limbs), the inverse of zero on x's first cell.  Not forced inline, for the
// reason gen_biguint_divrem is not.
template <class A>
__device__ __forceinline__ void nn_load(A &a, NonNative &f, uint32_t first, uint32_t count, uint32_t *out) {
  for (uint32_t i = 0; i < count; i++) f.push(i, a.get(first + i));
  f.reduce(count, out);
}
// word(0) .. word(digits - 1) into the `limbs` cells from `first` on
template <class A, class F>
__device__ __forceinline__ void nn_store(A &a, uint32_t first, uint32_t limbs, uint32_t digits, F &&word) {
  for (uint32_t i = 0; i < limbs; i++) a.set(first + i, i < digits ? (gl_t)word(i) : (gl_t)0);
  bool over = false;
  for (uint32_t i = limbs; i < digits; i++) over |= word(i) != 0;
  if (over) a.reject(limbs ? first + limbs - 1 : 0);
}

// NonNativeAdditionGenerator (:469-484): S = A + B; S > M (strictly, as upstream: A + B = M leaves sum = M): sum = S - M,
// overflow = 1; otherwise sum = S, overflow = 0.  shape {la, lb, 8, 1}
template <class A>
__device__ void gen_nonnative_add(A &a, const uint32_t shape[4], uint32_t field) {
  const uint32_t la = shape[0], lb = shape[1], out = la + lb;
  NonNative f(field);
  uint32_t x[NN_LIMBS], y[NN_LIMBS];
  nn_load(a, f, 0, la, x);
  nn_load(a, f, la, lb, y);
  const bool over = f.add_once(x, y);
  nn_store(a, out, shape[2], NN_LIMBS, [&](uint32_t i) { return x[i]; });
  nn_store(a, out + shape[2], shape[3], 1, [&](uint32_t) { return over ? 1u : 0u; });
}

// NonNativeSubtractionGenerator (:589-604): A >= B: diff = A - B, overflow = 0; otherwise diff = M + A - B, overflow = 1.
// shape {la, lb, 8, 1}
template <class A>
__device__ void gen_nonnative_sub(A &a, const uint32_t shape[4], uint32_t field) {
  const uint32_t la = shape[0], lb = shape[1], out = la + lb;
  NonNative f(field);
  uint32_t x[NN_LIMBS], y[NN_LIMBS];
  nn_load(a, f, 0, la, x);
  nn_load(a, f, la, lb, y);
  const bool over = f.sub_once(x, y);
  nn_store(a, out, shape[2], NN_LIMBS, [&](uint32_t i) { return x[i]; });
  nn_store(a, out + shape[2], shape[3], 1, [&](uint32_t) { return over ? 1u : 0u; });
}

// NonNativeMultiplicationGenerator (:645-658): (Q, R) = divmod(A B, M); prod = R, overflow = Q.  shape {la, lb, 8, la + lb - 8}
template <class A>
__device__ void gen_nonnative_mul(A &a, const uint32_t shape[4], uint32_t field) {
  const uint32_t la = shape[0], lb = shape[1], out = la + lb;
  NonNative f(field);
  uint32_t x[NN_LIMBS], y[NN_LIMBS];
  nn_load(a, f, 0, la, x);
  nn_load(a, f, la, lb, y);
  f.mul_divmod(x, y);
  nn_store(a, out, shape[2], NN_LIMBS, [&](uint32_t i) { return f.w.remainder_word(i); });
  nn_store(a, out + shape[2], shape[3], f.w.nq, [&](uint32_t i) { return f.w.quotient_word(i); });
}

// NonNativeInverseGenerator (:691-703): X = fold(x) mod M, inv = X^-1 mod M, div = (X inv) div M.  shape {lx, 0, lx, lx}
template <class A>
__device__ void gen_nonnative_inv(A &a, const uint32_t shape[4], uint32_t field) {
  const uint32_t lx = shape[0], out = lx + shape[1];
  NonNative f(field);
  uint32_t x[NN_LIMBS], inv[NN_LIMBS];
  nn_load(a, f, 0, lx, x);
  if (!f.invert(x, inv)) {
    a.reject(0);
    return;
  }
  nn_store(a, out, shape[2], NN_LIMBS, [&](uint32_t i) { return inv[i]; });
  f.mul_divmod(x, inv);
  nn_store(a, out + shape[2], shape[3], f.w.nq, [&](uint32_t i) { return f.w.quotient_word(i); });
}

// GLVDecompositionGenerator (plonky2_ecdsa/curve/gadgets/glv.rs:258-285, registered by `decompose_secp256k1_scalar` :131): no
// gate's own.  Its accessor numbers the cells k[0 .. lk) (read), then k1's four limbs, k2's four, k1_neg, k2_neg (set); shape
// {lk, 0, 8, 2} as the plan checked it.  K = fold(k) mod N, N the scalar field's order; glv.hpp decomposes it.  A magnitude above
// 128 bits (none is known: the lattice basis keeps both below 2^128) rejects on that target's top limb, by nn_store's rule.  Not
// forced inline, for the reason gen_biguint_divrem is not.
template <class A>
__device__ void gen_glv_decompose(A &a, const uint32_t shape[4]) {
  const uint32_t lk = shape[0], out = lk + shape[1], half = shape[2] / 2;
  Glv g;
  uint32_t k[NN_LIMBS];
  nn_load(a, g.f, 0, lk, k);
  g.decompose(k);
  nn_store(a, out, half, NN_LIMBS, [&](uint32_t i) { return g.k1[i]; });
  nn_store(a, out + half, half, NN_LIMBS, [&](uint32_t i) { return g.k2[i]; });
  a.set(out + 2 * half, g.k1_neg ? 1 : 0);
  a.set(out + 2 * half + 1, g.k2_neg ? 1 : 0);
}

// prc: the 360 round constants (wave-uniform index -> scalar loads)
template <class A>
__device__ __forceinline__ void gen_poseidon(A &a, const gl_t *prc) {
  gl_t st[12];
  const gl_t swap = a.get(24);
#pragma unroll
  for (int i = 0; i < 4; i++) {
    const gl_t l = a.get(i), r = a.get(i + 4);
    const gl_t dl = gl_mul(swap, gl_sub(r, l));
    a.set(25 + i, dl);
    st[i] = gl_add(l, dl);
    st[i + 4] = gl_sub(r, dl);
  }
#pragma unroll
  for (int i = 8; i < 12; i++) st[i] = a.get(i);
#pragma unroll 1
  for (int r = 0; r < 30; r++) {
#pragma unroll
    for (int i = 0; i < 12; i++) st[i] = gl_add(st[i], prc[12 * r + i]);
    const bool full = r < 4 || r >= 26;
    if (full) {
      if (r != 0) {
        const uint32_t base = r < 4 ? 29 + 12 * (r - 1) : 87 + 12 * (r - 26);
#pragma unroll
        for (int i = 0; i < 12; i++) a.set(base + i, st[i]);
      }
#pragma unroll
      for (int i = 0; i < 12; i++) st[i] = poseidon_sbox(st[i]);
    } else {
      a.set(65 + (r - 4), st[0]);
      st[0] = poseidon_sbox(st[0]);
    }
    poseidon_mds(st);
  }
#pragma unroll
  for (int i = 0; i < 12; i++) a.set(12 + i, st[i]);
}

template <class A>
__device__ __forceinline__ void gen_u32_arithmetic_op(A &a, const GateDesc &g, uint32_t i) {
  const uint32_t ops = g.p[0];
  uint64_t o = gl_add(gl_mul(a.get(6 * i), a.get(6 * i + 1)), a.get(6 * i + 2));
  const uint64_t hi = o >> 32, lo = o & 0xFFFFFFFFULL;
  a.set(6 * i + 3, lo);
  a.set(6 * i + 4, hi);
  const uint64_t diff = 0xFFFFFFFFULL - hi;
  a.set(6 * i + 5, diff ? gl_inv(diff) : 0);
  for (uint32_t j = 0; j < 32; j++) {
    a.set(6 * ops + 32 * i + j, o & 3);
    o >>= 2;
  }
}

template <class A>
__device__ __forceinline__ void gen_u32_add_many_op(A &a, const GateDesc &g, uint32_t i) {
  const uint32_t na = g.p[0], ops = g.p[1];
  const uint32_t b = (na + 3) * i;
  gl_t sum = 0;
  for (uint32_t j = 0; j <= na; j++) sum = gl_add(sum, a.get(b + j));
  const uint64_t res = sum & 0xFFFFFFFFULL, carry = sum >> 32;
  a.set(b + na + 1, res);
  a.set(b + na + 2, carry);
  for (uint32_t j = 0; j < 16; j++) a.set((na + 3) * ops + 18 * i + j, (res >> (2 * j)) & 3);
  for (uint32_t j = 0; j < 2; j++) a.set((na + 3) * ops + 18 * i + 16 + j, (carry >> (2 * j)) & 3);
}

template <class A>
__device__ __forceinline__ void gen_u32_subtraction_op(A &a, const GateDesc &g, uint32_t i) {
  const uint32_t ops = g.p[0];
  const gl_t init = gl_sub(gl_sub(a.get(5 * i), a.get(5 * i + 1)), a.get(5 * i + 2));
  const gl_t bout = init > (1ULL << 32) ? 1 : 0;
  const gl_t res = gl_add(init, gl_mul(bout, 1ULL << 32));
  a.set(5 * i + 3, res);
  a.set(5 * i + 4, bout);
  for (uint32_t j = 0; j < 16; j++) a.set(5 * ops + 16 * i + j, (res >> (2 * j)) & 3);
}

template <class A>
__device__ __forceinline__ void gen_u32_range_check(A &a, const GateDesc &g) {
  const uint32_t nl = g.p[0];
  for (uint32_t i = 0; i < nl; i++) {
    const uint32_t v = (uint32_t)a.get(i);
    for (uint32_t j = 0; j < 16; j++) a.set(nl + 16 * i + j, (v >> (2 * j)) & 3);
  }
}

template <class A>
__device__ __forceinline__ void gen_comparison(A &a, const GateDesc &g) {
  const uint32_t nb = g.p[0], nc = g.p[1], cb = (nb + nc - 1) / nc;
  const uint64_t a0 = a.get(0), b0 = a.get(1), cs = 1ULL << cb;
  uint64_t ta = a0, tb = b0;
  a.set(2, a0 <= b0 ? 1 : 0);
  gl_t msd = 0;
  for (uint32_t i = 0; i < nc; i++) {
    const gl_t f = ta % cs, s = tb % cs;
    ta /= cs;
    tb /= cs;
    a.set(4 + i, f);
    a.set(4 + nc + i, s);
    a.set(4 + 2 * nc + i, (f == s) ? 1 : gl_inv(gl_sub(s, f)));
    a.set(4 + 3 * nc + i, (f == s) ? 1 : 0);
    if (f != s) {
      msd = gl_sub(s, f);
      a.set(4 + 4 * nc + i, 0);
    } else {
      a.set(4 + 4 * nc + i, msd);
    }
  }
  a.set(3, msd);
  uint64_t v = gl_add(cs, msd);
  for (uint32_t i = 0; i < cb + 1; i++) {
    a.set(4 + 5 * nc + i, v & 1);
    v >>= 1;
  }
}

}  // namespace p2
