// selftest.hip -- kernels that exist only for the stage-level test operators (handle.hip p2gpu_field_selftest, p2gpu_ifft_batch,
// p2gpu_lde_batch).
#include "internal.hpp"

namespace p2 {

// ---- self-test of the field primitives (stage-level test operator p2gpu_field_selftest) -------------------
// a[i], b[i]: arbitrary u64.  Every carry-chain form of gl.hpp / mul_pow2 against the portable code, which is
// what the host and the oracle run: bad[0] canon, [1] add, [2] sub, [3] reduce128, [4] mul, [5] mul_add,
// [6] mul_pow2<1..95>, [7] Acc160, [8..13] the congruent-word (non-canonical) forms, [14..15] unused.
__global__ void field_selftest_kernel(const uint64_t *a, const uint64_t *b, uint32_t n, unsigned long long *bad) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint64_t x = a[i], y = b[i];
  const gl_t xc = gl_canon_c(x), yc = gl_canon_c(y);
  if (gl_canon(x) != xc) atomicAdd(&bad[0], 1ULL);
  if (gl_add(xc, yc) != gl_add_c(xc, yc)) atomicAdd(&bad[1], 1ULL);
  if (gl_sub(xc, yc) != gl_sub_c(xc, yc)) atomicAdd(&bad[2], 1ULL);
  if (gl_reduce128(x, y) != gl_reduce128_c(x, y)) atomicAdd(&bad[3], 1ULL);
  const uint64_t plo = xc * yc, phi = __umul64hi(xc, yc);
  const gl_t prod = gl_reduce128_c(plo, phi);
  if (gl_mul(xc, yc) != prod) atomicAdd(&bad[4], 1ULL);
  {
    uint64_t lo = plo + xc, hi = phi + (lo < xc);
    if (gl_mul_add(xc, yc, xc) != gl_reduce128_c(lo, hi)) atomicAdd(&bad[5], 1ULL);
  }
  gl_t pw = 1;
  bool ok = true;
  static_for<1, 96>([&](auto ec) {
    constexpr int e = decltype(ec)::value;
    pw = gl_add_c(pw, pw);
    const uint64_t l = xc * pw, h = __umul64hi(xc, pw);
    if (mul_pow2<e>(xc) != gl_reduce128_c(l, h)) ok = false;
  });
  if (!ok) atomicAdd(&bad[6], 1ULL);
  {
    Acc160 acc;
    acc.clear();
    acc.mac(xc, yc);
    acc.mac(yc, yc);
    acc.mac(xc, xc);
    const uint64_t l2 = yc * yc, h2 = __umul64hi(yc, yc), l3 = xc * xc, h3 = __umul64hi(xc, xc);
    const gl_t want = gl_add_c(gl_add_c(prod, gl_reduce128_c(l2, h2)), gl_reduce128_c(l3, h3));
    if (acc.value() != want) atomicAdd(&bad[7], 1ULL);
  }
  // The congruent-word forms (gl.hpp): operands ANY u64 -- x, y are used raw, so the edge set's words in [p, 2^64)
  // reach every branch -- result some u64 congruent to the canonical portable value.  [8] gl_mul_nc, [9] gl_mul_add_nc (one
  // factor canonical: the product plus the addend stays below 2^128), [10] gl_reduce128_nc, [11] gl_add / [12] gl_sub with a
  // non-canonical FIRST operand (a congruent word comes out; canonical when both operands are), [13] a chain: congruent words fed back into the congruent forms.
  if (gl_canon(gl_mul_nc(x, y)) != prod) atomicAdd(&bad[8], 1ULL);
  {
    uint64_t lo = plo + xc, hi = phi + (lo < xc);
    if (gl_canon(gl_mul_add_nc(x, yc, xc)) != gl_reduce128_c(lo, hi)) atomicAdd(&bad[9], 1ULL);
  }
  if (gl_canon(gl_reduce128_nc(x, y)) != gl_reduce128_c(x, y)) atomicAdd(&bad[10], 1ULL);
  if (gl_canon(gl_add(x, yc)) != gl_add_c(xc, yc) || gl_add(xc, yc) != gl_add_c(xc, yc)) atomicAdd(&bad[11], 1ULL);
  if (gl_canon(gl_sub(x, yc)) != gl_sub_c(xc, yc) || gl_sub(xc, yc) != gl_sub_c(xc, yc)) atomicAdd(&bad[12], 1ULL);
  {
    const uint64_t u = gl_mul_nc(x, y), v = gl_mul_add_nc(y, xc, yc);   // congruent to x y and y x + y
    const uint64_t w = gl_mul_nc(u, v);
    uint64_t l2 = plo + yc, h2 = phi + (l2 < yc);
    const gl_t vv = gl_reduce128_c(l2, h2);
    const uint64_t l3 = prod * vv, h3 = __umul64hi(prod, vv);
    if (gl_canon(w) != gl_reduce128_c(l3, h3)) atomicAdd(&bad[13], 1ULL);
    if (gl_canon(gl_add(w, xc)) != gl_add_c(gl_reduce128_c(l3, h3), xc)) atomicAdd(&bad[13], 1ULL);
    if (gl_canon(gl_sub(w, xc)) != gl_sub_c(gl_reduce128_c(l3, h3), xc)) atomicAdd(&bad[13], 1ULL);
  }
}
void field_selftest(hipStream_t st, const uint64_t *a, const uint64_t *b, uint32_t n, unsigned long long *bad) {
  hipLaunchKernelGGL(field_selftest_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a, b, n, bad);
}

// bit-reversal permutation of columns (only for the stage-level test operators
// that speak plonky2's natural-order coefficient convention)
__global__ void bitrev_cols_kernel(const gl_t *in, gl_t *out, uint32_t d, uint32_t cols) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t c = blockIdx.y;
  if (p >= (1u << d)) return;
  out[((size_t)c << d) + bitrev32(p, d)] = in[((size_t)c << d) + p];
}
void bitrev_cols(hipStream_t st, const gl_t *in, gl_t *out, uint32_t d, uint32_t cols) {
  uint32_t n = 1u << d;
  hipLaunchKernelGGL(bitrev_cols_kernel, dim3((n + 255) / 256, cols), dim3(256), 0, st, in, out, d, cols);
}

}  // namespace p2
