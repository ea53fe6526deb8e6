// columns.hip -- the class of every column of a batch (ColHints: zero, a multiple of a unit column, dense) and the clean marks of
// the buffers their transforms are written to.  Read by upload.hip, commit.hip and prover.hip; the transforms of the structured
// classes are ntt.hip structured_fill_kernel.
#include "internal.hpp"
#include <algorithm>

namespace p2 {

// Class of every column of vals [cols][n] (flags zeroed by the launcher): 0 = zero in every row; 1 = zero in every
// row but `sparse_row`, whose value goes to scalar[c]; 2 = anything else.  plonky2's build() hangs a random value
// on every unused wire of the PublicInputGate row (circuit_builder.rs randomize_unused_pi_wires; visible in the
// reference's own proofs, tests/golden/reference_proofs.py), so in a real witness the wires no gate uses are
// class 1 with that row, not class 0.  sparse_row = UINT32_MAX: no such row.
__global__ __launch_bounds__(256) void column_nonzero_kernel(const gl_t *__restrict__ vals, uint32_t d, SparseRows rows,
                                                             uint32_t *flags, gl_t *scalar, uint32_t sstride) {
  const size_t n = (size_t)1 << d;
  const gl_t *p = vals + (size_t)blockIdx.y * n;
  uint64_t acc = 0;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  const uint32_t r0 = rows.row[0], r1 = rows.row[1], r2 = rows.row[2], r3 = rows.row[3];  // UINT32_MAX: never matches
#pragma unroll 8
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
    const gl_t v = p[i];
    acc |= (i == r0 || i == r1 || i == r2 || i == r3) ? (gl_t)0 : v;  // a select, not a branch: the loads stay batched
  }
  // dense: a plain store (every wave of a dense column would otherwise hammer one address with atomics); the other
  // classes are told apart from the special rows' values by column_class_kernel, launched behind this one
  if (__any(acc != 0) && (threadIdx.x & 63) == 0) flags[blockIdx.y] = 2u;
  if (blockIdx.x == 0 && threadIdx.x < rows.count) scalar[(size_t)threadIdx.x * sstride + blockIdx.y] = p[rows.row[threadIdx.x]];
}
__global__ void column_class_kernel(uint32_t *flags, const gl_t *scalar, uint32_t sstride, uint32_t nrows, uint32_t cols) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols || flags[c] == 2u) return;
  bool more = false;
  for (uint32_t s = 1; s < nrows; s++) more |= scalar[(size_t)s * sstride + c] != 0;
  flags[c] = more ? 3u : ((nrows && scalar[c] != 0) ? 1u : 0u);
}
// "clean" bookkeeping of the buffers a column's transforms are written to (coefficients + LDE), so that the zeros of
// an unused wire are stored once per handle instead of once per proof.  Both steps are stream-ordered around the
// transforms: BEFORE them a non-zero column loses its clean mark (its buffers are about to be overwritten), AFTER them
// a zero column gains it (its buffers now hold zeros).  Anything that aborts in between leaves marks only cleared.
__global__ void column_clean_kernel(const uint32_t *nz, uint32_t cols, uint32_t *clean, int after) {
  const uint32_t c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  if (after) {
    if (nz[c] == 0) clean[c] = 1;
  } else {
    if (nz[c] != 0) clean[c] = 0;
  }
}
void column_clean_update(hipStream_t st, const uint32_t *nz, uint32_t cols, uint32_t *clean, bool after) {
  if (!cols) return;
  hipLaunchKernelGGL(column_clean_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, nz, cols, clean, after ? 1 : 0);
}
void column_flags(hipStream_t st, const gl_t *vals, uint32_t cols, uint32_t d, const SparseRows &rows, uint32_t *flags,
                  gl_t *scalar, uint32_t sstride) {
  if (!cols) return;
  (void)hipMemsetAsync(flags, 0, sizeof(uint32_t) * cols, st);
  const size_t n = (size_t)1 << d;
  const uint32_t bx = (uint32_t)std::max<size_t>(1, n / (256 * 8));
  ProfScope ps("column_nonzero_kernel", 8.0 * cols * (double)n);
  hipLaunchKernelGGL(column_nonzero_kernel, dim3(bx, cols), dim3(256), 0, st, vals, d, rows, flags, scalar, sstride);
  hipLaunchKernelGGL(column_class_kernel, dim3((cols + 255) / 256), dim3(256), 0, st, flags, scalar, sstride, rows.count, cols);
}

}  // namespace p2
