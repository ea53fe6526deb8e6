// tables.hip -- the per-handle tables around the transforms: powers of a root (the w_n^i tables of plonk.hip / fri.hip) and the
// coset scales the coefficients -> values transforms multiply into their bit-reversed input (ntt_batch `scale`).
#include "internal.hpp"

namespace p2 {

// tw[i] = root^i for i < count
__global__ void powers_kernel(gl_t *out, gl_t root, uint32_t count) {
  uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) out[i] = gl_pow(root, i);
}
// scale[c][p] = (shift * wN^c)^(bitrev_d(p)) * mult
__global__ void coset_scale_kernel(gl_t *out, gl_t shift, gl_t wN, uint32_t d, uint32_t cosets, gl_t mult) {
  uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t c = blockIdx.y;
  if (p >= (1u << d)) return;
  gl_t base = gl_mul(shift, gl_pow(wN, c));
  out[((size_t)c << d) + p] = gl_mul(gl_pow(base, bitrev32(p, d)), mult);
}

void fill_powers(hipStream_t st, gl_t *out, gl_t root, uint32_t count) {
  if (!count) return;
  hipLaunchKernelGGL(powers_kernel, dim3((count + 255) / 256), dim3(256), 0, st, out, root, count);
}
void fill_coset_scale(hipStream_t st, gl_t *out, gl_t shift, gl_t wN, uint32_t d, uint32_t cosets, gl_t mult) {
  uint32_t n = 1u << d;
  hipLaunchKernelGGL(coset_scale_kernel, dim3((n + 255) / 256, cosets), dim3(256), 0, st, out, shift, wN, d, cosets,
                     mult);
}

}  // namespace p2
