// witness.hip -- row-local witness filling on the GPU (SURVEY.md 8(f) "N1").
//
// After `generate_partial_witness` has propagated the copy constraints (CPU, Rust), what is
// left of witness generation is row-local: every gate's own SimpleGenerator derives the rest
// of its row -- limb decompositions, carries, inverses, S-box inputs -- from the row's input
// wires.  For the reference's circuits that is every NON-ROUTED column (154 of 234): the
// host only has to provide the 80 routed columns (84 MB instead of 245 MB over PCIe at 2^17
// rows) and this kernel fills the rest in HBM, one lane per row, column-major (unit-stride
// across the wave for every column).
//
// Restated generators (plonky2-backend/src/plonky2_ecdsa/biguint/gates/):
//   arithmetic_u32.rs:376-426, add_many_u32.rs:329-378, subtraction_u32.rs:298-343,
//   range_check_u32.rs:198-220, comparison.rs:439-537
// and the stock plonky2 ones (ArithmeticBaseGenerator, BaseSplitGenerator,
// RandomAccessGenerator, ConstantGate wires, PoseidonGenerator).  The bodies live in generators.hpp: the level walk of
// p2gpu_generate_witness (genwit.hip) runs the same ones.
#include "generators.hpp"

namespace p2 {

struct FillArgs {
  gl_t *wires;             // [W][n], in place
  const uint8_t *row_gate; // [n] index into gates
  const GateDesc *gates;
  const gl_t *gconsts;     // [ngc][n] gate-constant columns (after the selector columns)
  const gl_t *prc;         // 360 Poseidon round constants (wave-uniform index -> scalar loads)
  uint32_t d, ngc;
};

// the row as fill_witness sees it: the wire matrix itself
struct RowWires {
  gl_t *w;              // wires + row
  const gl_t *gconsts;  // gate-constant columns + row
  size_t n;
  uint32_t ngc;
  __device__ __forceinline__ gl_t get(uint32_t col) const { return w[(size_t)col * n]; }
  __device__ __forceinline__ void set(uint32_t col, gl_t v) { w[(size_t)col * n] = v; }
  __device__ __forceinline__ gl_t lc(uint32_t i) const { return i < ngc ? gconsts[(size_t)i * n] : (gl_t)0; }
  __device__ __forceinline__ void reject(uint32_t) {}
};

__global__ __launch_bounds__(256) void fill_witness_kernel(FillArgs a) {
  const size_t n = (size_t)1 << a.d;
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (row >= n) return;
  const GateDesc g = a.gates[a.row_gate[row]];
  RowWires w{a.wires + row, a.gconsts + row, n, a.ngc};
  switch (g.kind) {
  case G_CONSTANT:
    gen_constant(w, g);
    break;
  case G_ARITHMETIC: {
    const gl_t c0 = w.lc(0), c1 = w.lc(1);
    for (uint32_t i = 0; i < g.p[0]; i++) gen_arithmetic_op(w, i, c0, c1);
    break;
  }
  case G_BASE_SUM:
    gen_base_sum_split(w, g);
    break;
  case G_RANDOM_ACCESS:
    for (uint32_t cp = 0; cp < g.p[1]; cp++) gen_random_access_copy(w, g, cp);
    gen_random_access_consts(w, g);
    break;
  case G_POSEIDON:
    gen_poseidon(w, a.prc);
    break;
  case G_U32_ARITHMETIC:
    for (uint32_t i = 0; i < g.p[0]; i++) gen_u32_arithmetic_op(w, g, i);
    break;
  case G_U32_ADD_MANY:
    for (uint32_t i = 0; i < g.p[1]; i++) gen_u32_add_many_op(w, g, i);
    break;
  case G_U32_SUBTRACTION:
    for (uint32_t i = 0; i < g.p[0]; i++) gen_u32_subtraction_op(w, g, i);
    break;
  case G_U32_RANGE_CHECK:
    gen_u32_range_check(w, g);
    break;
  case G_COMPARISON:
    gen_comparison(w, g);
    break;
  default:
    break;
  }
}

void fill_witness(hipStream_t st, gl_t *wires, const uint8_t *row_gate, const GateDesc *gates, const gl_t *gconsts,
                  const gl_t *prc, uint32_t d, uint32_t ngc, uint32_t num_wires) {
  const size_t n = (size_t)1 << d;
  FillArgs a;
  a.wires = wires; a.row_gate = row_gate; a.gates = gates; a.gconsts = gconsts; a.prc = prc; a.d = d; a.ngc = ngc;
  ProfScope ps("fill_witness_kernel", 8.0 * (double)num_wires * (double)n);
  hipLaunchKernelGGL(fill_witness_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, a);
}

}  // namespace p2
