// build.hip -- `builder.build::<C>()` on the device: from the gate rows and the copy
// pairs, uploaded as they are, to the handle's resident tables -- row -> gate, gate constants, the special rows, and the sigma
// polynomials of the permutation argument (plonk/permutation_argument.rs WirePartition) -- without a blob in host memory.
// The host counterpart is p2gpu_build_blob (hostcore.hip); both give the same bytes (tests/test_gpu_device_build.py).
//
// Sigma: cells are numbered in the reference's listing order, key = row * R + col.
//   1. touch     every cell named by a copy pair becomes its own class and is appended once to the list of touched cells;
//   2. classes   rounds of hook / jump until no pair hooks: parent[x] = the smallest key of x's class (devclasses.hpp, the
//                union-find the device plan compiler shares);
//   3. cycles    sort the touched cells by (root, key); the successor of a cell is the next entry of its segment, the last
//                entry's successor is the root (= the segment's first entry);
//   4. values    sigma[col * n + row] = k_is[col'] * w^row', the identity for cells no pair names.
#include "devclasses.hpp"
#include "prover_internal.hpp"

using namespace p2;

namespace {

using classes::UNSET;
using classes::TPB;
using classes::grid_for;
using classes::subgroup_power;
// keys are < R * n <= MAX_ROUTED * 2^24 (circuit_parse: d <= 24): below UNSET, and (root, key) fits one 64-bit sort key
static_assert(((uint64_t)MAX_ROUTED << 24) <= ((uint64_t)1 << 31), "cell keys must stay below UNSET and 2 * key_bits below 64");

// the caller's copy pairs as devclasses.hpp's pair source: cells in the reference's listing order, key = row * R + col
struct CopyPairs {
  const uint4 *copies;
  uint32_t R;
  __device__ __forceinline__ bool get(size_t i, uint32_t &a, uint32_t &b) const {
    const uint4 e = copies[i];
    a = e.x * R + e.y;
    b = e.z * R + e.w;
    return true;
  }
};

// bad[0..2] = the smallest offending index of row_gate / the gate constants / the copy pairs (UINT64_MAX: none).  The only
// kernel that reads the caller's arrays unchecked, and it indexes nothing with them.
__global__ void build_validate_kernel(const uint32_t *row_gate, size_t n, uint32_t num_gates, const uint64_t *consts, size_t nconst,
                                      const uint4 *copies, size_t num_copies, uint32_t R, unsigned long long *bad) {
  const size_t total = max(max(n, nconst), num_copies), step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < total; i += step) {
    if (i < n && row_gate[i] >= num_gates) atomicMin(&bad[0], (unsigned long long)i);
    if (i < nconst && consts[i] >= GL_P) atomicMin(&bad[1], (unsigned long long)i);
    if (i < num_copies) {
      const uint4 e = copies[i];
      if (e.x >= n || e.z >= n || e.y >= R || e.w >= R) atomicMin(&bad[2], (unsigned long long)i);
    }
  }
}

__global__ void build_rows_kernel(const uint32_t *row_gate, size_t n, uint8_t *out) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t r = (size_t)blockIdx.x * TPB + threadIdx.x; r < n; r += step) out[r] = (uint8_t)row_gate[r];
}

// res[slot] = the first row >= (slot_after == UNSET ? 0 : res[slot_after] + 1) that holds a gate of `kind` (stays UNSET when
// there is none).  One atomic per wave at most: the lowest matching lane holds the wave's smallest row.
__global__ void build_first_row_kernel(const uint8_t *row_gate, const GateDesc *gates, size_t n, uint32_t kind, uint32_t slot,
                                       uint32_t slot_after, uint32_t *res) {
  uint32_t lo = 0;
  if (slot_after != UNSET) {
    const uint32_t prev = res[slot_after];
    if (prev == UNSET) return;
    lo = prev + 1;
  }
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t r0 = (size_t)blockIdx.x * TPB; r0 < n; r0 += step) {
    const size_t r = r0 + threadIdx.x;
    const bool hit = r < n && r >= lo && gates[row_gate[r]].kind == kind;
    const unsigned long long m = __ballot(hit);
    if (hit && (__lane_id() == (uint32_t)__ffsll((long long)m) - 1)) atomicMin(&res[slot], (uint32_t)r);
    if (m) return;  // (this wave's later tiles hold larger rows)
  }
}

__global__ void build_selectors_kernel(const uint8_t *row_gate, const GateDesc *gates, uint32_t num_selectors, size_t n, gl_t *out) {
  const uint32_t s = blockIdx.y;
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t r = (size_t)blockIdx.x * TPB + threadIdx.x; r < n; r += step) {
    const uint32_t gi = row_gate[r];
    out[(size_t)s * n + r] = (num_selectors == 1 || s == gates[gi].sel_index) ? (gl_t)gi : (gl_t)0xFFFFFFFFull;
  }
}

// list[i] = root << key_bits | key
__global__ void build_sort_keys_kernel(unsigned long long *list, size_t count, const uint32_t *parent, uint32_t key_bits) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < count; i += step) {
    const uint32_t x = (uint32_t)list[i];
    list[i] = ((unsigned long long)parent[x] << key_bits) | x;
  }
}

// the identity permutation: sigma[col][row] = k_is[col] * w^row, eight columns per thread
__global__ void build_sigma_identity_kernel(const gl_t *kis, const gl_t *tw, uint32_t d, uint32_t R, gl_t *sig) {
  const size_t n = (size_t)1 << d;
  const size_t row = (size_t)blockIdx.x * TPB + threadIdx.x;
  if (row >= n) return;
  const gl_t w = subgroup_power(tw, d, (uint32_t)row);
  const uint32_t c0 = blockIdx.y * 8, c1 = min(c0 + 8, R);
  for (uint32_t col = c0; col < c1; col++) sig[(size_t)col * n + row] = gl_mul(ld_uniform(kis + col), w);
}

__global__ void build_sigma_cycles_kernel(const unsigned long long *sorted, size_t count, uint32_t key_bits, uint32_t R, uint32_t d,
                                          const gl_t *kis, const gl_t *tw, gl_t *sig) {
  const unsigned long long mask = (1ull << key_bits) - 1;
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < count; i += step) {
    const unsigned long long k = sorted[i];
    const uint32_t x = (uint32_t)(k & mask), root = (uint32_t)(k >> key_bits);
    uint32_t next = root;
    if (i + 1 < count) {
      const unsigned long long k1 = sorted[i + 1];
      if ((uint32_t)(k1 >> key_bits) == root) next = (uint32_t)(k1 & mask);
    }
    const uint32_t row = x / R, col = x - row * R, row2 = next / R, col2 = next - row2 * R;
    sig[((size_t)col << d) + row] = gl_mul(kis[col2], subgroup_power(tw, d, row2));
  }
}

using BuildScratch = classes::Scratch;

}  // namespace

namespace p2 {

void build_selector_columns(hipStream_t st, const p2gpu_circuit *c, gl_t *consts) {
  hipLaunchKernelGGL(build_selectors_kernel, dim3(grid_for(c->n), c->num_selectors), dim3(TPB), 0, st, c->d_row_gate.p, c->d_gates.p,
                     c->num_selectors, c->n, consts);
}

int build_device_tables(p2gpu_circuit *c, const BuildInputs &in, const CreateTrace &tr) {
  hipStream_t st = c->stream;
  const size_t n = c->n, E = in.num_copies;
  const uint32_t R = c->R, d = c->d, ngc = c->NC - c->num_selectors;
  const size_t tot = (size_t)R * n, nconst = (size_t)ngc * n;
  uint32_t key_bits = 1;
  while (((size_t)1 << key_bits) < tot) key_bits++;
  if (tot >= UNSET || key_bits > 31) { set_err("p2gpu_circuit_build: %zu routed cells exceed 32-bit cell keys", tot); return P2GPU_E_ARG; }
  auto dev_fail = [&](const char *what, hipError_t e) {
    (void)hipGetLastError();
    set_err("p2gpu_circuit_build: %s: %s", what, hipGetErrorString(e));
    return P2GPU_E_DEVICE;
  };
#define BT(e, what)                                   \
  do {                                                \
    const hipError_t e_ = (e);                        \
    if (e_ != hipSuccess) return dev_fail(what, e_);  \
  } while (0)
  BuildScratch S;
  // ---- upload + validation ----
  uint32_t *rg32 = S.alloc<uint32_t>(n);
  uint4 *copies = S.alloc<uint4>(E);
  // [0..2] bad indices, [3] touched count, [5..6] special rows, [8]: the flag of one launch of the class loop
  unsigned long long *words = S.alloc<unsigned long long>(9);
  if (!rg32 || !copies || !words) return dev_fail("scratch", hipErrorOutOfMemory);
  uint32_t *flags = (uint32_t *)(words + 8), *rows = (uint32_t *)(words + 5);
  BT(hipMemcpyAsync(rg32, in.row_gate, 4 * n, hipMemcpyHostToDevice, st), "copy row_gate");
  if (ngc) BT(hipMemcpyAsync(c->d_gconsts.p, in.row_constants, 8 * nconst, hipMemcpyHostToDevice, st), "copy gate constants");
  if (E) BT(hipMemcpyAsync(copies, in.copies, 16 * E, hipMemcpyHostToDevice, st), "copy the copy pairs");
  BT(hipMemsetAsync(words, 0xFF, 24, st), "scratch");
  BT(hipMemsetAsync(words + 3, 0, 16, st), "scratch");
  BT(hipMemsetAsync(words + 5, 0xFF, 16, st), "scratch");
  hipLaunchKernelGGL(build_validate_kernel, dim3(grid_for(std::max({n, nconst, E}))), dim3(TPB), 0, st, rg32, n, c->num_gates,
                     c->d_gconsts.p, nconst, copies, E, R, words);
  unsigned long long h[8];
  BT(hipMemcpyAsync(h, words, 24, hipMemcpyDeviceToHost, st), "read validation");
  BT(hipStreamSynchronize(st), "validation");
  tr.mark("build: upload + validation");
  // (the order and the words of p2gpu_build_blob's refusals)
  if (h[0] != UINT64_MAX) {
    set_err("row %zu holds gate index %u of %u", (size_t)h[0], in.row_gate[h[0]], c->num_gates);
    return P2GPU_E_ARG;
  }
  if (h[1] != UINT64_MAX) {
    set_err("gate constant (%u, %zu) is not canonical", (uint32_t)(h[1] / n), (size_t)(h[1] % n));
    return P2GPU_E_ARG;
  }
  if (h[2] != UINT64_MAX) {
    set_err("copy constraint %zu names a cell outside the routed wires", (size_t)h[2]);
    return P2GPU_E_ARG;
  }
  // ---- row -> gate, special rows ----
  hipLaunchKernelGGL(build_rows_kernel, dim3(grid_for(n)), dim3(TPB), 0, st, rg32, n, c->d_row_gate.p);
  hipLaunchKernelGGL(build_first_row_kernel, dim3(grid_for(n)), dim3(TPB), 0, st, c->d_row_gate.p, c->d_gates.p, n, (uint32_t)G_PUBLIC_INPUT,
                     0u, UNSET, rows);
  for (uint32_t s = 1; s < MAX_SPARSE_ROWS; s++)
    hipLaunchKernelGGL(build_first_row_kernel, dim3(grid_for(n)), dim3(TPB), 0, st, c->d_row_gate.p, c->d_gates.p, n, (uint32_t)G_POSEIDON, s,
                       s == 1 ? UNSET : s - 1, rows);
  static_assert(MAX_SPARSE_ROWS == 4, "words[5..6] hold four rows");
  // ---- sigma: identity, then the cycles of the touched cells ----
  hipLaunchKernelGGL(build_sigma_identity_kernel, dim3((uint32_t)((n + TPB - 1) / TPB), (R + 7) / 8), dim3(TPB), 0, st, c->d_kis.p, c->tw_fwd.p,
                     d, R, c->d_sigmas.p);
  size_t T = 0;
  if (E) {
    uint32_t *parent = S.alloc<uint32_t>(tot);
    const size_t list_cap = std::min(2 * E, tot);
    unsigned long long *list = S.alloc<unsigned long long>(list_cap);
    if (!parent || !list) return dev_fail("scratch (parents, touched cells)", hipErrorOutOfMemory);
    BT(hipMemsetAsync(parent, 0xFF, 4 * tot, st), "scratch");
    hipLaunchKernelGGL(classes::touch_kernel<CopyPairs>, dim3(grid_for(E)), dim3(TPB), 0, st, CopyPairs{copies, R}, E, parent, list, words + 3);
    BT(hipMemcpyAsync(h + 3, words + 3, 8, hipMemcpyDeviceToHost, st), "read touched count");
    BT(hipStreamSynchronize(st), "touch");
    T = (size_t)h[3];
    if (T > list_cap) { set_err("p2gpu_circuit_build: internal error (touched cells)"); return P2GPU_E_DEVICE; }
    tr.mark("build: touched cells");
    if (int rc = classes::settle(CopyPairs{copies, R}, E, list, T, parent, flags, st, "p2gpu_circuit_build")) return rc;
    tr.mark("build: copy classes");
    // cycles
    unsigned long long *sorted = S.alloc<unsigned long long>(T);
    if (!sorted) return dev_fail("scratch (sort)", hipErrorOutOfMemory);
    hipLaunchKernelGGL(build_sort_keys_kernel, dim3(grid_for(T)), dim3(TPB), 0, st, list, T, parent, key_bits);
    const auto sort = S.radix_sort_keys(list, sorted, T, 0u, 2 * key_bits, st);
    BT(sort.e, sort.step);
    if (trace_on()) {
      (void)hipStreamSynchronize(st);
      tr.mark("build: sort by (root, key)");
    }
    hipLaunchKernelGGL(build_sigma_cycles_kernel, dim3(grid_for(T)), dim3(TPB), 0, st, sorted, T, key_bits, R, d, c->d_kis.p, c->tw_fwd.p,
                       c->d_sigmas.p);
  }
  BT(hipMemcpyAsync(h + 5, words + 5, 16, hipMemcpyDeviceToHost, st), "read special rows");
  BT(hipStreamSynchronize(st), "sigma fill");
  BT(hipGetLastError(), "kernel launch");
#undef BT
  S.release();
  // the special rows of the column classification: the PublicInputGate row first, then the PoseidonGate rows
  uint32_t hr[MAX_SPARSE_ROWS];
  memcpy(hr, h + 5, sizeof hr);
  c->sparse_rows = SparseRows();
  c->sparse_row = hr[0];
  if (c->sparse_row != UINT32_MAX) {
    c->sparse_rows.row[c->sparse_rows.count++] = c->sparse_row;
    for (uint32_t s = 1; s < MAX_SPARSE_ROWS && hr[s] != UINT32_MAX; s++) c->sparse_rows.row[c->sparse_rows.count++] = hr[s];
  }
  tr.mark("build: sigma fill, rows");
  return P2GPU_OK;
}

}  // namespace p2
