// check.hip -- why a witness is wrong (p2gpu_check_witness, p2gpu_check_witness_dev; include/p2gpu.h states the semantics): the
// gate constraints of the n base rows, the copy constraints of the routed cells and the canonicity of every word, per witness
// of a batch, keeping WHERE they fail.
//   check_canon_kernel     one lane per word: a word >= p is counted, the smallest key col << d | row kept (atomicMin)
//   check_gates_kernel<P>  one lane per (row, witness), the row on x -- column reads are coalesced --, the witness on blockIdx.y.
//                          The lane evaluates the row's OWN gate (gates.hpp eval_gate, dispatched on the row's kind: rows of one
//                          kind lie in runs, a wave diverges only where two runs meet) into a consumer that keeps the first
//                          non-zero constraint's index and value.  P = false skips PoseidonGate rows and P = true takes only
//                          those, in a launch of its own as plonk.hip's poseidon_gate_kernel: the 12-word state and the three
//                          fused linear layers would otherwise set the register allocation of every other gate.
//   check_copies_kernel    one lane per (routed cell, witness) against the partner cells genplan.hip's sigma_partners decoded once
//                          per call: the same decode the witness plan takes its copy classes from
// Per witness the kernels leave six words (DevReport): three counts (atomicAdd) and three firsts (64-bit atomicMin on
// row << 16 | constraint, and on the cell key); the value behind the first gate finding is read from the per-row values the
// failing lanes wrote.  A word >= p is used reduced once (v - p), so that gl.hpp's arithmetic never sees it.
#include "devclasses.hpp"
#include "genplan.hpp"

using namespace p2;

namespace {

using classes::TPB;
using classes::grid_for;
constexpr uint32_t UNSET = PLAN_UNSET;
constexpr uint32_t NO_CONSTRAINT = 0xFFFFu;
static_assert(MAX_GATE_CONSTRAINTS < NO_CONSTRAINT, "a constraint index fits the 16 bits under the row");

// the words of one witness on the device; the firsts start as UINT64_MAX
struct DevReport {
  unsigned long long gate_rows, copy_cells, noncanonical, first_gate, first_copy, first_noncanonical;
};

const char *gate_kind_name(uint32_t kind) {
  static const char *const names[G_KIND_COUNT] = {"NoopGate", "ConstantGate", "PublicInputGate", "ArithmeticGate", "BaseSumGate", "RandomAccessGate",
                                                  "PoseidonGate", "U32ArithmeticGate", "U32AddManyGate", "U32SubtractionGate", "U32RangeCheckGate",
                                                  "ComparisonGate"};
  return kind < G_KIND_COUNT ? names[kind] : "unknown gate";
}

// the first non-zero constraint: index and canonical value.  Constraints arrive as any congruent word (BaseOps::mul_out)
struct FirstNonZero {
  uint32_t t = 0, first = NO_CONSTRAINT;
  gl_t value = 0;
  __device__ __forceinline__ void emit(gl_t c) {
    c = gl_canon(c);
    const bool hit = c != 0 && first == NO_CONSTRAINT;
    first = hit ? t : first;
    value = hit ? c : value;
    t++;
  }
};

__global__ __launch_bounds__(256) void check_canon_kernel(const gl_t *wires, size_t matrix, uint32_t d, DevReport *rep) {
  const gl_t *w = wires + (size_t)blockIdx.y * matrix;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < matrix; x += step)
    if (w[x] >= GL_P) {
      atomicAdd(&rep[blockIdx.y].noncanonical, 1ull);
      atomicMin(&rep[blockIdx.y].first_noncanonical, (unsigned long long)x);  // (x = col * n + row is the key)
    }
}

struct GateArgs {
  const gl_t *wires;        // [batch][W][n]
  const uint8_t *row_gate;  // [n]
  const GateDesc *gates;
  const gl_t *gconsts;      // [ngc][n]
  const gl_t *pih;          // [batch][4]
  const gl_t *prc;          // the 360 round constants, poseidon_device_constants form
  DevReport *rep;           // [batch]
  uint16_t *row_status;     // [batch][n] or null
  gl_t *row_value;          // [batch][n]: written by failing rows only
  uint32_t d, W;
};

template <bool POSEIDON>
__global__ __launch_bounds__(256) void check_gates_kernel(const GateArgs a) {
  const size_t n = (size_t)1 << a.d;
  const size_t row = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const uint32_t b = blockIdx.y;
  if (row >= n) return;
  const GateDesc g = a.gates[a.row_gate[row]];
  if ((g.kind == G_POSEIDON) != POSEIDON) return;
  const gl_t *w = a.wires + (size_t)b * a.W * n + row;
  const gl_t *gc = a.gconsts + row;
  auto Wf = [&](uint32_t c) { return gl_canon(w[(size_t)c * n]); };
  auto LC = [&](uint32_t i) { return gc[(size_t)i * n]; };
  gl_t pih[4];
  for (int i = 0; i < 4; i++) pih[i] = a.pih[4 * b + i];
  FirstNonZero out;
  if constexpr (POSEIDON) eval_poseidon_gate<BaseOps>(Wf, a.prc, out);
  else eval_gate<BaseOps, false>(g, Wf, LC, pih, a.prc, out);
  if (a.row_status) a.row_status[(size_t)b * n + row] = (uint16_t)out.first;
  if (out.first != NO_CONSTRAINT) {
    a.row_value[(size_t)b * n + row] = out.value;
    atomicAdd(&a.rep[b].gate_rows, 1ull);
    atomicMin(&a.rep[b].first_gate, (unsigned long long)row << 16 | out.first);
  }
}

// cells: R * n routed cells, key = index; flags [batch][cells] or null
__global__ __launch_bounds__(256) void check_copies_kernel(const gl_t *wires, size_t matrix, const uint32_t *partner, size_t cells, DevReport *rep,
                                                           uint8_t *flags) {
  const uint32_t b = blockIdx.y;
  const gl_t *w = wires + (size_t)b * matrix;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  for (size_t x = (size_t)blockIdx.x * blockDim.x + threadIdx.x; x < cells; x += step) {
    const uint32_t y = partner[x];
    const bool differ = y != UNSET && gl_canon(w[x]) != gl_canon(w[y]);
    if (flags) flags[(size_t)b * cells + x] = differ ? 1 : 0;
    if (differ) {
      atomicAdd(&rep[b].copy_cells, 1ull);
      atomicMin(&rep[b].first_copy, (unsigned long long)x);
    }
  }
}

int device_fail(const char *what, hipError_t e) {
  (void)hipGetLastError();
  set_err("p2gpu_check_witness: %s: %s", what, hipGetErrorString(e));
  return P2GPU_E_DEVICE;
}
#define CHECK_TRY(expr, what)                                   \
  do {                                                          \
    const hipError_t e_ = (expr);                               \
    if (e_ != hipSuccess) return device_fail(what, e_);         \
  } while (0)

}  // namespace

namespace p2 {

int check_witness_impl(p2gpu_circuit *c, const gl_t *wires, size_t batch, const uint64_t *pis, uint32_t n_pi, p2gpu_witness_report *reports,
                       uint16_t *row_status, uint8_t *cell_flags) {
  const uint32_t d = c->d, R = c->R, W = c->W;
  const size_t n = c->n, cells = (size_t)R * n, matrix = (size_t)W * n, B = batch;
  CHECK_TRY(hipSetDevice(c->device), "select the device");
  ProfGuard prof(c);
  hipStream_t st = c->stream;
  classes::Scratch S;
  // ---- host side: the public-inputs hash of every witness, the counters' start ----
  std::vector<gl_t> pih(4 * B);
  for (size_t b = 0; b < B; b++) poseidon_hash_no_pad_host(pis + b * n_pi, n_pi, pih.data() + 4 * b, c->poseidon_rc);
  std::vector<DevReport> rep(B, DevReport{0, 0, 0, UINT64_MAX, UINT64_MAX, UINT64_MAX});
  unsigned long long bad_sigma = UINT64_MAX;
  bool has_poseidon = false, has_other = false;
  for (const GateDesc &g : c->gates) (g.kind == G_POSEIDON ? has_poseidon : has_other) = true;

  DevReport *d_rep = S.alloc<DevReport>(B);
  gl_t *d_pih = S.alloc<gl_t>(4 * B), *d_prc = S.alloc<gl_t>(360), *d_row_value = S.alloc<gl_t>(B * n);
  uint32_t *partner = S.alloc<uint32_t>(cells);
  unsigned long long *d_bad = S.alloc<unsigned long long>(1);
  uint16_t *d_status = row_status ? S.alloc<uint16_t>(B * n) : nullptr;
  uint8_t *d_flags = cell_flags ? S.alloc<uint8_t>(B * cells) : nullptr;
  if (!d_rep || !d_pih || !d_prc || !d_row_value || !partner || !d_bad || (row_status && !d_status) || (cell_flags && !d_flags))
    return device_fail("scratch", hipErrorOutOfMemory);
  CHECK_TRY(hipMemcpyAsync(d_rep, rep.data(), sizeof(DevReport) * B, hipMemcpyHostToDevice, st), "copy the counters");
  CHECK_TRY(hipMemcpyAsync(d_pih, pih.data(), 32 * B, hipMemcpyHostToDevice, st), "copy the public-inputs hashes");
  CHECK_TRY(hipMemcpyAsync(d_prc, c->poseidon_rc_gate, sizeof c->poseidon_rc_gate, hipMemcpyHostToDevice, st), "copy the round constants");
  CHECK_TRY(hipMemcpyAsync(d_bad, &bad_sigma, 8, hipMemcpyHostToDevice, st), "copy the counters");

  // ---- canonicity, gates ----
  {
    ProfScope ps("check_canon_kernel", 8.0 * (double)matrix * B);
    hipLaunchKernelGGL(check_canon_kernel, dim3(std::min<uint32_t>(grid_for(matrix), 2048), (uint32_t)B), dim3(TPB), 0, st, wires, matrix, d, d_rep);
  }
  GateArgs a;
  a.wires = wires; a.row_gate = c->d_row_gate.p; a.gates = c->d_gates.p; a.gconsts = c->d_gconsts.p; a.pih = d_pih; a.prc = d_prc;
  a.rep = d_rep; a.row_status = d_status; a.row_value = d_row_value; a.d = d; a.W = W;
  const dim3 rows_grid((uint32_t)((n + 255) / 256), (uint32_t)B);
  if (has_other) {
    ProfScope ps("check_gates_kernel", 8.0 * (double)c->gate_wires * n * B);
    hipLaunchKernelGGL(check_gates_kernel<false>, rows_grid, dim3(256), 0, st, a);
  }
  if (has_poseidon) {
    ProfScope ps("check_poseidon_kernel", 1.0 * (double)n * B);  // (what every lane reads: its row's gate; the PoseidonGate rows are few)
    hipLaunchKernelGGL(check_gates_kernel<true>, rows_grid, dim3(256), 0, st, a);
  }
  // ---- copies: sigma -> partner cells once, then every witness against them ----
  const char *step = "decode sigma";
  {
    ProfScope ps("check_sigma_decode", 12.0 * (double)cells);  // (the sorted powers of w, then a binary search per cell that moves)
    CHECK_TRY(sigma_partners(c, S, partner, d_bad, &step), step);
  }
  {
    ProfScope ps("check_copies_kernel", (4.0 + 16.0 * B) * (double)cells);
    hipLaunchKernelGGL(check_copies_kernel, dim3(std::min<uint32_t>(grid_for(cells), 2048), (uint32_t)B), dim3(TPB), 0, st, wires, matrix, partner,
                       cells, d_rep, d_flags);
  }
  CHECK_TRY(hipGetLastError(), "launch");
  CHECK_TRY(hipMemcpyAsync(rep.data(), d_rep, sizeof(DevReport) * B, hipMemcpyDeviceToHost, st), "read the counters");
  CHECK_TRY(hipMemcpyAsync(&bad_sigma, d_bad, 8, hipMemcpyDeviceToHost, st), "read the counters");
  if (row_status) CHECK_TRY(hipMemcpyAsync(row_status, d_status, 2 * B * n, hipMemcpyDeviceToHost, st), "read the row status");
  if (cell_flags) CHECK_TRY(hipMemcpyAsync(cell_flags, d_flags, B * cells, hipMemcpyDeviceToHost, st), "read the cell flags");
  CHECK_TRY(hipStreamSynchronize(st), "check");
  if (bad_sigma != UINT64_MAX) {
    set_err("p2gpu_check_witness: the sigma value of cell (row %llu, column %llu) names no routed cell", bad_sigma & (n - 1), bad_sigma >> d);
    return P2GPU_E_ARG;
  }

  // ---- the reports; the words behind a first finding are read one by one (a failing witness is the rare case) ----
  auto word = [&](const void *dev, void *host, size_t bytes) { return hipMemcpy(host, dev, bytes, hipMemcpyDeviceToHost); };
  int rc = P2GPU_OK;
  for (size_t b = B; b-- > 0;) {  // downwards: p2gpu_last_error keeps the lowest failing witness
    const DevReport &r = rep[b];
    p2gpu_witness_report &o = reports[b];
    memset(&o, 0, sizeof o);
    o.gate_rows_failed = r.gate_rows; o.copy_cells_failed = r.copy_cells; o.noncanonical_cells = r.noncanonical;
    o.gate_row = o.gate_index = o.gate_kind = o.constraint = UINT32_MAX;
    o.copy_cell[0] = o.copy_cell[1] = o.copy_partner[0] = o.copy_partner[1] = o.noncanonical_cell[0] = o.noncanonical_cell[1] = UINT32_MAX;
    const gl_t *w = wires + b * matrix;
    char who[48] = "", text[200] = "";
    if (B > 1) snprintf(who, sizeof who, "witness %zu of the batch: ", b);
    gl_t nc_word = 0;
    if (r.noncanonical) {
      const size_t x = (size_t)r.first_noncanonical;
      if (x >= matrix) { set_err("p2gpu_check_witness: internal error (cell key)"); return P2GPU_E_DEVICE; }
      o.noncanonical_cell[0] = (uint32_t)(x & (n - 1)); o.noncanonical_cell[1] = (uint32_t)(x >> d);
      CHECK_TRY(word(w + x, &nc_word, 8), "read a cell");
      snprintf(text, sizeof text, "cell (%u, %u) = 0x%016llx is not a canonical field element", o.noncanonical_cell[0], o.noncanonical_cell[1],
               (unsigned long long)nc_word);
    }
    if (r.copy_cells) {
      const size_t x = (size_t)r.first_copy;
      uint32_t y = UNSET;
      if (x < cells) CHECK_TRY(word(partner + x, &y, 4), "read a partner cell");
      if (x >= cells || y >= cells) { set_err("p2gpu_check_witness: internal error (cell key)"); return P2GPU_E_DEVICE; }
      o.copy_cell[0] = (uint32_t)(x & (n - 1)); o.copy_cell[1] = (uint32_t)(x >> d);
      o.copy_partner[0] = y & (uint32_t)(n - 1); o.copy_partner[1] = y >> d;
      CHECK_TRY(word(w + x, &o.copy_values[0], 8), "read a cell");
      CHECK_TRY(word(w + y, &o.copy_values[1], 8), "read a cell");
      snprintf(text, sizeof text, "copy (%u, %u) = 0x%016llx != (%u, %u) = 0x%016llx", o.copy_cell[0], o.copy_cell[1],
               (unsigned long long)o.copy_values[0], o.copy_partner[0], o.copy_partner[1], (unsigned long long)o.copy_values[1]);
    }
    if (r.gate_rows) {
      const size_t row = (size_t)(r.first_gate >> 16);
      uint8_t gi = 0;
      if (row >= n) { set_err("p2gpu_check_witness: internal error (row)"); return P2GPU_E_DEVICE; }
      CHECK_TRY(word(c->d_row_gate.p + row, &gi, 1), "read a row's gate");
      CHECK_TRY(word(d_row_value + b * n + row, &o.constraint_value, 8), "read a constraint");
      if (gi >= c->gates.size()) { set_err("p2gpu_check_witness: internal error (gate index)"); return P2GPU_E_DEVICE; }
      o.gate_row = (uint32_t)row; o.gate_index = gi; o.gate_kind = c->gates[gi].kind; o.constraint = (uint32_t)(r.first_gate & 0xFFFF);
      snprintf(text, sizeof text, "row %u (%s, gate %u): constraint %u = 0x%016llx", o.gate_row, gate_kind_name(o.gate_kind), o.gate_index,
               o.constraint, (unsigned long long)o.constraint_value);
    }
    if (text[0]) {
      set_err("%s%s", who, text);
      rc = P2GPU_E_UNSATISFIED;
    }
  }
  return rc;
}

}  // namespace p2

// the refusals that need no device (P2GPU_E_ARG), shared by the two entry points; 0: the call may go on
static int check_args(p2gpu_circuit *c, const void *wires, size_t batch, const uint64_t *pis, uint32_t n_pi, const void *reports) {
  if (!c || !wires || !reports || batch == 0 || batch > 65535) return P2GPU_E_ARG;  // (the witness is the grid's y)
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty()) {
    set_err("p2gpu_check_witness: a device group holds no witness of its own: check on a plain handle (p2gpu_circuit_create_on)");
    return P2GPU_E_ARG;
  }
  if (n_pi != c->num_pi) return check_public_inputs(c, pis, n_pi);
  for (size_t b = 0; b < batch; b++)
    if (int rc = check_public_inputs(c, pis ? pis + b * n_pi : nullptr, n_pi)) return rc;
  if (c->d < 1 || (size_t)c->R * c->n >= PLAN_UNSET) {
    set_err("p2gpu_check_witness: the routed cells do not fit a 32-bit key");
    return P2GPU_E_ARG;
  }
  return 0;
}

extern "C" {

int p2gpu_check_witness_dev(p2gpu_circuit *c, const uint64_t *wires_dev, size_t batch, const uint64_t *pis, uint32_t n_pi,
                            p2gpu_witness_report *reports, uint16_t *row_status, uint8_t *cell_flags) try {
  if (int rc = check_args(c, wires_dev, batch, pis, n_pi, reports)) return rc;
  return check_witness_impl(c, wires_dev, batch, pis, n_pi, reports, row_status, cell_flags);
} P2GPU_CATCH

int p2gpu_check_witness(p2gpu_circuit *c, const uint64_t *wires, const uint64_t *pis, uint32_t n_pi, p2gpu_witness_report *report,
                        uint16_t *row_status, uint8_t *cell_flags) try {
  if (int rc = check_args(c, wires, 1, pis, n_pi, report)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(c->wires_vals.p, wires, 8 * (size_t)c->W * c->n, hipMemcpyHostToDevice, c->stream));
  return check_witness_impl(c, c->wires_vals.p, 1, pis, n_pi, report, row_status, cell_flags);
} P2GPU_CATCH

}  // extern "C"
