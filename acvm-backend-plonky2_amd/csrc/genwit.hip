// genwit.hip -- the witness from the solver's values, on the device (SURVEY 8(f) "P2": `generate_partial_witness`,
// iop/generator.rs -- every generator in dependency order, every copy constraint propagated).
//
// The plan (once per circuit and seed set) is witplan.hip's: classes, slots, ops and levels as planhost.hpp states them.
// Proof (p2gpu_generate_witness): one persistent workgroup walks the levels with a barrier in between (the SHA-256
// compression circuit: 6 170 levels of median width 38 -- a chain, not a wave front), a wide kernel scatters the slot
// values over the routed cells, fill_witness derives the rest.  The first contradiction, by op order, comes back in
// one word after everything is queued.
// Batch (p2gpu_generate_witness_batch): B witnesses of one plan through the SAME kernels.  Only the values are per
// witness -- val[slot][B], seed_vals[seed][B], err[B], the witness index innermost -- and a lane of the walk takes the pair
// (op, witness) with the witness as the fast index: neighbouring lanes run one generator on neighbouring words.  Groups of
// WALK_GROUP witnesses get a workgroup each; a group shares nothing it writes with another, so nothing synchronises across
// workgroups.  The lone call is the batch of one: one routine, one set of buffers (witplan.hpp).
#include "generators.hpp"
#include "witplan.hpp"

using namespace p2;

namespace {

constexpr uint32_t UNSET = PLAN_UNSET, WRITER = PLAN_WRITER;
constexpr uint32_t WALK_TPB = 512;
// witnesses per workgroup of the walk; a power of two.  8 is the starting value (41 ops of the median SHA level x 8 = 328 of 512
// lanes), NOT yet a measured choice: profiles/device_witness.md says how 4 / 8 / 16 are to be compared
constexpr uint32_t WALK_GROUP = 8;

struct WalkArgs {
  const OpRec *ops;
  const uint32_t *level_off;  // [levels + 1]
  uint32_t levels;
  const uint32_t *cell_slot;  // [R][n]
  const uint32_t *gen_table;  // one word per cell a generator names: cell key | WRITER; generator g's begin at gen_off[g]
  const uint32_t *gen_off;    // [generators + 1]
  const uint32_t *gen_shape;  // [generators] la | lb << 8 | ld << 16 | lr << 24
  const uint32_t *seed_out;   // a bit per routed cell: a seed's cell that a row op of its row sets as well; null when there is none
  gl_t *val;                  // [slots][B]
  const uint2 *seed_cells;    // (row, col)
  const gl_t *seed_vals;      // [seeds][B]
  const uint8_t *row_gate;
  const GateDesc *gates;
  const gl_t *gconsts, *prc;
  unsigned long long *err;    // [B]: per witness, the smallest (op position << 8 | column, or a generator's cell position) that contradicts
  uint32_t d, R, ngc, B;
};

// the row as the level walk sees it: witness b's slot values behind the routed cells
struct RowSlots {
  const WalkArgs &a;
  size_t row;
  uint32_t pos;  // of the op in the schedule
  uint32_t b;    // witness of the batch
  bool seed = false;  // the op is a seed: the writer bit of a cell that a seed and a row op both set is the seed's
  __device__ __forceinline__ gl_t &slot(uint32_t s) const { return a.val[(size_t)s * a.B + b]; }
  // whether the writer bit of cell `key` is this op's: a row op's unless a seed names the very cell -- that seed wrote (or compared
  // with) the slot in an earlier level, so the row op compares
  __device__ __forceinline__ bool owns_bit(size_t key) const { return seed || !a.seed_out || !((a.seed_out[key >> 5] >> (key & 31)) & 1); }
  __device__ __forceinline__ gl_t get(uint32_t col) const {
    if (col >= a.R) return 0;
    const uint32_t s = a.cell_slot[((size_t)col << a.d) + row];
    return s == UNSET ? (gl_t)0 : slot(s & ~WRITER);
  }
  __device__ __forceinline__ void set(uint32_t col, gl_t v) {
    if (col >= a.R) return;  // gate-internal column: fill_witness derives it
    const size_t key = ((size_t)col << a.d) + row;
    const uint32_t s = a.cell_slot[key];
    if (s == UNSET) return;
    if ((s & WRITER) && owns_bit(key)) slot(s & ~WRITER) = v;
    else if (slot(s & ~WRITER) != v) reject(col);
  }
  __device__ __forceinline__ gl_t lc(uint32_t i) const { return i < a.ngc ? a.gconsts[((size_t)i << a.d) + row] : (gl_t)0; }
  __device__ __forceinline__ void reject(uint32_t col) { atomicMin(a.err + b, ((unsigned long long)pos << 8) | col); }
};

// a generator that is no gate's own as the level walk sees it: witness b's slot values behind its cells, numbered 0 .. cells - 1
// as the plan's table names them from the generator's offset on (every one has a slot); the writer bits are the table words',
// not cell_slot's
struct GenSlots {
  const WalkArgs &a;
  const uint32_t *words;  // the generator's words of the table
  uint32_t pos;           // of the op in the schedule
  uint32_t b;             // witness of the batch
  __device__ __forceinline__ gl_t &slot(uint32_t s) const { return a.val[(size_t)s * a.B + b]; }
  __device__ __forceinline__ uint32_t slot_of(uint32_t i) const { return a.cell_slot[words[i] & ~WRITER] & ~WRITER; }
  __device__ __forceinline__ gl_t get(uint32_t i) const { return slot(slot_of(i)); }
  __device__ __forceinline__ void set(uint32_t i, gl_t v) {
    if (words[i] & WRITER) slot(slot_of(i)) = v;
    else if (slot(slot_of(i)) != v) reject(i);
  }
  __device__ __forceinline__ void reject(uint32_t i) { atomicMin(a.err + b, ((unsigned long long)pos << 8) | i); }
};

// The div-rem generator, called and not inlined: its word arrays (bigdiv.hpp, 53 words and the loop state) are private memory
// of THIS frame.  A call in the kernel still costs every other arm (the SHA-256 walk 15.5 -> 23.8 ms: profiles/
// device_witness.md), so the big-integer arms exist only in the walk kernel's BIGINT = true form, which runs the plans that list such a
// generator (or a nonnative one or the GLV decomposition, below); every other plan runs the form without them.  Lanes of one op run it with different trip counts.
static_assert(BIGDIV_MAX_A == PLAN_DIVREM_MAX_A && BIGDIV_MAX_B == PLAN_DIVREM_MAX_B, "the plan admits the shapes the division's arrays hold");
__device__ __noinline__ void run_biguint_divrem(const WalkArgs &a, uint32_t g, uint32_t pos, uint32_t b) {
  const uint32_t sw = a.gen_shape[g];
  const uint32_t shape[4] = {sw & 0xFF, (sw >> 8) & 0xFF, (sw >> 16) & 0xFF, sw >> 24};
  GenSlots w{a, a.gen_table + a.gen_off[g], pos, b};
  gen_biguint_divrem(w, shape);
}

// The four nonnative generators behind one call, for the same reason: NonNative's arrays (nonnative.hpp: BigDiv, the modulus, the
// operands, the four numbers of the inversion) are this frame's.  field: the op record's, < NN_FIELDS as the plan checked it.
static_assert(NN_LIMBS == PLAN_NONNATIVE_LIMBS && NN_MAX_OPERAND == PLAN_NONNATIVE_MAX && NN_FIELDS == PLAN_NONNATIVE_FIELDS, "the plan admits the shapes and fields the arithmetic holds");
__device__ __noinline__ void run_nonnative(const WalkArgs &a, uint32_t code, uint32_t field, uint32_t g, uint32_t pos, uint32_t b) {
  const uint32_t sw = a.gen_shape[g];
  const uint32_t shape[4] = {sw & 0xFF, (sw >> 8) & 0xFF, (sw >> 16) & 0xFF, sw >> 24};
  GenSlots w{a, a.gen_table + a.gen_off[g], pos, b};
  switch (code) {
  case OP_NONNATIVE_ADD: gen_nonnative_add(w, shape, field); break;
  case OP_NONNATIVE_SUB: gen_nonnative_sub(w, shape, field); break;
  case OP_NONNATIVE_MUL: gen_nonnative_mul(w, shape, field); break;
  default: gen_nonnative_inv(w, shape, field); break;
  }
}

// The GLV decomposition generator behind a call of its own, for the same reason (glv.hpp: NonNative and four more numbers).
static_assert(GLV_LIMBS == PLAN_GLV_LIMBS, "the plan admits the shape the decomposition writes");
__device__ __noinline__ void run_glv_decompose(const WalkArgs &a, uint32_t g, uint32_t pos, uint32_t b) {
  const uint32_t sw = a.gen_shape[g];
  const uint32_t shape[4] = {sw & 0xFF, (sw >> 8) & 0xFF, (sw >> 16) & 0xFF, sw >> 24};
  GenSlots w{a, a.gen_table + a.gen_off[g], pos, b};
  gen_glv_decompose(w, shape);
}

template <bool BIGINT>
__device__ __forceinline__ void run_op(const WalkArgs &a, uint32_t pos, uint32_t b) {
  const OpRec op = a.ops[pos];
  const uint32_t code = op.y & 0xFF, sub = op.y >> 8;
  if (code == OP_SEED) {
    const uint2 cell = a.seed_cells[op.x];
    const gl_t v = a.seed_vals[(size_t)op.x * a.B + b];
    RowSlots w{a, cell.x, pos, b, true};
    if (v >= GL_P) w.reject(cell.y);
    else w.set(cell.y, v);
    return;
  }
  if (code == OP_EQUALITY) {
    GenSlots w{a, a.gen_table + a.gen_off[op.x], pos, b};
    gen_equality(w);
    return;
  }
  if (BIGINT && op_is_bigint_generator(code)) {  // (a plan with such an op runs the BIGINT form: walk_and_scatter)
    if (code == OP_BIGUINT_DIVREM) run_biguint_divrem(a, op.x, pos, b);
    else if (code == OP_GLV_DECOMPOSE) run_glv_decompose(a, op.x, pos, b);
    else run_nonnative(a, code, sub, op.x, pos, b);
    return;
  }
  RowSlots w{a, op.x, pos, b};
  const GateDesc g = a.gates[a.row_gate[op.x]];
  switch (code) {
  case OP_CONSTANT: gen_constant(w, g); break;
  case OP_ARITHMETIC: gen_arithmetic_op(w, sub, w.lc(0), w.lc(1)); break;
  case OP_BASE_SPLIT: gen_base_sum_split(w, g); break;
  case OP_BASE_JOIN: gen_base_sum_join(w, g); break;
  case OP_RA_COPY: gen_random_access_copy(w, g, sub); break;
  case OP_RA_CONSTS: gen_random_access_consts(w, g); break;
  case OP_POSEIDON: gen_poseidon(w, a.prc); break;
  case OP_U32_ARITHMETIC: gen_u32_arithmetic_op(w, g, sub); break;
  case OP_U32_ADD_MANY: gen_u32_add_many_op(w, g, sub); break;
  case OP_U32_SUBTRACTION: gen_u32_subtraction_op(w, g, sub); break;
  case OP_U32_RANGE_CHECK: gen_u32_range_check(w, g); break;
  case OP_COMPARISON: gen_comparison(w, g); break;
  default: break;
  }
}

// ONE workgroup per group of WALK_GROUP witnesses (the last group may hold fewer): the waves of a workgroup share their CU's
// vector cache, so what a level stored is what the next level loads after the barrier, and a group reads and writes its own
// witnesses' words only; the rest of the device stays free for the proofs in flight.  With 1 << sh the group's width rounded
// up to a power of two, lane t takes witness t & mask of the group and the level's ops t >> sh, + 512 >> sh, ... (the lone
// call: sh = 0, a lane per op).
template <bool BIGINT>
__global__ __launch_bounds__(WALK_TPB) void genwit_walk_kernel(WalkArgs a) {
  const uint32_t b0 = blockIdx.x * WALK_GROUP, gw = min(WALK_GROUP, a.B - b0);
  const uint32_t sh = gw > 1 ? 32 - __clz(gw - 1) : 0, lb = threadIdx.x & ((1u << sh) - 1);
  const uint32_t first = threadIdx.x >> sh, step = WALK_TPB >> sh;
  for (uint32_t l = 0; l < a.levels; l++) {
    const uint32_t end = a.level_off[l + 1];
    if (lb < gw)
      for (uint32_t pos = a.level_off[l] + first; pos < end; pos += step) run_op<BIGINT>(a, pos, b0 + lb);
    __syncthreads();
  }
}

// wires[b][col][row] = witness b's value of the slot, zero for a cell without one and for the gate-internal columns
// (cells <= i < matrix); cell_slot is read once for the whole batch.  A lane keeps its cell and loops over b: the stores of a
// wave are 64 consecutive words of one matrix, and a lane's loads are the B consecutive words of its slot (whole cache lines
// from B = 16 on) -- a lane per (cell, b) would coalesce the loads and scatter every store over B matrices instead.
__global__ __launch_bounds__(256) void genwit_scatter_kernel(const uint32_t *cell_slot, const gl_t *val, size_t cells, size_t matrix,
                                                             uint32_t B, gl_t *wires) {
  const size_t step = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < matrix; i += step) {
    const uint32_t s = i < cells ? cell_slot[i] : UNSET;
    const gl_t *v = s == UNSET ? nullptr : val + (size_t)(s & ~WRITER) * B;
    for (uint32_t b = 0; b < B; b++) wires[b * matrix + i] = v ? v[b] : (gl_t)0;
  }
}

// the seeds no slot carries: pi_rows = 0: those on gate-internal columns; 1: those in PublicInputGate rows, whose wires are
// the caller's whatever ran in between.  A lane per (seed, witness), the witness the fast index as in vals.
__global__ void genwit_seed_write_kernel(const uint2 *cells, const gl_t *vals, uint32_t count, uint32_t B, uint32_t R, uint32_t d,
                                         int pi_rows, const uint8_t *row_gate, const GateDesc *gates, size_t matrix, gl_t *wires) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)count * B) return;
  const uint2 c = cells[k / B];
  if (pi_rows ? gates[row_gate[c.x]].kind == G_PUBLIC_INPUT : c.y >= R) wires[(k % B) * matrix + ((size_t)c.y << d) + c.x] = vals[k];
}

// everything of B witnesses on the handle's stream: p->pin holds the seed values [n_seeds][B] on entry and, from
// p->pin + n_seeds * B on, the B contradiction words when this returns.  wires: [B][num_wires][n]
int walk_and_scatter(p2gpu_witness_plan *p, uint32_t B, gl_t *wires) {
  p2gpu_circuit *c = p->c;
  hipStream_t st = c->stream;
  const uint32_t ngc = c->NC - c->num_selectors;
  const size_t n_vals = (size_t)p->n_seeds * B;
  if (n_vals) HIP_TRY(hipMemcpyAsync(p->seed_vals.p, p->pin, 8 * n_vals, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(p->err.p, 0xFF, 8 * (size_t)B, st));
  WalkArgs a;
  a.ops = p->ops.p; a.level_off = p->level_off.p; a.levels = p->levels; a.cell_slot = p->cell_slot.p; a.gen_table = p->gen_table.p; a.gen_off = p->gen_off.p; a.gen_shape = p->gen_shape.p; a.val = p->val.p;
  a.seed_out = p->has_seed_out ? p->seed_out.p : nullptr;
  a.seed_cells = p->seed_cells.p; a.seed_vals = p->seed_vals.p; a.row_gate = c->d_row_gate.p; a.gates = c->d_gates.p;
  a.gconsts = c->d_gconsts.p; a.prc = c->d_prc.p; a.err = p->err.p; a.d = c->d; a.R = c->R; a.ngc = ngc; a.B = B;
  HIP_TRY(hipEventRecord(p->ev0, st));
  {
    ProfScope ps("genwit_walk_kernel", 16.0 * (double)p->n_ops * B);
    const dim3 grid((B + WALK_GROUP - 1) / WALK_GROUP);
    if (p->has_bigint) hipLaunchKernelGGL(genwit_walk_kernel<true>, grid, dim3(WALK_TPB), 0, st, a);
    else hipLaunchKernelGGL(genwit_walk_kernel<false>, grid, dim3(WALK_TPB), 0, st, a);
  }
  HIP_TRY(hipEventRecord(p->ev1, st));
  const size_t cells = (size_t)c->R * c->n, matrix = (size_t)c->W * c->n;
  {
    ProfScope ps("genwit_scatter_kernel", 4.0 * (double)cells + 8.0 * (double)(cells + matrix) * B);
    hipLaunchKernelGGL(genwit_scatter_kernel, dim3((unsigned)std::min<size_t>((matrix + 255) / 256, 1 << 16)), dim3(256), 0, st,
                       p->cell_slot.p, p->val.p, cells, matrix, B, wires);
  }
  const dim3 sg((unsigned)((n_vals + 255) / 256));
  if (n_vals)
    hipLaunchKernelGGL(genwit_seed_write_kernel, sg, dim3(256), 0, st, p->seed_cells.p, p->seed_vals.p, p->n_seeds, B, c->R, c->d, 0,
                       c->d_row_gate.p, c->d_gates.p, matrix, wires);
  for (uint32_t b = 0; b < B; b++)
    fill_witness(st, wires + b * matrix, c->d_row_gate.p, c->d_gates.p, c->d_gconsts.p, c->d_prc.p, c->d, ngc, c->W);
  if (n_vals)
    hipLaunchKernelGGL(genwit_seed_write_kernel, sg, dim3(256), 0, st, p->seed_cells.p, p->seed_vals.p, p->n_seeds, B, c->R, c->d, 1,
                       c->d_row_gate.p, c->d_gates.p, matrix, wires);
  HIP_TRY(hipMemcpyAsync(p->pin + n_vals, p->err.p, 8 * (size_t)B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  float ms = 0;
  if (hipEventElapsedTime(&ms, p->ev0, p->ev1) == hipSuccess) p->walk_ms = ms;
  return P2GPU_OK;
}

// a contradiction word as (row, col) and as p2gpu_last_error's text behind `who`; seed_values: that witness's, [n_seeds]
int name_contradiction(const p2gpu_witness_plan *p, uint64_t e, const uint64_t *seed_values, const char *who, uint32_t cell[2]) {
  const size_t pos = (size_t)(e >> 8);
  const uint32_t col = (uint32_t)(e & 0xFF);
  if (pos >= p->h_ops.size()) { set_err("p2gpu_generate_witness: internal error (contradiction word)"); return P2GPU_E_DEVICE; }
  const OpRec op = p->h_ops[pos];
  if (op_is_listed_generator(op.y & 0xFF)) {  // (the low byte is the generator's cell position, not a column)
    const std::vector<uint32_t> &off = p->h_gens.off;
    const size_t at = op.x < p->h_gens.size() ? (size_t)off[op.x] + col : SIZE_MAX;
    if (op.x >= p->h_gens.size() || at >= off[op.x + 1] || at >= p->h_gen_table.size()) { set_err("p2gpu_generate_witness: internal error (contradiction word)"); return P2GPU_E_DEVICE; }
    const uint32_t key = p->h_gen_table[at] & ~WRITER;
    cell[0] = key & (uint32_t)(p->c->n - 1);
    cell[1] = key >> p->c->d;
    set_err("%sunsatisfiable: generator %u: cell (row %u, column %u) already has another value", who, op.x, cell[0], cell[1]);
    return P2GPU_E_UNSATISFIED;
  }
  const bool seed = (op.y & 0xFF) == OP_SEED;
  cell[0] = seed ? p->h_seed_cells[op.x].row : op.x;
  cell[1] = col;
  if (seed)
    set_err("%sseed %u for cell (row %u, column %u) %s", who, op.x, cell[0], col,
            seed_values[op.x] >= GL_P ? "is not a canonical field element" : "contradicts the value its copy class already has");
  else
    set_err("%sunsatisfiable: the generator of row %u contradicts the value cell (row %u, column %u) already has", who, op.x, op.x, col);
  return P2GPU_E_UNSATISFIED;
}

// B witnesses: stage the seed values, walk, read the B words, name the contradictions.  seed_values: [batch][n_seeds];
// status: [batch]; bad_cells: [batch][2] or null.  A member of a batch is named in front of its message; the lone call
// (prefix = false) words it as it is.  Returns after the contradiction words have arrived.
int generate_batch(p2gpu_witness_plan *p, const uint64_t *seed_values, size_t batch, gl_t *wires, int *status, uint32_t *bad_cells, bool prefix) {
  HIP_TRY(hipSetDevice(p->c->device));
  if (int rc = plan_reserve(p, batch)) return rc;
  const uint32_t B = (uint32_t)batch, S = p->n_seeds;
  for (uint32_t b = 0; b < B; b++)
    for (uint32_t i = 0; i < S; i++) p->pin[(size_t)i * B + b] = seed_values[(size_t)b * S + i];
  if (int rc = walk_and_scatter(p, B, wires)) return rc;
  int rc = P2GPU_OK;
  for (uint32_t b = B; b-- > 0;) {  // downwards: p2gpu_last_error keeps the lowest failing witness
    const uint64_t e = p->pin[(size_t)S * B + b];
    uint32_t cell[2] = {UINT32_MAX, UINT32_MAX};
    status[b] = P2GPU_OK;
    if (e != UINT64_MAX) {
      char who[48] = "";
      if (prefix) snprintf(who, sizeof who, "witness %u of the batch: ", b);
      status[b] = name_contradiction(p, e, seed_values + (size_t)b * S, who, cell);
      if (status[b] != P2GPU_E_UNSATISFIED || rc == P2GPU_OK) rc = status[b];  // (an internal error, once seen, is what returns)
    }
    if (bad_cells) bad_cells[2 * b] = cell[0], bad_cells[2 * b + 1] = cell[1];
  }
  return rc;
}

// one witness: the batch of one
int generate(p2gpu_witness_plan *p, const uint64_t *seed_values, gl_t *wires) {
  int status;
  return generate_batch(p, seed_values, 1, wires, &status, nullptr, false);
}

}  // namespace

extern "C" {

int p2gpu_generate_witness(p2gpu_witness_plan *p, const uint64_t *seed_values, uint64_t *wires_dev_out) try {
  if (!p || !wires_dev_out || (p->n_seeds && !seed_values)) return P2GPU_E_ARG;
  ProfGuard pg(p->c);
  return generate(p, seed_values, wires_dev_out);
} P2GPU_CATCH

int p2gpu_generate_witness_batch(p2gpu_witness_plan *p, const uint64_t *seed_values, size_t batch, uint64_t *wires_dev_out, int *status,
                                 uint32_t *bad_cells) try {
  if (!p || !wires_dev_out || !status || batch == 0 || (p->n_seeds && !seed_values)) return P2GPU_E_ARG;
  if (batch >= ((size_t)1 << 32) / std::max<uint32_t>(1, p->n_seeds)) return P2GPU_E_ARG;  // (the seed-write kernel's grid)
  ProfGuard pg(p->c);
  return generate_batch(p, seed_values, batch, wires_dev_out, status, bad_cells, true);
} P2GPU_CATCH

int p2gpu_prove_seeds(p2gpu_witness_plan *p, const uint64_t *seed_values, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out,
                      size_t *proof_len, p2gpu_timings *tm) try {
  if (!p || !proof_out || !proof_len || (p->n_seeds && !seed_values)) return P2GPU_E_ARG;
  p2gpu_circuit *c = p->c;
  const double t0 = now_ms();
  {
    ProfGuard pg(c);
    if (int rc = generate(p, seed_values, c->wires_vals.p)) return rc;
  }
  // (h2d_ms: what stands in front of the resident proof -- here the witness generation)
  return prove_impl(c, c->wires_vals.p, pis, n_pi, proof_out, proof_len, tm, now_ms() - t0);
} P2GPU_CATCH

int p2gpu_check_seeds(p2gpu_witness_plan *p, const uint64_t *seed_values, const uint64_t *pis, uint32_t n_pi, p2gpu_witness_report *report,
                      uint16_t *row_status, uint8_t *cell_flags) try {
  if (!p || !report || (p->n_seeds && !seed_values)) return P2GPU_E_ARG;
  p2gpu_circuit *c = p->c;  // (a plan exists on a plain prover handle only)
  if (int rc = check_public_inputs(c, pis, n_pi)) return rc;
  {
    ProfGuard pg(c);
    if (int rc = generate(p, seed_values, c->wires_vals.p)) return rc;
  }
  return check_witness_impl(c, c->wires_vals.p, 1, pis, n_pi, report, row_status, cell_flags);
} P2GPU_CATCH

}  // extern "C"
