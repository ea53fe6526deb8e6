// witplan.hip -- the witness plan of a circuit and a seed set, made once (SURVEY 8(f) "P2"): the front checks and the ownership
// of a half-made plan, one of the two compilers, and the tail that attaches the compiled arrays to the handle.
//   p2gpu_witness_plan_create   the host compiler (planhost.hpp) over the circuit's tables as the device holds them -- a handle
//                               from a blob and one from p2gpu_circuit_build hold the same sigma, hence give the same plan;
//   p2gpu_witness_plan_build    the same plan compiled on the device (genplan.hip); the host one is its differential oracle.
//   ..._create_genv / _build_genv the same two routines with a list of generators that are no gate's own, each a kind, a shape
//                               and its cells in one flat list (planhost.hpp states the rules);
//   ..._create_gen / _build_gen their case of four-cell records, and the entry points above the case of an empty list.
// genwit.hip runs a plan.
#include <chrono>
#include <functional>
#include "devclasses.hpp"
#include "witplan.hpp"

using namespace p2;

namespace {

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

// The tail of both compilers: the plan's own buffers, filled from the three arrays and the generator table (an upload for the host compiler, a copy
// inside HBM and ONE read-back -- the op records name_contradiction needs -- for the device one).
int plan_finish(p2gpu_witness_plan *p, const PlanArrays &a) {
  p2gpu_circuit *c = p->c;
  const size_t n_seeds = p->n_seeds, tot = (size_t)c->R * c->n;
  p->levels = a.levels; p->slots = a.slots; p->n_ops = a.n_ops; p->widest = a.widest;
  HIP_TRY(p->ops.alloc(std::max<size_t>(1, a.n_ops)));
  HIP_TRY(p->level_off.alloc((size_t)a.levels + 1));
  HIP_TRY(p->cell_slot.alloc(tot));
  HIP_TRY(p->seed_cells.alloc(std::max<size_t>(1, n_seeds)));
  const size_t n_gens = p->h_gens.size();
  HIP_TRY(p->gen_table.alloc(std::max<size_t>(1, a.n_gen_cells)));
  HIP_TRY(p->gen_off.alloc(n_gens + 1));
  HIP_TRY(p->gen_shape.alloc(std::max<size_t>(1, n_gens)));
  p->h_gen_table.resize(a.n_gen_cells);
  std::vector<uint32_t> shapes(n_gens);
  for (size_t g = 0; g < n_gens; g++) {
    shapes[g] = p->h_gens.shape_word(g);
    p->has_bigint |= op_is_bigint_generator(p->h_gens.code(g));
  }
  HIP_TRY(hipMemcpyAsync(p->gen_off.p, p->h_gens.off.data(), 4 * (n_gens + 1), hipMemcpyHostToDevice, c->stream));
  if (n_gens) HIP_TRY(hipMemcpyAsync(p->gen_shape.p, shapes.data(), 4 * n_gens, hipMemcpyHostToDevice, c->stream));
  if (a.n_gen_cells) {
    HIP_TRY(hipMemcpyAsync(p->gen_table.p, a.gen_table, 4 * p->h_gen_table.size(), a.kind, c->stream));
    if (a.kind == hipMemcpyHostToDevice) memcpy(p->h_gen_table.data(), a.gen_table, 4 * p->h_gen_table.size());
    else HIP_TRY(hipMemcpyAsync(p->h_gen_table.data(), a.gen_table, 4 * p->h_gen_table.size(), hipMemcpyDeviceToHost, c->stream));
  }
  // the seeds on a row op's own output column (witplan.hpp seed_out): the registry's output columns of the seed's row
  {
    std::vector<uint8_t> row_gate(c->n);
    HIP_TRY(hipMemcpyAsync(row_gate.data(), c->d_row_gate.p, c->n, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::vector<uint32_t> bits;
    for (const PlanSeed &cell : p->h_seed_cells) {
      if (cell.col >= c->R || row_gate[cell.row] >= c->gates.size()) continue;
      const GateDesc &g = c->gates[row_gate[cell.row]];
      bool is_out = false;
      for (uint32_t k = 0, m = row_num_ops(g); k < m && !is_out; k++)
        for_cols(row_op(g, k, 1, 1).out, [&](uint32_t col) { is_out |= col == cell.col; });
      if (!is_out) continue;
      if (bits.empty()) bits.assign((tot + 31) / 32, 0);
      const size_t key = ((size_t)cell.col << c->d) + cell.row;
      bits[key >> 5] |= 1u << (key & 31);
    }
    p->has_seed_out = !bits.empty();
    if (p->has_seed_out) {
      HIP_TRY(p->seed_out.alloc(bits.size()));
      HIP_TRY(hipMemcpyAsync(p->seed_out.p, bits.data(), 4 * bits.size(), hipMemcpyHostToDevice, c->stream));
      HIP_TRY(hipStreamSynchronize(c->stream));  // (bits goes out of scope)
    }
  }
  if (int rc = plan_reserve(p, 1)) return rc;
  HIP_TRY(hipEventCreate(&p->ev0));
  HIP_TRY(hipEventCreate(&p->ev1));
  p->h_ops.resize(a.n_ops);
  if (a.n_ops) {
    HIP_TRY(hipMemcpyAsync(p->ops.p, a.ops, sizeof(OpRec) * a.n_ops, a.kind, c->stream));
    if (a.kind == hipMemcpyHostToDevice) memcpy(p->h_ops.data(), a.ops, sizeof(OpRec) * a.n_ops);
    else HIP_TRY(hipMemcpyAsync(p->h_ops.data(), a.ops, sizeof(OpRec) * a.n_ops, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(p->level_off.p, a.level_off, 4 * ((size_t)a.levels + 1), a.kind, c->stream));
  HIP_TRY(hipMemcpyAsync(p->cell_slot.p, a.cell_slot, 4 * tot, a.kind, c->stream));
  if (n_seeds) HIP_TRY(hipMemcpyAsync(p->seed_cells.p, p->h_seed_cells.data(), sizeof(uint2) * n_seeds, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(p->val.p, 0, 8 * (size_t)std::max<uint32_t>(1, a.slots), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (the arrays go out of scope)
  return P2GPU_OK;
}

// the host compiler: the circuit's three tables as the device holds them, read back
int plan_compile(p2gpu_witness_plan *p) {
  p2gpu_circuit *c = p->c;
  const uint32_t ngc = c->NC - c->num_selectors;
  const size_t n = c->n, tot = (size_t)c->R * n;
  std::vector<gl_t> sigma(tot), gconsts((size_t)ngc * n);
  std::vector<uint8_t> row_gate(n);
  HIP_TRY(hipMemcpyAsync(sigma.data(), c->d_sigmas.p, 8 * tot, hipMemcpyDeviceToHost, c->stream));
  if (ngc) HIP_TRY(hipMemcpyAsync(gconsts.data(), c->d_gconsts.p, 8 * gconsts.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(row_gate.data(), c->d_row_gate.p, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  const PlanInput in{c->d, c->R, c->W, ngc, sigma.data(), gconsts.data(), row_gate.data(), c->gates.data(), c->k_is.data()};
  HostPlan plan;
  if (PlanRefusal r = plan_compile_host(in, p->h_seed_cells, p->h_gens, plan)) return plan_refuse(c, r);
  PlanArrays a;
  a.cell_slot = plan.cell_slot.data(); a.ops = reinterpret_cast<const OpRec *>(plan.ops.data()); a.level_off = plan.level_off.data();
  a.levels = plan.levels; a.slots = plan.slots; a.widest = plan.widest; a.n_ops = plan.ops.size();
  a.gen_table = plan.gen_table.data(); a.n_gen_cells = plan.gen_table.size();
  return plan_finish(p, a);
}

// the device compiler (genplan.hip) in front of the same tail
int plan_build(p2gpu_witness_plan *p) {
  classes::Scratch S;
  PlanArrays a;
  if (int rc = plan_compile_device(p->c, p->h_seed_cells, p->h_gens, S, a)) return rc;
  return plan_finish(p, a);  // (S goes out of scope behind it: the plan holds what a host-compiled one holds)
}

// the front checks, the seed and generator checks and the ownership of a half-made plan, for either compiler
// check_generators(d, R, list): the caller's generator list of either record form through planhost.hpp's checks
using GeneratorCheck = std::function<PlanRefusal(uint32_t, uint32_t, PlanGenList &)>;
int plan_new(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, size_t n_generators, size_t n_generator_cells, const GeneratorCheck &check_generators,
             p2gpu_witness_plan **out, int (*compile)(p2gpu_witness_plan *)) {
  static_assert(sizeof(p2gpu_generator) == sizeof(PlanGenerator) && P2GPU_GEN_EQUALITY == PLAN_GEN_EQUALITY, "planhost.hpp restates the record");
  static_assert(sizeof(p2gpu_generator_v) == sizeof(PlanGeneratorV) && P2GPU_GEN_BIGUINT_DIVREM == PLAN_GEN_BIGUINT_DIVREM, "planhost.hpp restates the record");
  static_assert(P2GPU_GEN_NONNATIVE_ADD == PLAN_GEN_NONNATIVE_ADD && P2GPU_GEN_NONNATIVE_SUB == PLAN_GEN_NONNATIVE_SUB && P2GPU_GEN_NONNATIVE_MUL == PLAN_GEN_NONNATIVE_MUL &&
                    P2GPU_GEN_NONNATIVE_INV == PLAN_GEN_NONNATIVE_INV && P2GPU_FIELD_SECP256K1_BASE == 0 && P2GPU_FIELD_SECP256K1_SCALAR == 1 &&
                    P2GPU_GEN_GLV_DECOMPOSE == PLAN_GEN_GLV_DECOMPOSE,
                "planhost.hpp restates the kinds");
  if (out) *out = nullptr;
  if (!c || !out || (n_seeds && !seed_cells) || n_generators >= ((size_t)1 << 32) || n_generator_cells >= ((size_t)1 << 32)) return P2GPU_E_ARG;
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty()) {
    set_err("p2gpu_witness_plan_create: a device group takes a wire matrix (every rank of a sharded proof reads all of it)");
    return P2GPU_E_ARG;
  }
  if (c->R > 256 || n_seeds >= ((size_t)1 << 32)) return P2GPU_E_ARG;  // (the contradiction word keeps the column in 8 bits)
  HIP_TRY(hipSetDevice(c->device));
  const double t0 = wall_ms();
  p2gpu_witness_plan *p = new p2gpu_witness_plan();
  p->c = c;
  p->n_seeds = (uint32_t)n_seeds;
  int rc;
  try {
    PlanRefusal r = plan_seeds(c->d, c->W, seed_cells, n_seeds, p->h_seed_cells);
    if (!r) r = check_generators(c->d, c->R, p->h_gens);
    rc = r ? plan_refuse(c, r) : compile(p);
  } catch (...) {
    p->release();
    delete p;
    throw;
  }
  if (rc) {
    p->release();
    delete p;
    return rc;
  }
  p->compile_ms = wall_ms() - t0;
  *out = p;
  return P2GPU_OK;
}

// the two record forms of the generator list in front of plan_new
int plan_new_gen(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator *generators, size_t n_generators,
                 p2gpu_witness_plan **out, int (*compile)(p2gpu_witness_plan *)) {
  const PlanGenerator *recs = reinterpret_cast<const PlanGenerator *>(generators);
  return plan_new(c, seed_cells, n_seeds, n_generators, 0,
                  [=](uint32_t d, uint32_t R, PlanGenList &list) { return plan_generators(d, R, recs, n_generators, list); }, out, compile);
}
int plan_new_genv(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator_v *generators, size_t n_generators,
                  const uint32_t *cells, size_t n_cells, p2gpu_witness_plan **out, int (*compile)(p2gpu_witness_plan *)) {
  const PlanGeneratorV *recs = reinterpret_cast<const PlanGeneratorV *>(generators);
  return plan_new(c, seed_cells, n_seeds, n_generators, n_cells,
                  [=](uint32_t d, uint32_t R, PlanGenList &list) { return plan_generators_v(d, R, recs, n_generators, cells, n_cells, list); }, out, compile);
}

}  // namespace

namespace p2 {

int plan_reserve(p2gpu_witness_plan *p, size_t batch) {
  if (batch <= p->cap) return P2GPU_OK;
  // (the one set goes before the larger one comes: a call that fails here leaves cap = 0, and the next call allocates again)
  p->release_values();
  HIP_TRY(p->val.alloc(batch * std::max<uint32_t>(1, p->slots)));
  HIP_TRY(p->seed_vals.alloc(batch * std::max<uint32_t>(1, p->n_seeds)));
  HIP_TRY(p->err.alloc(batch));
  HIP_TRY(hipHostMalloc((void **)&p->pin, 8 * batch * ((size_t)p->n_seeds + 1), hipHostMallocDefault));
  p->cap = batch;
  return P2GPU_OK;
}

}  // namespace p2

extern "C" {

int p2gpu_witness_plan_create(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, p2gpu_witness_plan **out) try {
  return plan_new_gen(c, seed_cells, n_seeds, nullptr, 0, out, plan_compile);
} P2GPU_CATCH

int p2gpu_witness_plan_build(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, p2gpu_witness_plan **out) try {
  return plan_new_gen(c, seed_cells, n_seeds, nullptr, 0, out, plan_build);
} P2GPU_CATCH

int p2gpu_witness_plan_create_gen(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator *generators,
                                  size_t n_generators, p2gpu_witness_plan **out) try {
  return plan_new_gen(c, seed_cells, n_seeds, generators, n_generators, out, plan_compile);
} P2GPU_CATCH

int p2gpu_witness_plan_build_gen(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator *generators,
                                 size_t n_generators, p2gpu_witness_plan **out) try {
  return plan_new_gen(c, seed_cells, n_seeds, generators, n_generators, out, plan_build);
} P2GPU_CATCH

int p2gpu_witness_plan_create_genv(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator_v *generators,
                                   size_t n_generators, const uint32_t *cells, size_t n_cells, p2gpu_witness_plan **out) try {
  return plan_new_genv(c, seed_cells, n_seeds, generators, n_generators, cells, n_cells, out, plan_compile);
} P2GPU_CATCH

int p2gpu_witness_plan_build_genv(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator_v *generators,
                                  size_t n_generators, const uint32_t *cells, size_t n_cells, p2gpu_witness_plan **out) try {
  return plan_new_genv(c, seed_cells, n_seeds, generators, n_generators, cells, n_cells, out, plan_build);
} P2GPU_CATCH

int p2gpu_witness_plan_export_generators_v(const p2gpu_witness_plan *p, uint32_t *off, uint32_t *table, size_t sizes[2]) try {
  if (!p || !sizes) return P2GPU_E_ARG;
  const size_t n_gens = p->h_gens.size(), n_words = p->h_gens.n_cells();
  sizes[0] = n_gens; sizes[1] = n_words;
  if (!off && !table) return P2GPU_OK;
  if (!off || !table) return P2GPU_E_ARG;
  const p2gpu_circuit *c = p->c;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(off, p->gen_off.p, 4 * (n_gens + 1), hipMemcpyDeviceToHost, c->stream));
  if (n_words) HIP_TRY(hipMemcpyAsync(table, p->gen_table.p, 4 * n_words, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return P2GPU_OK;
} P2GPU_CATCH

int p2gpu_witness_plan_export_generators(const p2gpu_witness_plan *p, uint32_t *table, size_t *n_generators) try {
  if (!p || !n_generators) return P2GPU_E_ARG;
  *n_generators = p->h_gens.size();
  if (!p->h_gens.four_cells_each()) {
    set_err("p2gpu_witness_plan_export_generators: a generator of this plan has more than four cells (p2gpu_witness_plan_export_generators_v reads it)");
    return P2GPU_E_ARG;
  }
  if (!table || p->h_gens.empty()) return P2GPU_OK;
  const p2gpu_circuit *c = p->c;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(table, p->gen_table.p, 4 * (size_t)PLAN_GEN_CELLS * p->h_gens.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return P2GPU_OK;
} P2GPU_CATCH

int p2gpu_witness_plan_export(const p2gpu_witness_plan *p, uint32_t *cell_slot, uint64_t *ops, uint32_t *level_off, size_t sizes[3]) try {
  if (!p || !sizes) return P2GPU_E_ARG;
  const p2gpu_circuit *c = p->c;
  const size_t tot = (size_t)c->R * c->n;
  sizes[0] = tot; sizes[1] = p->n_ops; sizes[2] = (size_t)p->levels + 1;
  if (!cell_slot && !ops && !level_off) return P2GPU_OK;
  if (!cell_slot || !ops || !level_off) return P2GPU_E_ARG;
  static_assert(sizeof(OpRec) == sizeof(uint64_t), "an op record is one 64-bit word: row | (code | sub << 8) << 32");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(cell_slot, p->cell_slot.p, 4 * tot, hipMemcpyDeviceToHost, c->stream));
  if (p->n_ops) HIP_TRY(hipMemcpyAsync(ops, p->ops.p, sizeof(OpRec) * p->n_ops, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(level_off, p->level_off.p, 4 * sizes[2], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return P2GPU_OK;
} P2GPU_CATCH

void p2gpu_witness_plan_destroy(p2gpu_witness_plan *p) {
  if (!p) return;
  (void)hipSetDevice(p->c->device);
  (void)hipStreamSynchronize(p->c->stream);
  p->release();
  delete p;
}

int p2gpu_witness_plan_info(const p2gpu_witness_plan *p, uint64_t counts[5], double ms[2]) {
  if (!p || !counts || !ms) return P2GPU_E_ARG;
  counts[0] = p->n_ops; counts[1] = p->levels; counts[2] = p->widest; counts[3] = p->slots; counts[4] = p->n_seeds;
  ms[0] = p->compile_ms; ms[1] = p->walk_ms;
  return P2GPU_OK;
}

}  // extern "C"
