// witplan.hpp -- the witness plan object: made and owned by witplan.hip (either compiler, then plan_finish), run by genwit.hip.
#pragma once
#include "genplan.hpp"

struct p2gpu_witness_plan {
  p2gpu_circuit *c = nullptr;
  uint32_t n_seeds = 0, levels = 0, slots = 0, widest = 0;
  size_t n_ops = 0;
  double compile_ms = 0, walk_ms = 0;
  std::vector<p2::OpRec> h_ops;  // the schedule, to name the cell of a contradiction
  p2::DBuf<p2::OpRec> ops;
  p2::DBuf<uint32_t> level_off, cell_slot;
  p2::DBuf<uint2> seed_cells;
  std::vector<p2::PlanSeed> h_seed_cells;
  // the generators that are no gate's own: the checked list, and the plan's table (one word per cell a generator names: cell
  // key | PLAN_WRITER; generator g's words begin at h_gens.off[g]) on the device for the walk and on the host to name the cell
  // of a contradiction; gen_off [generators + 1] and gen_shape [generators] (PlanGenList::shape_word) are the list's, for the walk
  p2::PlanGenList h_gens;
  std::vector<uint32_t> h_gen_table;
  p2::DBuf<uint32_t> gen_table, gen_off, gen_shape;
  bool has_bigint = false;  // a big-integer generator (div-rem, nonnative) is listed: the walk kernel's form with those arms runs this plan
  // One bit per routed cell, set for a seed's cell that is also an output column of a row op of its row: the cell's writer bit is
  // the seed's there, and the row op compares (planhost.hpp, "writer bits").  Not allocated when the plan has no such cell.
  p2::DBuf<uint32_t> seed_out;
  bool has_seed_out = false;
  // The values of `cap` witnesses (plan_finish: 1; a batch grows them).  A call of B <= cap witnesses lays its values out
  // with its own B as the stride, in the front of the buffers: val [slots][B], seed_vals [n_seeds][B], err [B].
  size_t cap = 0;
  p2::DBuf<p2::gl_t> val, seed_vals;
  p2::DBuf<unsigned long long> err;
  p2::DBuf<p2::gl_t> batch_wires;  // [batch][W][n]: the matrices of p2gpu_prove_seeds_batch, grown to the largest batch seen
  uint64_t *pin = nullptr;  // page-locked: [n_seeds][B] staging of the seed values, then the B contradiction words
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  void release_values() {
    val.release(); seed_vals.release(); err.release(); batch_wires.release();
    if (pin) (void)hipHostFree(pin);
    pin = nullptr;
    cap = 0;
  }
  void release() {
    ops.release(); level_off.release(); cell_slot.release(); seed_cells.release(); gen_table.release(); gen_off.release(); gen_shape.release();
    seed_out.release();
    release_values();
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    ev0 = ev1 = nullptr;
  }
};

namespace p2 {

// the value buffers grown to hold `batch` witnesses (the stream is idle between calls: one call at a time per handle).
// Nothing is cleared: every slot has a writer (a plan with an unreached one is refused) and is written before it is read.
int plan_reserve(p2gpu_witness_plan *p, size_t batch);

}  // namespace p2
