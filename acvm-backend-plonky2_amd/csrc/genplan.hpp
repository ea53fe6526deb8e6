// genplan.hpp -- what the two plan compilers of the device witness share inside the library: the host one (planhost.hpp, run by
// witplan.hip's plan_compile: the differential oracle) and the device one (genplan.hip, plan_compile_device).  Both hand the
// same three arrays to witplan.hip's plan_finish and word their refusals through planhost.hpp's plan_refusal_text.
#pragma once
#include <vector>
#include "planhost.hpp"
#include "prover_internal.hpp"

namespace p2 {

namespace classes {
struct Scratch;  // devclasses.hpp
}

// x: the row (OP_SEED: the seed's index, OP_EQUALITY .. OP_GLV_DECOMPOSE: the generator's), y: code | sub << 8 (the slot / copy inside the row): HostPlan's 64-bit word
typedef uint2 OpRec;
static_assert(sizeof(PlanSeed) == sizeof(uint2), "the kernels read a seed cell as a uint2 (row, col)");

// a compiled plan before it is attached to a handle: host memory (kind = hipMemcpyHostToDevice) or device memory
struct PlanArrays {
  const uint32_t *cell_slot = nullptr;  // [R][n]
  const OpRec *ops = nullptr;           // [n_ops], by (level, creation order)
  const uint32_t *level_off = nullptr;  // [levels + 1]
  const uint32_t *gen_table = nullptr;  // [n_gen_cells]: one word per cell a generator names (the offsets are the checked list's)
  size_t n_gen_cells = 0;
  uint32_t levels = 0, slots = 0, widest = 0;
  size_t n_ops = 0;
  hipMemcpyKind kind = hipMemcpyHostToDevice;
};

// a refusal of either compiler as the call's result: p2gpu_last_error's text and the code
inline int plan_refuse(const p2gpu_circuit *c, const PlanRefusal &r) {
  set_err("%s", plan_refusal_text(r, c->d, c->W, c->R).c_str());
  return P2GPU_E_ARG;
}

// The decode of the handle's sigma columns, shared by the plan compiler and the witness check (check.hip): partner [R][n] (device,
// the caller's) <- for every routed cell x, numbered key = col << d | row as sigma is laid out, the key sigma[x] names;
// PLAN_UNSET for a fixed point and for a refused value (>= p, or naming no routed cell), the smallest refused key through an
// atomicMin on *bad (a device word the caller presets to UINT64_MAX).  The tables it needs (the cosets' n-th powers, the sorted
// powers of w) live in S; everything is enqueued on c->stream, d >= 1.  A failing runtime call comes back with its step's words.
hipError_t sigma_partners(p2gpu_circuit *c, classes::Scratch &S, uint32_t *partner, unsigned long long *bad, const char **step);

// The plan of circuit c for `seeds` (already through plan_seeds) and `gens` (already through plan_generators), compiled on c->stream.  The arrays of `out` live in S,
// which the caller releases once plan_finish has copied them.  Refusals carry p2gpu_witness_plan_create's codes and words.
int plan_compile_device(p2gpu_circuit *c, const std::vector<PlanSeed> &seeds, const PlanGenList &gens, classes::Scratch &S, PlanArrays &out);

}  // namespace p2
