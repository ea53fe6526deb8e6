// genplan.hpp -- what the two plan compilers of the device witness share: the host one in genwit.hip (plan_compile, the
// differential oracle) and the device one in genplan.hip (plan_compile_device).  Both hand the same three arrays to
// genwit.hip's plan_finish.
#pragma once
#include <vector>
#include "devclasses.hpp"
#include "genops.hpp"
#include "prover_internal.hpp"

namespace p2 {

constexpr uint32_t PLAN_UNSET = 0xFFFFFFFFu;   // cell without a slot
constexpr uint32_t PLAN_WRITER = 0x80000000u;  // cell_slot bit: this cell's op writes the slot (every other one compares)
// x: the row (OP_SEED: the seed's index), y: code | sub << 8 (the slot / copy inside the row)
typedef uint2 OpRec;

// a compiled plan before it is attached to a handle: host memory (kind = hipMemcpyHostToDevice) or device memory
struct PlanArrays {
  const uint32_t *cell_slot = nullptr;  // [R][n]
  const OpRec *ops = nullptr;           // [n_ops], by (level, creation order)
  const uint32_t *level_off = nullptr;  // [levels + 1]
  uint32_t levels = 0, slots = 0, widest = 0;
  size_t n_ops = 0;
  hipMemcpyKind kind = hipMemcpyHostToDevice;
};

// The plan of circuit c for `seeds` ((row, col), already checked against the matrix and each other), compiled on c->stream.
// The arrays of `out` live in S, which the caller releases once plan_finish has copied them.  Refusals carry
// p2gpu_witness_plan_create's codes and words.
int plan_compile_device(p2gpu_circuit *c, const std::vector<uint2> &seeds, classes::Scratch &S, PlanArrays &out);

}  // namespace p2
