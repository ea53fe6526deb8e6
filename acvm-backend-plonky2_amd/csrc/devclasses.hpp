// devclasses.hpp -- lock-free union-find on the device, shared by build.hip (copy pairs -> sigma) and genplan.hip (sigma -> copy
// classes).  The kernels are generic over the PAIR SOURCE P, which names the two cell keys of pair i:
//   __device__ bool P::get(size_t i, uint32_t &a, uint32_t &b) const      false: entry i holds no pair
// build.hip numbers cells key = row * R + col over the caller's copy pairs, genplan.hip key = col << d | row over the decoded
// partner of every routed cell.
//   touch   every cell named by a pair becomes its own class (parent[key] = key; untouched cells stay UNSET) and is appended
//           once to the list of touched cells;
//   hook    for every pair whose ends point at different cells, atomicMin(parent[larger], smaller);
//   jump    parent[x] <- parent[parent[...]] until every touched cell points at a root.
// Rounds of { hook, jump until settled } until no pair hooks.  Parents only ever decrease and only within a true class, so the
// fixed point is parent[x] = the smallest key of x's class whatever order the atomics land in.  No thread ever waits for
// another one or retries.
#pragma once
#include <algorithm>
#include <vector>
#include "gl.hpp"

namespace p2 {
namespace classes {

constexpr uint32_t UNSET = 0xFFFFFFFFu;  // no cell's key
constexpr uint32_t TPB = 256;
constexpr int JUMP_STEPS = 32;  // parent look-ups of one thread in one jump launch

inline uint32_t grid_for(size_t count) { return (uint32_t)std::min<size_t>(std::max<size_t>(1, (count + TPB - 1) / TPB), (size_t)1 << 16); }

// parent[] is read while other threads of the same launch lower it: one 32-bit load, exactly once, never re-read
__device__ __forceinline__ uint32_t ld_parent(const uint32_t *p) { return __atomic_load_n(p, __ATOMIC_RELAXED); }

__device__ __forceinline__ void touch_cell(uint32_t x, uint32_t *parent, unsigned long long *list, unsigned long long *count) {
  // the plain load is a filter only (a hub cell named by thousands of pairs costs one atomic per wave that still sees it
  // untouched, not one per pair); the compare-and-swap decides who appends the cell
  if (ld_parent(parent + x) != UNSET) return;
  if (atomicCAS(&parent[x], UNSET, x) == UNSET) list[atomicAdd(count, 1ull)] = x;
}

template <class P>
__global__ void touch_kernel(P pairs, size_t num_pairs, uint32_t *parent, unsigned long long *list, unsigned long long *count) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < num_pairs; i += step) {
    uint32_t a, b;
    if (!pairs.get(i, a, b)) continue;
    touch_cell(a, parent, list, count);
    if (b != a) touch_cell(b, parent, list, count);
  }
}

// Before the first launch parent is the identity on the touched cells, before every later one each touched cell points at a
// root.  A value read here may already have been lowered by another thread of the same launch: it is then still a cell of
// the same class, which is all the atomicMin needs.  A pair whose link lost against a smaller one hooks again next round.
template <class P>
__global__ void hook_kernel(P pairs, size_t num_pairs, uint32_t *parent, uint32_t *changed) {
  const size_t step = (size_t)gridDim.x * TPB;
  bool any = false;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < num_pairs; i += step) {
    uint32_t a, b;
    if (!pairs.get(i, a, b)) continue;
    const uint32_t pa = ld_parent(parent + a), pb = ld_parent(parent + b);
    if (pa == pb) continue;
    any = true;
    const uint32_t hi = max(pa, pb), lo = min(pa, pb);
    if (ld_parent(parent + hi) > lo) atomicMin(&parent[hi], lo);  // (filter: a star's hub takes one atomic per improvement, not per pair)
  }
  if (any) *changed = 1;
}

// parent[x] <- an ancestor up to STEPS links higher (callers: JUMP_STEPS).  Stores go to the thread's own cell, values read are ancestors
// whenever they were written, roots do not change during the launch.
template <int STEPS>
__global__ void jump_kernel(const unsigned long long *list, size_t count, uint32_t *parent, uint32_t *changed) {
  const size_t step = (size_t)gridDim.x * TPB;
  bool any = false;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < count; i += step) {
    const uint32_t x = (uint32_t)list[i];
    const uint32_t p0 = ld_parent(parent + x);
    uint32_t p = p0, g = ld_parent(parent + p);
    for (int k = 0; k < STEPS && g != p; k++) {
      p = g;
      g = ld_parent(parent + p);
    }
    if (g != p) any = true;
    if (p != p0) __atomic_store_n(parent + x, p, __ATOMIC_RELAXED);
  }
  if (any) *changed = 1;
}

// w^row from the forward twiddles tw[i] = w^i, i < n / 2:  w^(i + n/2) = -w^i
__device__ __forceinline__ gl_t subgroup_power(const gl_t *tw, uint32_t d, uint32_t row) {
  const uint32_t half = 1u << (d - 1);
  const gl_t v = tw[row & (half - 1)];
  return row & half ? gl_sub(0, v) : v;
}

// the device scratch of one compilation: everything is released when it goes out of scope
struct Scratch {
  std::vector<void *> ptrs;
  Scratch() = default;
  Scratch(const Scratch &) = delete;
  Scratch &operator=(const Scratch &) = delete;
  ~Scratch() { release(); }
  void release() {
    for (void *p : ptrs) (void)hipFree(p);
    ptrs.clear();
  }
  template <class T> T *alloc(size_t n) {
    void *p = nullptr;
    if (hipMalloc(&p, (n ? n : 1) * sizeof(T)) != hipSuccess) {
      (void)hipGetLastError();
      return nullptr;
    }
    ptrs.push_back(p);
    return (T *)p;
  }
};

}  // namespace classes
}  // namespace p2
