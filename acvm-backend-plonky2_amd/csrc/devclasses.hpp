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
// another one or retries.  settle() is that loop; Scratch holds a compilation's device memory and runs rocprim's scans and
// sorts on a temporary it grows on demand.
#pragma once
#include <algorithm>
#include <cstring>  // (rocprim's headers use memcpy without including it)
#include <vector>
#include <rocprim/rocprim.hpp>
#include "circuit.hpp"
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

// Rounds of { hook, jump until settled } over the touched cells list[0 .. T), T > 0, until no pair hooks; `flag` (a device
// word) is cleared in front of every launch and read back behind it.  While a pair is left to hook, every round removes at
// least one root; in practice a handful of rounds.  The bounds are backstops against a defect, not part of the algorithm:
// past them the call fails, it never loops on.  `who` opens the error text.
template <class P>
int settle(const P &pairs, size_t num_pairs, const unsigned long long *list, size_t T, uint32_t *parent, uint32_t *flag, hipStream_t st,
           const char *who) {
  uint32_t hc = 0;
  auto ok = [&](hipError_t e, const char *what) {
    if (e == hipSuccess) return true;
    (void)hipGetLastError();
    set_err("%s: %s: %s", who, what, hipGetErrorString(e));
    return false;
  };
  auto clear = [&] { return ok(hipMemsetAsync(flag, 0, 4, st), "scratch"); };
  auto read = [&](const char *what) { return ok(hipMemcpyAsync(&hc, flag, 4, hipMemcpyDeviceToHost, st), "read flag") && ok(hipStreamSynchronize(st), what); };
  for (int round = 0;; round++) {
    if (round > (1 << 16)) { set_err("%s: internal error (classes did not settle)", who); return P2GPU_E_DEVICE; }
    if (!clear()) return P2GPU_E_DEVICE;
    hipLaunchKernelGGL(hook_kernel<P>, dim3(grid_for(num_pairs)), dim3(TPB), 0, st, pairs, num_pairs, parent, flag);
    if (!read("hook")) return P2GPU_E_DEVICE;
    if (!hc) break;
    for (int j = 0;; j++) {
      if (j > 64) { set_err("%s: internal error (compression did not settle)", who); return P2GPU_E_DEVICE; }
      if (!clear()) return P2GPU_E_DEVICE;
      hipLaunchKernelGGL(jump_kernel<JUMP_STEPS>, dim3(grid_for(T)), dim3(TPB), 0, st, list, T, parent, flag);
      if (!read("jump")) return P2GPU_E_DEVICE;
      if (!hc) break;
    }
  }
  return P2GPU_OK;
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
    tmp = nullptr;
    tmp_cap = 0;
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
  // rocprim's temporary storage, grown on demand (an outgrown one stays until release()), and the three calls that use it:
  // size query, grow, run.  A failure comes back with the step it happened in, in the words of the sorts' error texts.
  // Templates, so that a unit holds the kernels of the calls it makes and no others; pointer and size types as the callers
  // have them: they name rocprim's kernels.
  struct Result {
    hipError_t e;
    const char *step;
  };
  void *tmp = nullptr;
  size_t tmp_cap = 0;
  template <class Run> Result with_tmp(Run &&run) {
    size_t bytes = 0;
    const hipError_t e = run(nullptr, bytes);
    if (e != hipSuccess) return {e, "sort (size)"};
    if (bytes > tmp_cap) {
      tmp = alloc<uint8_t>(bytes);
      tmp_cap = tmp ? bytes : 0;
      if (!tmp) return {hipErrorOutOfMemory, "scratch (sort)"};
    }
    return {run(tmp, tmp_cap), "sort"};
  }
  template <class T> hipError_t exclusive_scan(const T *in, T *out, size_t m, hipStream_t st) {
    return with_tmp([&](void *t, size_t &b) { return rocprim::exclusive_scan(t, b, in, out, T(0), m, rocprim::plus<T>(), st); }).e;
  }
  template <class K, class N> Result radix_sort_keys(K *in, K *out, N m, unsigned bit0, unsigned bit1, hipStream_t st) {
    return with_tmp([&](void *t, size_t &b) { return rocprim::radix_sort_keys(t, b, in, out, m, bit0, bit1, st); });
  }
  template <class K, class V, class N>
  Result radix_sort_pairs(K *kin, K *kout, V *vin, V *vout, N m, unsigned bit0, unsigned bit1, hipStream_t st) {
    return with_tmp([&](void *t, size_t &b) { return rocprim::radix_sort_pairs(t, b, kin, kout, vin, vout, m, bit0, bit1, st); });
  }
};

}  // namespace classes
}  // namespace p2
