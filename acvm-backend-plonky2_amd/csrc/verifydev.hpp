// verifydev.hpp -- what the device entry points of the verifier share: p2gpu_verify_batch (verifydev.hip) and the entry points
// for compressed proofs (decompressdev.hip), which end in the same query and verdict kernels.
#pragma once
#include "hostproof.hpp"
#include "prover_internal.hpp"

namespace p2 {
namespace vdev {

struct DevArgs {
  vc::CircuitView c;  // device pointers
  vc::Layout L;
  const uint8_t *proofs;  // [m] proofs of L.want bytes, back to back
  uint32_t m;
  gl_t *sponge;            // [12][m]
  ext_t *terms;            // [identity_terms][m]
  vc::HeadRecord *rec;     // [m]
  uint32_t *head_reason;   // [m]
  uint32_t *query_reason;  // [m * num_queries][2]: reason, oracle / step
  uint32_t *verdict;       // [m][3]: reason, query, index
  const uint32_t *cflags;  // [m] or null: what the decompression found (dc::F_*), which ranks before the head's reason
};

// what one call allocates: freed, the stream of a verifier-only handle destroyed and the caller's device selected again when it ends
struct CallState {
  std::vector<void *> ptrs;
  hipStream_t own_stream = nullptr;
  int prev_device = -1;
  ~CallState() {
    for (void *p : ptrs) (void)hipFree(p);
    if (own_stream) (void)hipStreamDestroy(own_stream);
    if (prev_device >= 0) (void)hipSetDevice(prev_device);
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

// `entry`: the C function that speaks
inline int device_fail(const char *entry, const char *what, hipError_t e) {
  (void)hipGetLastError();
  set_err("%s: %s: %s", entry, what, hipGetErrorString(e));
  return P2GPU_E_DEVICE;
}
#define VB_TRY(expr, what)                                     \
  do {                                                         \
    const hipError_t e_ = (expr);                              \
    if (e_ != hipSuccess) return p2::vdev::device_fail(VB_ENTRY, what, e_); \
  } while (0)

// ---- verifydev.hip ----
// the handle's own device and stream, or the first device of p2gpu_init and a stream of the call's for a verifier-only handle
int open_device(const char *entry, const p2gpu_circuit *c, CallState &S, hipStream_t *st);
// the circuit's share (gate table, cap, k_is, round constants) to the device; *dv: hv with device pointers
int upload_circuit(const char *entry, CallState &S, const vc::CircuitView &hv, vc::CircuitView *dv, hipStream_t st);
// verify_query_kernel and verify_verdict_kernel over a.proofs, behind whatever left a.rec and a.head_reason
void launch_queries(const DevArgs &a, hipStream_t st);

}  // namespace vdev
}  // namespace p2
