// verifydev.hip -- p2gpu_verify_batch: the verifier core (verifycore.hpp) as kernels, a verdict per proof of a batch.
//   verify_head_kernel<HK>   one lane per proof: canonicity, public-input hash, transcript, zeta^n != 1, the plonk identity at
//                            zeta, proof-of-work.  The transcript is serial inside a proof and the same sequence of steps in every
//                            proof of a circuit, so the lanes of a wave never diverge before one of them rejects, and nothing
//                            crosses lanes.  Leaves a HeadRecord and the head's reason per proof.
//   verify_query_kernel<HK>  one lane per (proof, query): skips proofs whose head failed, runs verify_query, writes its reason
//                            and the oracle / step it names.
//   verify_verdict_kernel    one lane per proof: the head's reason if there is one, else that of the lowest failing query --
//                            the verdict of the host's loop, which stops at the first failure in this order.
// Waves are 64 proofs (or proof-query pairs) wide and blocks are one wave: the work of a lane is long and latency-bound (a
// few hundred dependent hash permutations), so what matters is that the waves of a batch spread over all compute units.
// Run-time-indexed per-lane arrays (sponge state, constraint terms) are in scratch, element i of lane b at [i * lanes + b]:
// the lanes of a wave touch neighbouring words.  Everything else a lane needs it reads from its proof, at offsets the circuit
// fixes (verifycore.hpp states why no proof byte can move a read); proofs are uploaded back to back at their common length,
// the buffer padded so that the aligned words ld64() reads are inside it.
// Proofs of another length than the circuit's get their verdict on the host and are not uploaded.  Scratch, the proofs and the
// circuit's share (gate table, cap, k_is, round constants: a few kilobytes) are allocated per call and freed before it returns.
// The entry points for compressed proofs (decompressdev.hip) end in the query and verdict kernels of this file: launch_queries,
// the device and the circuit's upload are shared through verifydev.hpp, and DevArgs::cflags carries what the decompression found.
#include "verifydev.hpp"

using namespace p2;
using p2::vdev::CallState;
using p2::vdev::DevArgs;

namespace {

const char *const VB_ENTRY = "p2gpu_verify_batch";

template <int HK>
__global__ __launch_bounds__(64) void verify_head_kernel(const DevArgs a) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.m) return;
  a.head_reason[b] = vc::verify_head<HK>(a.c, a.L, a.proofs + (size_t)b * a.L.want, vc::Strided<gl_t>{a.sponge + b, a.m},
                                         vc::Strided<ext_t>{a.terms + b, a.m}, a.rec + b);
}

template <int HK>
__global__ __launch_bounds__(64) void verify_query_kernel(const DevArgs a) {
  const uint32_t lane = blockIdx.x * blockDim.x + threadIdx.x, nq = a.c.num_queries;
  const uint32_t b = lane / nq, q = lane - b * nq;
  if (b >= a.m || a.head_reason[b] != vc::VR_OK || (a.cflags && a.cflags[b])) return;
  uint32_t index = vc::VR_NONE;
  const uint32_t r = vc::verify_query<HK>(a.c, a.L, a.proofs + (size_t)b * a.L.want, a.rec + b, q, &index);
  a.query_reason[2 * (size_t)lane] = r;
  a.query_reason[2 * (size_t)lane + 1] = index;
}

__global__ __launch_bounds__(64) void verify_verdict_kernel(const DevArgs a) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x, nq = a.c.num_queries;
  if (b >= a.m) return;
  // a compressed proof: the container, the indices against the transcript's, the initial paths, the step paths -- then the head
  uint32_t reason = a.cflags && a.cflags[b] ? dc::flags_reason(a.cflags[b]) : a.head_reason[b], query = vc::VR_NONE, index = vc::VR_NONE;
  if (reason == vc::VR_OK)
    for (uint32_t q = 0; q < nq; q++) {
      const uint32_t r = a.query_reason[2 * ((size_t)b * nq + q)];
      if (r != vc::VR_OK) {
        reason = r;
        query = q;
        index = a.query_reason[2 * ((size_t)b * nq + q) + 1];
        break;
      }
    }
  a.verdict[3 * (size_t)b] = reason;
  a.verdict[3 * (size_t)b + 1] = query;
  a.verdict[3 * (size_t)b + 2] = index;
}

void launch_head(const DevArgs &a, hipStream_t st) {
  ProfScope ps("verify_head_kernel", (double)a.L.queries_at * a.m);
  if (a.c.hasher) hipLaunchKernelGGL(verify_head_kernel<1>, dim3((a.m + 63) / 64), dim3(64), 0, st, a);
  else hipLaunchKernelGGL(verify_head_kernel<0>, dim3((a.m + 63) / 64), dim3(64), 0, st, a);
}

}  // namespace

namespace p2 {
namespace vdev {

void launch_queries(const DevArgs &a, hipStream_t st) {
  const uint32_t lanes = a.m * a.c.num_queries;
  {
    ProfScope ps("verify_query_kernel", (double)a.L.query_bytes * lanes);
    if (a.c.hasher) hipLaunchKernelGGL(verify_query_kernel<1>, dim3((lanes + 63) / 64), dim3(64), 0, st, a);
    else hipLaunchKernelGGL(verify_query_kernel<0>, dim3((lanes + 63) / 64), dim3(64), 0, st, a);
  }
  hipLaunchKernelGGL(verify_verdict_kernel, dim3((a.m + 63) / 64), dim3(64), 0, st, a);
}

int open_device(const char *VB_ENTRY, const p2gpu_circuit *c, CallState &S, hipStream_t *st) {
  int prev = 0;
  VB_TRY(hipGetDevice(&prev), "query the device");
  S.prev_device = prev;
  VB_TRY(hipSetDevice(c->device >= 0 ? c->device : g_devices[0]), "select the device");
  if (c->device >= 0) *st = c->stream;
  else {
    VB_TRY(hipStreamCreateWithFlags(&S.own_stream, hipStreamNonBlocking), "create a stream");
    *st = S.own_stream;
  }
  return 0;
}

int upload_circuit(const char *VB_ENTRY, CallState &S, const vc::CircuitView &hv, vc::CircuitView *dv, hipStream_t st) {
  const size_t ncap = (size_t)1 << hv.cap_h;
  GateDesc *d_gates = S.alloc<GateDesc>(hv.num_gates);
  gl_t *d_kis = S.alloc<gl_t>(hv.R), *d_prc = S.alloc<gl_t>(360);
  dig_t *d_cap = S.alloc<dig_t>(ncap);
  if (!d_gates || !d_kis || !d_prc || !d_cap) return device_fail(VB_ENTRY, "scratch", hipErrorOutOfMemory);
  *dv = hv;
  dv->gates = d_gates; dv->k_is = d_kis; dv->prc = d_prc; dv->cs_cap = d_cap;
  VB_TRY(hipMemcpyAsync(d_gates, hv.gates, sizeof(GateDesc) * hv.num_gates, hipMemcpyHostToDevice, st), "copy the gate table");
  if (hv.R) VB_TRY(hipMemcpyAsync(d_kis, hv.k_is, 8 * (size_t)hv.R, hipMemcpyHostToDevice, st), "copy k_is");
  VB_TRY(hipMemcpyAsync(d_prc, hv.prc, 8 * 360, hipMemcpyHostToDevice, st), "copy the round constants");
  VB_TRY(hipMemcpyAsync(d_cap, hv.cs_cap, sizeof(dig_t) * ncap, hipMemcpyHostToDevice, st), "copy the cap");
  return 0;
}

}  // namespace vdev
}  // namespace p2

extern "C" int p2gpu_verify_batch(const p2gpu_circuit *c, const uint8_t *proofs, const size_t *offsets, size_t batch,
                                  p2gpu_verify_report *reports) try {
  if (int rc = verify_batch_args(c, proofs, offsets, batch, reports)) return rc;
  const vc::CircuitView hv = view_of(c);
  const vc::Layout L = vc::make_layout(hv);
  // ---- the shape step, on the host: only proofs of the circuit's length go to the device ----
  std::vector<size_t> slot;  // batch index of device proof i
  for (size_t b = 0; b < batch; b++) {
    const size_t len = offsets[b + 1] - offsets[b];
    const uint8_t *p = proofs + offsets[b];
    const vc::Verdict v = hv.hasher ? vc::shape_verdict<1>(hv, L, p, len) : vc::shape_verdict<0>(hv, L, p, len);
    if (v.reason) verify_report_fill(&reports[b], v);
    else slot.push_back(b);
  }
  if (slot.size() > UINT32_MAX / 64) {
    set_err("p2gpu_verify_batch: %zu proofs in one call", slot.size());
    return P2GPU_E_ARG;
  }
  // ---- the device: the handle's own, or the first of p2gpu_init for a verifier-only handle ----
  if (int rc = ensure_device()) return rc;  // (also when no proof is left for it: never a silent host-only answer)
  const uint32_t m = (uint32_t)slot.size();
  CallState S;
  hipStream_t st = nullptr;
  if (m)
    if (int rc = vdev::open_device(VB_ENTRY, c, S, &st)) return rc;
  if (m) {
    // the "profile" knob of a prover handle times the launches below like every other launch on its stream: the kernel
    // statistics are the one part of a handle this call changes (include/p2gpu.h says so), hence the cast
    p2gpu_circuit *pc = c->device >= 0 ? const_cast<p2gpu_circuit *>(c) : nullptr;
    std::unique_ptr<ProfGuard> prof(pc && pc->profile ? new ProfGuard(pc) : nullptr);
    const size_t nterms = vc::identity_terms(hv), lanes = (size_t)m * hv.num_queries;
    const size_t proof_bytes = (size_t)m * L.want;
    DevArgs a;
    a.L = L;
    a.m = m;
    a.cflags = nullptr;
    uint8_t *d_proofs = S.alloc<uint8_t>(proof_bytes + 16);
    a.sponge = S.alloc<gl_t>(12 * (size_t)m);
    a.terms = S.alloc<ext_t>(nterms * m);
    a.rec = S.alloc<vc::HeadRecord>(m);
    a.head_reason = S.alloc<uint32_t>(m);
    a.query_reason = S.alloc<uint32_t>(2 * lanes);
    a.verdict = S.alloc<uint32_t>(3 * (size_t)m);
    if (!d_proofs || !a.sponge || !a.terms || !a.rec || !a.head_reason || !a.query_reason || !a.verdict)
      return vdev::device_fail(VB_ENTRY, "scratch", hipErrorOutOfMemory);
    a.proofs = d_proofs;
    if (int rc = vdev::upload_circuit(VB_ENTRY, S, hv, &a.c, st)) return rc;
    VB_TRY(hipMemsetAsync(d_proofs + proof_bytes, 0, 16, st), "clear the padding");
    // proofs that lie back to back in the caller's buffer go up in one copy
    for (uint32_t i = 0; i < m;) {
      uint32_t j = i + 1;
      while (j < m && slot[j] == slot[j - 1] + 1 && offsets[slot[j]] == offsets[slot[j - 1]] + L.want) j++;
      VB_TRY(hipMemcpyAsync(d_proofs + (size_t)i * L.want, proofs + offsets[slot[i]], (size_t)(j - i) * L.want, hipMemcpyHostToDevice, st),
             "copy the proofs");
      i = j;
    }
    launch_head(a, st);
    vdev::launch_queries(a, st);
    VB_TRY(hipGetLastError(), "launch");
    std::vector<uint32_t> verdict(3 * (size_t)m);
    VB_TRY(hipMemcpyAsync(verdict.data(), a.verdict, 12 * (size_t)m, hipMemcpyDeviceToHost, st), "read the verdicts");
    VB_TRY(hipStreamSynchronize(st), "verify");
    for (uint32_t i = 0; i < m; i++) {
      const vc::Verdict v{verdict[3 * (size_t)i], verdict[3 * (size_t)i + 1], verdict[3 * (size_t)i + 2]};
      if (v.reason >= vc::VR_COUNT) {
        set_err("p2gpu_verify_batch: internal error (reason %u)", v.reason);
        return P2GPU_E_DEVICE;
      }
      verify_report_fill(&reports[slot[i]], v);
    }
  }
  return verify_batch_finish(batch, offsets, L, reports);
} P2GPU_CATCH
