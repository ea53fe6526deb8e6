// decompressdev.hip -- p2gpu_verify_batch_compressed and p2gpu_proof_decompress_batch: the decompression core
// (decompresscore.hpp) as kernels in front of the batch verifier's query and verdict kernels (verifydev.hip).
//   scatter_kernel<HK>   one wave per proof: head, tail and leaves to their place in the uncompressed proof, the canonicity
//                        checks of the container as flags
//   head_kernel<HK>      one lane per proof: the transcript, once -- the HeadRecord, the stored indices against the transcript's,
//                        the head's own reason kept aside (it ranks after every failure of the decompression)
//   infer_kernel         one wave per proof, one lane per query: the inferred evaluation of every fold step; a step boundary is
//                        a sync of the wave
//   rebuild_kernel<HK>   one wave per proof and tree (four initial trees, one per fold step), one lane per query: the full
//                        Merkle paths, layer by layer; digests cross lanes through LDS
// then verify_query_kernel and verify_verdict_kernel over the rebuilt bytes, unchanged but for the verdict's precedence.
// Blocks are one wave, as in verifydev.hip: a lane's work is a chain of dependent hash permutations, and the waves of a batch
// spread over the compute units.  A stage skips a proof an earlier stage has flagged; a wave is one proof, so the skip is uniform.
// The compressed proofs go up back to back at their own lengths with their offset tables (the host's container walk); the
// uncompressed bytes exist only in device memory unless p2gpu_proof_decompress_batch reads them back.  A proof whose walk fails
// is answered by the host's lone path and never uploaded.  Everything is allocated per call and freed before it returns.
#include "verifydev.hpp"

using namespace p2;
using p2::vdev::CallState;

namespace {

const char *const VB_ENTRY = "p2gpu_verify_batch_compressed";

struct DecArgs {
  vc::CircuitView c;  // device pointers
  vc::Layout L;
  const uint8_t *cbytes;  // the compressed proofs, back to back
  const uint64_t *coff;   // [m + 1]: where each begins
  const uint32_t *tabs;   // [m][table_words]
  uint32_t tw, m, judge;
  uint8_t *out;           // [m] proofs of L.want bytes
  gl_t *sponge;           // [12][m]
  ext_t *terms;           // [identity_terms][m]
  vc::HeadRecord *rec;    // [m]
  uint32_t *flags;        // [m]: dc::F_*
  uint32_t *head_reason;  // [m]
};

template <int HK>
__global__ __launch_bounds__(64) void scatter_kernel(const DecArgs a) {
  const uint32_t b = blockIdx.x;
  const uint32_t flags = dc::scatter_lane<HK>(a.c, a.L, a.cbytes + a.coff[b], a.tabs + (size_t)b * a.tw, a.out + (size_t)b * a.L.want, threadIdx.x, 64);
  if (flags) atomicOr(&a.flags[b], flags);
}

template <int HK>
__global__ __launch_bounds__(64) void head_kernel(const DecArgs a) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= a.m) return;
  a.head_reason[b] = vc::VR_OK;
  if (a.flags[b]) return;
  uint32_t head_reason;
  const uint32_t flags = dc::head_lane<HK>(a.c, a.L, a.cbytes + a.coff[b], a.out + (size_t)b * a.L.want, vc::Strided<gl_t>{a.sponge + b, a.m},
                                           vc::Strided<ext_t>{a.terms + b, a.m}, a.rec + b, a.judge != 0, &head_reason);
  a.head_reason[b] = head_reason;
  if (flags) a.flags[b] = flags;
}

__global__ __launch_bounds__(64) void infer_kernel(const DecArgs a) {
  const uint32_t b = blockIdx.x, q = threadIdx.x;
  if (a.flags[b]) return;
  const bool active = q < a.c.num_queries;
  const uint8_t *cp = a.cbytes + a.coff[b];
  const uint32_t *tab = a.tabs + (size_t)b * a.tw;
  uint8_t *out = a.out + (size_t)b * a.L.want;
  const vc::HeadRecord *rec = a.rec + b;
  dc::InferLane n;
  if (active) dc::infer_begin(a.c, a.L, out, rec, q, n);
  for (uint32_t s = 0; s < a.c.n_steps; s++) {
    if (active) dc::infer_place(a.c, a.L, cp, tab, out, rec, s, q, n);
    __syncthreads();  // the values a later query of the leaf copies are in place
    if (active) dc::infer_fold(a.c, a.L, out, rec, s, q, n);
  }
}

template <int HK>
__global__ __launch_bounds__(64) void rebuild_kernel(const DecArgs a) {
  __shared__ dc::TreeShared sh;
  const uint32_t ntrees = 4 + a.c.n_steps, b = blockIdx.x / ntrees, tree = blockIdx.x - b * ntrees, q = threadIdx.x, nq = a.c.num_queries;
  if (a.flags[b] & (dc::F_INIT_PATH - 1)) return;  // (the two path flags are this kernel's own, of other waves of the proof)
  const bool active = q < nq;
  const uint8_t *cp = a.cbytes + a.coff[b];
  uint8_t *out = a.out + (size_t)b * a.L.want;
  const dc::Tree T = dc::tree_of(a.c, a.L, tree);
  dc::PathLane n;
  bool ok = true;
  if (active) dc::rebuild_begin<HK>(a.c, a.L, cp, a.tabs + (size_t)b * a.tw, out, a.rec + b, tree, T, q, sh, n);
  __syncthreads();
  for (uint32_t layer = 0; layer < T.levels; layer++) {
    if (active) ok &= dc::rebuild_read<HK>(a.L, cp, nq, layer, q, sh, n);
    __syncthreads();  // every lane's digest and what the reading lanes read are in LDS
    if (active) dc::rebuild_hash<HK>(a.c, a.L, out, layer, q, sh, n);
    __syncthreads();  // ... and have been taken: the next layer overwrites them
  }
  if (active) ok &= dc::rebuild_end(n);
  if (!ok) atomicOr(&a.flags[b], T.flag);
}

template <int HK>
void launch(const DecArgs &a, hipStream_t st) {
  const uint32_t ntrees = 4 + a.c.n_steps;
  {
    ProfScope ps("decompress_scatter_kernel", (double)a.L.want * a.m);
    hipLaunchKernelGGL(scatter_kernel<HK>, dim3(a.m), dim3(64), 0, st, a);
  }
  {
    ProfScope ps("decompress_head_kernel", (double)a.L.queries_at * a.m);
    hipLaunchKernelGGL(head_kernel<HK>, dim3((a.m + 63) / 64), dim3(64), 0, st, a);
  }
  if (a.c.n_steps) {
    ProfScope ps("decompress_infer_kernel", (double)a.L.query_bytes * a.m * a.c.num_queries);
    hipLaunchKernelGGL(infer_kernel, dim3(a.m), dim3(64), 0, st, a);
  }
  {
    ProfScope ps("decompress_rebuild_kernel", (double)a.L.query_bytes * a.m * a.c.num_queries);
    hipLaunchKernelGGL(rebuild_kernel<HK>, dim3(a.m * ntrees), dim3(64), 0, st, a);
  }
}

// Both entry points.  reports: the verdicts (p2gpu_verify_batch_compressed); else out and status (p2gpu_proof_decompress_batch).
int run(const p2gpu_circuit *c, const uint8_t *cproofs, const size_t *offsets, size_t batch, p2gpu_verify_report *reports, uint8_t *out, int32_t *status) {
  const vc::CircuitView hv = view_of(c);
  const vc::Layout L = vc::make_layout(hv);
  // ---- the container walk, on the host: only proofs it gets through go to the device ----
  std::vector<uint32_t> reason, tabs;
  std::vector<size_t> slot;  // batch index of device proof i
  if (int rc = cbatch_walk(c, hv, L, cproofs, offsets, batch, reason, slot, tabs)) return rc;
  for (size_t b = 0; b < batch; b++) {
    if (reports) verify_report_fill(&reports[b], vc::Verdict{reason[b], vc::VR_NONE, vc::VR_NONE});
    else {
      status[b] = P2GPU_OK;
      if (reason[b]) {  // the lone call's return code
        size_t n = 0;
        status[b] = p2gpu_proof_decompress(c, cproofs + offsets[b], offsets[b + 1] - offsets[b], nullptr, &n);
      }
    }
  }
  if (out && !L.bad_arity) memset(out, 0, batch * L.want);
  if (slot.size() > UINT32_MAX / (64 * (4 + vc::VC_MAX_STEPS))) {
    set_err("%s: %zu proofs in one call", VB_ENTRY, slot.size());
    return P2GPU_E_ARG;
  }
  if (int rc = ensure_device()) return rc;  // (also when no proof is left for it: never a silent host-only answer)
  const uint32_t m = (uint32_t)slot.size();
  if (m) {
    CallState S;
    hipStream_t st = nullptr;
    if (int rc = vdev::open_device(VB_ENTRY, c, S, &st)) return rc;
    // (the "profile" knob of a prover handle: as in p2gpu_verify_batch)
    p2gpu_circuit *pc = c->device >= 0 ? const_cast<p2gpu_circuit *>(c) : nullptr;
    std::unique_ptr<ProfGuard> prof(pc && pc->profile ? new ProfGuard(pc) : nullptr);
    const size_t nterms = vc::identity_terms(hv), lanes = (size_t)m * hv.num_queries, out_bytes = (size_t)m * L.want;
    std::vector<uint64_t> coff(m + 1, 0);
    for (uint32_t i = 0; i < m; i++) coff[i + 1] = coff[i] + (offsets[slot[i] + 1] - offsets[slot[i]]);
    const size_t cbytes = coff[m];
    DecArgs a;
    a.L = L;
    a.m = m;
    a.tw = dc::table_words(hv);
    a.judge = reports != nullptr;
    uint8_t *d_c = S.alloc<uint8_t>(cbytes + 16);
    uint64_t *d_coff = S.alloc<uint64_t>(m + 1);
    uint32_t *d_tabs = S.alloc<uint32_t>(tabs.size());
    a.out = S.alloc<uint8_t>(out_bytes + 16);
    a.sponge = S.alloc<gl_t>(12 * (size_t)m);
    a.terms = S.alloc<ext_t>(nterms * m);
    a.rec = S.alloc<vc::HeadRecord>(m);
    a.flags = S.alloc<uint32_t>(m);
    a.head_reason = S.alloc<uint32_t>(m);
    if (!d_c || !d_coff || !d_tabs || !a.out || !a.sponge || !a.terms || !a.rec || !a.flags || !a.head_reason)
      return vdev::device_fail(VB_ENTRY, "scratch", hipErrorOutOfMemory);
    a.cbytes = d_c;
    a.coff = d_coff;
    a.tabs = d_tabs;
    if (int rc = vdev::upload_circuit(VB_ENTRY, S, hv, &a.c, st)) return rc;
    VB_TRY(hipMemsetAsync(d_c + cbytes, 0, 16, st), "clear the padding");
    VB_TRY(hipMemsetAsync(a.out + out_bytes, 0, 16, st), "clear the padding");
    VB_TRY(hipMemsetAsync(a.flags, 0, 4 * (size_t)m, st), "clear the flags");
    VB_TRY(hipMemcpyAsync(d_coff, coff.data(), 8 * (size_t)(m + 1), hipMemcpyHostToDevice, st), "copy the offsets");
    VB_TRY(hipMemcpyAsync(d_tabs, tabs.data(), 4 * tabs.size(), hipMemcpyHostToDevice, st), "copy the offset tables");
    // proofs that lie back to back in the caller's buffer go up in one copy
    for (uint32_t i = 0; i < m;) {
      uint32_t j = i + 1;
      while (j < m && slot[j] == slot[j - 1] + 1) j++;
      VB_TRY(hipMemcpyAsync(d_c + coff[i], cproofs + offsets[slot[i]], coff[j] - coff[i], hipMemcpyHostToDevice, st), "copy the proofs");
      i = j;
    }
    if (hv.hasher) launch<1>(a, st);
    else launch<0>(a, st);
    VB_TRY(hipGetLastError(), "launch");
    if (reports) {
      vdev::DevArgs v;
      v.c = a.c;
      v.L = L;
      v.proofs = a.out;
      v.m = m;
      v.sponge = a.sponge;
      v.terms = a.terms;
      v.rec = a.rec;
      v.head_reason = a.head_reason;
      v.cflags = a.flags;
      v.query_reason = S.alloc<uint32_t>(2 * lanes);
      v.verdict = S.alloc<uint32_t>(3 * (size_t)m);
      if (!v.query_reason || !v.verdict) return vdev::device_fail(VB_ENTRY, "scratch", hipErrorOutOfMemory);
      vdev::launch_queries(v, st);
      VB_TRY(hipGetLastError(), "launch");
      std::vector<uint32_t> verdict(3 * (size_t)m);
      VB_TRY(hipMemcpyAsync(verdict.data(), v.verdict, 12 * (size_t)m, hipMemcpyDeviceToHost, st), "read the verdicts");
      VB_TRY(hipStreamSynchronize(st), "verify");
      for (uint32_t i = 0; i < m; i++) {
        const vc::Verdict vd{verdict[3 * (size_t)i], verdict[3 * (size_t)i + 1], verdict[3 * (size_t)i + 2]};
        if (vd.reason >= dc::VR_C_END) {
          set_err("%s: internal error (reason %u)", VB_ENTRY, vd.reason);
          return P2GPU_E_DEVICE;
        }
        verify_report_fill(&reports[slot[i]], vd);
      }
    } else {
      std::vector<uint32_t> flags(m);
      std::vector<uint8_t> bytes(out_bytes);
      VB_TRY(hipMemcpyAsync(flags.data(), a.flags, 4 * (size_t)m, hipMemcpyDeviceToHost, st), "read the flags");
      VB_TRY(hipMemcpyAsync(bytes.data(), a.out, out_bytes, hipMemcpyDeviceToHost, st), "read the proofs");
      VB_TRY(hipStreamSynchronize(st), "decompress");
      for (uint32_t i = 0; i < m; i++) {
        if (flags[i]) status[slot[i]] = P2GPU_E_VERIFY;  // (what decompress returns at every site)
        else memcpy(out + slot[i] * L.want, bytes.data() + (size_t)i * L.want, L.want);
      }
    }
  }
  return 0;
}

}  // namespace

extern "C" int p2gpu_verify_batch_compressed(const p2gpu_circuit *c, const uint8_t *cproofs, const size_t *offsets, size_t batch,
                                             p2gpu_verify_report *reports) try {
  if (int rc = verify_batch_args(c, cproofs, offsets, batch, reports)) return rc;
  if (int rc = run(c, cproofs, offsets, batch, reports, nullptr, nullptr)) return rc;
  return cbatch_finish(batch, reports);
} P2GPU_CATCH

extern "C" int p2gpu_proof_decompress_batch(const p2gpu_circuit *c, const uint8_t *cproofs, const size_t *offsets, size_t batch, uint8_t *out,
                                            int32_t *status) try {
  if (!out) return P2GPU_E_ARG;
  if (int rc = verify_batch_args(c, cproofs, offsets, batch, status)) return rc;
  return run(c, cproofs, offsets, batch, nullptr, out, status);
} P2GPU_CATCH
