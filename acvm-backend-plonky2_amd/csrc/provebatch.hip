// provebatch.hip -- p2gpu_prove_batch_dev / p2gpu_prove_seeds_batch: the proofs of a batch of witnesses of one small circuit
// (degree_bits <= P2GPU_PROVE_BATCH_MAX_DEGREE_BITS) in one fixed sequence of launches per slab of proofs.
//
// The bodies and their order are provebatchcore.hpp's (pb::prove_slab); this file launches them as kernels -- one generic
// kernel per body shape, the body its template argument --, owns the slab's buffers on the handle and answers for the arguments.
//   lanes<F>   one lane per item (an LDE row, a coefficient, an opening, a proof for the transcript steps)
//   blocks<F>  one workgroup per item with 2^lg words of LDS twice over: a column's transforms, a cap subtree, a scan, the
//              windows of a proof-of-work search
// Per slab the host enqueues the public inputs, the launches and the copy of the proof bytes and statuses, then synchronises
// once.  Nothing of prover.hip's proof runs here and nothing there changes: the lone path stays what it was, byte for byte,
// and this path writes the same bytes (tests/test_gpu_prove_batch.py; tests/provebatch_check.cpp runs the same sequence
// on the host against the CPU prover of the tests).
#include "hostproof.hpp"
#include "prover_internal.hpp"
#include "provebatchcore.hpp"
#include "witplan.hpp"

using namespace p2;

namespace {

const char *const ENTRY = "p2gpu_prove_batch_dev";

// what a slab of proofs may take of the device's memory, free memory allowing (knob "prove_batch_slab" overrides the count)
constexpr size_t SLAB_BUDGET_BYTES = (size_t)8 << 30;
constexpr uint32_t SLAB_MAX_PROOFS = 1024;

template <void (*F)(const pb::Args &, uint32_t)>
__global__ __launch_bounds__(256) void pb_lanes_kernel(const pb::Args a, uint32_t total) {
  const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g < total) F(a, g);
}
template <void (*F)(const pb::Args &, uint32_t, uint32_t, uint32_t, gl_t *)>
__global__ __launch_bounds__(256) void pb_blocks_kernel(const pb::Args a) {
  extern __shared__ gl_t pb_lds[];
  F(a, blockIdx.x, threadIdx.x, blockDim.x, pb_lds);
}

struct DeviceRun {
  hipStream_t st;
  uint32_t launches = 0;
  uint32_t pow_groups() const { return pb::POW_GROUPS; }
  uint32_t pow_threads() const { return pb::POW_THREADS; }
  template <void (*F)(const pb::Args &, uint32_t)>
  void lanes(const pb::Args &a, size_t total, const char *name) {
    ProfScope ps(name, 0);
    const uint32_t threads = total <= 16384 ? 64 : 256;  // few items (a lane per proof): spread them over the compute units
    hipLaunchKernelGGL((pb_lanes_kernel<F>), dim3((uint32_t)((total + threads - 1) / threads)), dim3(threads), 0, st, a, (uint32_t)total);
    launches++;
  }
  template <void (*F)(const pb::Args &, uint32_t, uint32_t, uint32_t, gl_t *)>
  void blocks(const pb::Args &a, size_t nblocks, uint32_t threads, size_t lds_words, const char *name) {
    ProfScope ps(name, 0);
    hipLaunchKernelGGL((pb_blocks_kernel<F>), dim3((uint32_t)nblocks), dim3(threads), 8 * lds_words, st, a);
    launches++;
  }
};

// the slab's buffers, kept on the handle (CircuitState::prove_batch): one device arena, grown to the largest slab seen
struct State {
  void *arena = nullptr;
  size_t arena_bytes = 0;
  uint32_t last_launches = 0, last_slab = 0;
};

struct Counting {
  size_t bytes = 0;
  void *operator()(size_t b) {
    bytes += (b + 255) & ~(size_t)255;
    return (void *)(uintptr_t)256;  // (any non-null pointer: only the sizes matter)
  }
};
struct Bump {
  uint8_t *base;
  size_t used = 0, cap;
  void *operator()(size_t b) {
    const size_t at = used;
    used += (b + 255) & ~(size_t)255;
    return used <= cap ? base + at : nullptr;
  }
};

// everything of pb::Args that does not depend on the slab
pb::Args circuit_args(const p2gpu_circuit *c) {
  pb::Args a;
  memset(&a, 0, sizeof a);
  a.c = view_of(c);
  a.L = vc::make_layout(a.c);
  a.c.gates = c->d_gates.p;
  a.c.k_is = c->d_kis.p;
  a.c.prc = c->d_prc_hash.p;
  a.c.cs_cap = nullptr;
  a.nterms = a.c.K + a.c.K * a.c.nchunks + a.c.max_gate_constraints;
  a.self_check = c->self_check ? 1 : 0;
  a.dh = c->d;
  a.tw_fwd = c->tw_fwd.p; a.tw_inv = c->tw_inv.p; a.scale = c->scale.p; a.inv_scale = c->inv_scale.p;
  a.sigmas = c->d_sigmas.p;
  a.cs_coef = c->cs.coeffs.p; a.cs_lde = c->cs.lde.p; a.cs_dig = c->cs.dig.p;
  for (size_t l = 0; l < c->cs.level_off.size() && l < pb::MAX_TREE_LEVELS; l++) a.cs_level_off[l] = c->cs.level_off[l];
  return a;
}

size_t slab_bytes(const pb::Args &base, uint32_t B) {
  pb::Args a = base;
  Counting cnt;
  pb::slab_buffers(a, B, cnt);
  return cnt.bytes;
}

// the arguments of p2gpu_prove_batch_dev, in the order the header gives; no device call
int batch_args(const p2gpu_circuit *c, const void *wires_dev, size_t batch, const uint64_t *pis, uint32_t n_pi, const void *proofs_out,
               const void *status) {
  if (!c || !wires_dev || !proofs_out || !status) {
    set_err("%s: a null %s", ENTRY, !c ? "handle" : !wires_dev ? "witness matrix" : !proofs_out ? "proof buffer" : "status array");
    return P2GPU_E_ARG;
  }
  if (batch == 0) {
    set_err("%s: batch == 0", ENTRY);
    return P2GPU_E_ARG;
  }
  if (n_pi != c->num_pi || (n_pi && !pis)) {
    set_err("%s: expected %u public inputs per witness, got %u", ENTRY, c->num_pi, n_pi);
    return P2GPU_E_ARG;
  }
  for (size_t b = 0; b < batch; b++)
    for (uint32_t i = 0; i < n_pi; i++)
      if (pis[b * n_pi + i] >= GL_P) {
        set_err("%s: witness %zu of the batch: public input %u is not a canonical field element", ENTRY, b, i);
        return P2GPU_E_ARG;
      }
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty() || c->peer || sharded(c) || c->shard_world > 1 || c->shard_fn || c->rccl_comm) {
    set_err("%s: a plain handle is needed, not a device group or a handle with sharding configured", ENTRY);
    return P2GPU_E_ARG;
  }
  if (c->d > P2GPU_PROVE_BATCH_MAX_DEGREE_BITS || c->nchunks > pb::MAX_CHUNKS) {
    set_err("%s: degree_bits %u is above the limit P2GPU_PROVE_BATCH_MAX_DEGREE_BITS = %u of the batched prover (%u chunks of routed wires, at most %u): "
            "prove each witness with p2gpu_prove_dev",
            ENTRY, c->d, (unsigned)P2GPU_PROVE_BATCH_MAX_DEGREE_BITS, c->nchunks, pb::MAX_CHUNKS);
    return P2GPU_E_ARG;
  }
  return 0;
}

const char *status_words(int st) {
  switch (st) {
  case P2GPU_E_UNSATISFIED: return "witness does not satisfy the circuit: the plonk identity fails at zeta (vanishing != Z_H * quotient)";
  case P2GPU_E_OPENING_IN_SUBGROUP: return "Opening point is in the subgroup.";
  }
  return "internal error (proof of work)";
}

int prove_batch_impl(p2gpu_circuit *c, const gl_t *wires_dev, size_t batch, const uint64_t *pis, uint32_t n_pi, uint8_t *proofs_out, int *status) {
  HIP_TRY(hipSetDevice(c->device));
  ProfGuard prof(c);
  const pb::Args base = circuit_args(c);
  const vc::Layout &L = base.L;
  if (!c->prove_batch) c->prove_batch = new State();
  State *S = (State *)c->prove_batch;
  // the slab: the knob's count, or what the budget and the free memory hold
  const size_t per_proof = slab_bytes(base, 1);
  size_t slab = c->prove_batch_slab;
  if (!slab) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    const size_t usable = std::min(SLAB_BUDGET_BYTES, (free_b + S->arena_bytes) / 4 * 3);
    slab = std::max<size_t>(1, usable / per_proof);
  }
  slab = std::min({slab, batch, (size_t)SLAB_MAX_PROOFS, ((size_t)1 << 30) >> L.lgN});
  if (!slab) slab = 1;
  const size_t need = slab_bytes(base, (uint32_t)slab);
  if (need > S->arena_bytes) {
    if (S->arena) (void)hipFree(S->arena);
    S->arena = nullptr;
    S->arena_bytes = 0;
    const hipError_t e = hipMalloc(&S->arena, need);
    if (e != hipSuccess) {
      (void)hipGetLastError();
      set_err("%s: %zu bytes for a slab of %zu proofs: %s", ENTRY, need, slab, hipGetErrorString(e));
      return P2GPU_E_DEVICE;
    }
    S->arena_bytes = need;
  }
  const size_t want = L.want, matrix = (size_t)c->W * c->n;
  std::vector<int32_t> st_host(slab);
  for (size_t b0 = 0; b0 < batch; b0 += slab) {
    const uint32_t B = (uint32_t)std::min(slab, batch - b0);
    pb::Args a = base;
    Bump bump{(uint8_t *)S->arena, 0, S->arena_bytes};
    if (!pb::slab_buffers(a, B, bump)) {
      set_err("%s: internal error (slab arena)", ENTRY);
      return P2GPU_E_DEVICE;
    }
    a.wires = wires_dev + b0 * matrix;
    if (n_pi) HIP_TRY(hipMemcpyAsync((void *)a.pis, pis + b0 * n_pi, 8 * (size_t)B * n_pi, hipMemcpyHostToDevice, c->stream));
    DeviceRun run{c->stream};
    if (c->hasher) pb::prove_slab<1>(run, a);
    else pb::prove_slab<0>(run, a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy2DAsync(proofs_out + b0 * want, want, a.proofs, a.want8, want, B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpy2DAsync(st_host.data(), 4, &a.rec[0].status, sizeof(pb::Record), 4, B, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (uint32_t b = 0; b < B; b++) status[b0 + b] = st_host[b];
    S->last_launches = run.launches;
    S->last_slab = B;
  }
  if (c->profile && c->pending.size() > 16384) flush_kstats(c);
  int rc = P2GPU_OK;
  for (size_t b = batch; b-- > 0;)
    if (status[b] != P2GPU_OK) {
      memset(proofs_out + b * want, 0, want);
      rc = status[b];
      set_err("witness %zu of the batch: %s", b, status_words(rc));
    }
  return rc;
}

}  // namespace

namespace p2 {

void prove_batch_release(p2gpu_circuit *c) {
  State *S = (State *)c->prove_batch;
  if (!S) return;
  if (S->arena) (void)hipFree(S->arena);
  delete S;
  c->prove_batch = nullptr;
}

}  // namespace p2

extern "C" {

uint32_t p2gpu_prove_batch_max_degree_bits(void) { return pb::MAX_DEGREE_BITS; }

int p2gpu_prove_batch_info(const p2gpu_circuit *c, uint64_t out[4]) {
  if (!c || !out) return P2GPU_E_ARG;
  const State *S = c->device >= 0 ? (const State *)c->prove_batch : nullptr;
  out[0] = S ? S->last_launches : 0;
  out[1] = S ? S->last_slab : 0;
  out[2] = S ? S->arena_bytes : 0;
  out[3] = SLAB_BUDGET_BYTES;
  return P2GPU_OK;
}

int p2gpu_prove_batch_dev(p2gpu_circuit *c, const uint64_t *wires_dev, size_t batch, const uint64_t *pis, uint32_t n_pi, uint8_t *proofs_out,
                          int *status) try {
  if (int rc = batch_args(c, wires_dev, batch, pis, n_pi, proofs_out, status)) return rc;
  return prove_batch_impl(c, wires_dev, batch, pis, n_pi, proofs_out, status);
} P2GPU_CATCH

int p2gpu_prove_seeds_batch(p2gpu_witness_plan *p, const uint64_t *seed_values, size_t batch, const uint64_t *pis, uint32_t n_pi,
                            uint8_t *proofs_out, int *status, uint32_t *bad_cells) try {
  if (!p || (p->n_seeds && !seed_values)) {
    set_err("p2gpu_prove_seeds_batch: a null %s", !p ? "plan" : "seed array");
    return P2GPU_E_ARG;
  }
  p2gpu_circuit *c = p->c;  // (a plan exists on a plain prover handle only)
  // (the matrix is the plan's own: any non-null pointer stands in for it while the arguments are looked at)
  if (int rc = batch_args(c, p, batch, pis, n_pi, proofs_out, status)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t matrix = (size_t)c->W * c->n, want = vc::make_layout(view_of(c)).want;
  if (p->batch_wires.count < batch * matrix) {
    p->batch_wires.release();
    HIP_TRY(p->batch_wires.alloc(batch * matrix));
  }
  gl_t *wires = p->batch_wires.p;
  const int walk = p2gpu_generate_witness_batch(p, seed_values, batch, wires, status, bad_cells);
  if (walk != P2GPU_OK && walk != P2GPU_E_UNSATISFIED) return walk;
  const std::string walk_words = walk ? p2gpu_last_error() : "";
  // the members the walk accepted, moved to the front of the buffer in their order
  std::vector<size_t> good;
  for (size_t b = 0; b < batch; b++)
    if (status[b] == P2GPU_OK) good.push_back(b);
  std::vector<uint64_t> gpis(good.size() * n_pi);
  for (size_t i = 0; i < good.size(); i++) {
    if (good[i] != i) HIP_TRY(hipMemcpyAsync(wires + i * matrix, wires + good[i] * matrix, 8 * matrix, hipMemcpyDeviceToDevice, c->stream));
    if (n_pi) memcpy(&gpis[i * n_pi], pis + good[i] * n_pi, 8 * (size_t)n_pi);
  }
  memset(proofs_out, 0, batch * want);
  int rc = P2GPU_OK;
  size_t first_bad = batch;
  std::string words;
  if (!good.empty()) {
    std::vector<uint8_t> proofs(good.size() * want);
    std::vector<int> st(good.size());
    rc = prove_batch_impl(c, wires, good.size(), gpis.data(), n_pi, proofs.data(), st.data());
    if (rc != P2GPU_OK && rc != P2GPU_E_UNSATISFIED && rc != P2GPU_E_OPENING_IN_SUBGROUP) return rc;
    for (size_t i = 0; i < good.size(); i++) {
      status[good[i]] = st[i];
      memcpy(proofs_out + good[i] * want, &proofs[i * want], want);
      if (st[i] != P2GPU_OK && first_bad == batch) {
        first_bad = good[i];
        words = status_words(st[i]);
      }
    }
  }
  // the lowest failing member speaks, whichever stage refused it
  for (size_t b = 0; b < batch; b++)
    if (status[b] != P2GPU_OK) {
      if (b == first_bad) set_err("witness %zu of the batch: %s", b, words.c_str());
      else last_error_restore(walk_words);
      return status[b];
    }
  return P2GPU_OK;
} P2GPU_CATCH

}  // extern "C"
