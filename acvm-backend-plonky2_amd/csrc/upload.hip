// upload.hip -- the host-witness pipeline of libp2gpu.so: p2gpu_prove (the full wire matrix in host memory) and
// p2gpu_prove_sparse (its dense columns + one value per unused wire) bring the witness across PCIe in column chunks while
// the transforms and the leaf sponge of the chunks that have arrived already run, then hand over to the proof (prover.hip
// prove_impl).  Nothing here touches the transcript.
#include "prover_internal.hpp"
#include <atomic>

using namespace p2;

namespace {

// Host-side look at the witness of the full-matrix entry point (p2gpu_prove): the longest SUFFIX of columns that are
// zero outside `row` -- the wires no gate of the circuit uses, which plonky2's build() leaves at zero except for one random
// value in the PublicInputGate row.  They need not cross PCIe (154 of 234 columns, 161 of 245 MB, for a circuit without
// ECC gates): what p2gpu_prove_sparse lets a caller say, found here by looking.  A few host threads read the columns from
// the last one down and stop at the first column that is dense (a dense witness costs a few cache lines); the scan runs
// while the first chunks (columns below the routed-wire count) are already crossing PCIe.
struct HostScan {
  uint32_t ncols = 0;            // columns [ncols, W) are zero outside `row`
  std::vector<uint64_t> tail;    // their values in `row`
};
void host_scan_suffix(const uint64_t *wires, uint32_t W, size_t n, uint32_t row, uint32_t lo, HostScan *out) {
  // several proofs may be in flight, each with its own scan: a quarter of the CPUs this process may use (the cgroup
  // quota where there is one: the MI355X boxes show 256 hardware threads and grant 16 CPUs), at most 8.  (Round 6 tried
  // twice as many for a scan that finds no other one running: the 154 MB it reads at 2^17 rows take 1.8 ms either way --
  // memory-bound -- and the extra threads cost the pageable upload's staging copy 0.5 ms; gpurun_out/r06_host.)
  static const unsigned T = [] {
    unsigned n = std::thread::hardware_concurrency();
    if (FILE *f = fopen("/sys/fs/cgroup/cpu.max", "r")) {
      long long q = 0, per = 0;
      if (fscanf(f, "%lld %lld", &q, &per) == 2 && q > 0 && per > 0) n = std::min<unsigned>(n, (unsigned)std::max<long long>(1, q / per));
      fclose(f);
    }
    n /= 4;
    return n < 1 ? 1u : (n > 8 ? 8u : n);
  }();
  std::atomic<uint32_t> dense_max{lo};  // columns below this one are not worth looking at any more
  std::vector<uint8_t> sparse(W, 0);
  auto work = [&](unsigned t) {
    for (int64_t j = (int64_t)W - 1 - t; j >= (int64_t)lo; j -= T) {
      if ((uint32_t)j < dense_max.load(std::memory_order_relaxed)) break;
      const uint64_t *p = wires + (size_t)j * n;
      bool zero = true;
      for (size_t b = 0; b < n && zero; b += 2048) {  // 16 KB at a time: early exit on a dense column
        const size_t e = std::min(n, b + 2048);
        uint64_t a0 = 0, a1 = 0, a2 = 0, a3 = 0;
        size_t i = b;
        for (; i + 4 <= e; i += 4) { a0 |= p[i]; a1 |= p[i + 1]; a2 |= p[i + 2]; a3 |= p[i + 3]; }
        for (; i < e; i++) a0 |= p[i];
        uint64_t acc = a0 | a1 | a2 | a3;
        if (acc && row >= b && row < e) {  // the block holding the special row: look again without it
          acc = 0;
          for (size_t k = b; k < e; k++) acc |= (k == row) ? 0 : p[k];
        }
        zero = acc == 0;
      }
      if (zero) sparse[j] = 1;
      else {
        uint32_t cur = dense_max.load(std::memory_order_relaxed);
        while ((uint32_t)j + 1 > cur && !dense_max.compare_exchange_weak(cur, (uint32_t)j + 1, std::memory_order_relaxed)) {}
      }
    }
  };
  std::vector<std::thread> th;
  for (unsigned t = 1; t < T; t++) th.emplace_back(work, t);
  work(0);
  for (auto &x : th) x.join();
  uint32_t nc = W;
  while (nc > lo && sparse[nc - 1]) nc--;
  out->ncols = nc;
  out->tail.resize(W - nc);
  for (uint32_t j = nc; j < W; j++) out->tail[j - nc] = row < n ? wires[(size_t)j * n + row] : 0;
}

// P2GPU_HOST_PRESCAN=0: ship the whole matrix as rounds 1-2 did (for A/B measurements)
bool host_prescan_on() {
  static const bool on = env_flag("P2GPU_HOST_PRESCAN", true);
  return on;
}

}  // namespace

namespace p2 {

// p2gpu_prove (ncols = W) and p2gpu_prove_sparse (ncols < W: the columns >= ncols are zero except in `row`, where
// column j holds tail[j - ncols]; they are written in HBM instead of crossing PCIe)
int prove_host(p2gpu_circuit *c, const uint64_t *wires, uint32_t ncols, const uint64_t *tail, uint32_t row, const uint64_t *pis,
               uint32_t n_pi, uint8_t *proof_out, size_t *proof_len, p2gpu_timings *tm) {
  HIP_TRY(hipSetDevice(c->device));
  // the unused wires of the witness: zeros + one value per column, made on the device (stream-ordered before
  // every consumer below; the host part of the matrix arrives on the copy stream into the columns before them)
  auto make_tail = [&]() -> int {
    if (ncols >= c->W) return 0;
    const uint32_t nt = c->W - ncols;
    gl_t *tv = c->wires_vals.p + (size_t)ncols * c->n;
    HIP_TRY(hipMemsetAsync(tv, 0, 8 * (size_t)nt * c->n, c->stream));
    HIP_TRY(hipMemcpy2DAsync(tv + row, 8 * c->n, tail, 8, 8, nt, hipMemcpyHostToDevice, c->stream));
    return 0;
  };
  // full matrix given: look for the unused-wire suffix on the host while the first chunks upload (see host_scan_suffix).
  // Only where it can pay: the handle still classifies columns (a handle that found a dense witness stopped), and the
  // witness of a sharded proof is split by columns anyway.
  g_hp.mark("host:begin");
  HostScan scan;
  std::thread scan_thread;
  bool scanning = false;
  uint64_t *tail_pinned = nullptr;
  if (ncols == c->W && c->zero_columns && !c->structured_off && c->shard_world == 1 && host_prescan_on() && c->W > c->R) {
    row = c->sparse_row != UINT32_MAX ? c->sparse_row : 0;
    scan_thread = std::thread(host_scan_suffix, wires, c->W, c->n, row, c->R, &scan);
    scanning = true;
  }
  struct Joiner {  // never leave the function with the scan still running
    std::thread &t;
    ~Joiner() { if (t.joinable()) t.join(); }
  } joiner{scan_thread};
  if (int rc = make_tail()) return rc;
  // (Round 6 tried ONE bulk upload + the resident path whenever other proofs are in flight on the device -- their kernels fill
  // the chip anyway: 192 proofs/s against 205 with the chunks, same box, four in flight, pageable witness: the staging copy of
  // 84 MB then sits on the calling thread in one piece in front of the proof instead of under its own transforms.  Removed.)
  // The witness crosses PCIe in column chunks on a copy stream; the inverse transform and the
  // LDE of a chunk run while the next chunk is still in flight (values -> coefficients -> LDE are
  // per-column; only the leaf hash needs every column).
  // The leaf hash is a sponge over the columns in order, 17 per permutation: the rate blocks of the
  // columns that have arrived are absorbed chunk by chunk too (states wait in HBM), so that after
  // the last chunk only its own two permutations and the tree remain.
  const double t0 = now_ms();
  // rate blocks (17 columns) per upload chunk; the override is for measurements (scratch/chunk_sweep.sh, 2^20 rows, round 3 with the
  // host scan shipping 80 columns: 2 blocks 6.85-7.2 ms lone / 202-203 proofs/s in flight, 3: 7.75-8.05 / 206, 4: 7.5 / 186, 5: 9.6-10 / 203)
  static const uint64_t chunk_blocks = env_uint("P2GPU_CHUNK_BLOCKS", 2);
  const uint32_t W = c->W, chunk = 17 * (uint32_t)(chunk_blocks >= 1 && chunk_blocks <= 64 ? chunk_blocks : 2);  // two rate blocks
  const size_t n = c->n;
  if (c->shard_world > 1 && ncols < c->W) {
    // sharded proof from the compact witness: every rank uploads the dense columns itself (they are what is left
    // of the matrix once the unused wires are made on the device); no exchange
    HIP_TRY(hipMemcpyAsync(c->wires_vals.p, wires, 8 * (size_t)ncols * n, hipMemcpyHostToDevice, c->stream));
    return prove_impl(c, c->wires_vals.p, pis, n_pi, proof_out, proof_len, tm, now_ms() - t0);
  }
  if (c->shard_world > 1) {
    // Sharded proof, witness in host memory: a rank pulls only ITS block of columns
    // [q * cpr, (q + 1) * cpr) across its own PCIe link -- W / G columns, 31 MB instead of 245 MB at d = 17 and
    // G = 8 -- and the blocks are exchanged GPU to GPU with one in-place all-gather (xGMI on a real node).
    // The inverse transform then runs replicated on every rank: at 0.5 ms it is cheaper than a second
    // exchange of the same 245 MB as coefficients would be.
    const uint32_t G = (uint32_t)c->shard_world, q = (uint32_t)c->shard_rank, cpr = (W + G - 1) / G;
    if (c->wires_vals.count < (size_t)G * cpr * n) {
      HIP_TRY(hipStreamSynchronize(c->stream));
      c->wires_vals.release();
      HIP_TRY(c->wires_vals.alloc((size_t)G * cpr * n));
    }
    const uint32_t c0 = std::min(q * cpr, W), c1 = std::min((q + 1) * cpr, W);
    if (c1 > c0)
      HIP_TRY(hipMemcpyAsync(c->wires_vals.p + (size_t)c0 * n, wires + (size_t)c0 * n, 8 * (size_t)(c1 - c0) * n, hipMemcpyHostToDevice,
                             c->stream));
    {
      // (the exchange belongs to the proof's profile like the ones inside prove_impl: `profile` = 2 counts it)
      ProfGuard xprof(c);
      if (int rc = shard_allgather(c, c->wires_vals.p + (size_t)q * cpr * n, c->wires_vals.p, 8 * (size_t)cpr * n)) return rc;
    }
    return prove_impl(c, c->wires_vals.p, pis, n_pi, proof_out, proof_len, tm, now_ms() - t0);
  }
  const gl_t ninv = gl_inv((gl_t)n);
  Batch &b = c->wires;
  // (also implies a hashed leaf: more than 3 columns); the chunk-wise sponge is the Keccak one (17-column rate blocks)
  const bool incremental = W > chunk && c->hasher == 0;
  if (incremental && c->hash_state.count < (size_t)b.ncl * 25 * n) {  // also after set_shard(world 1 again): more local cosets
    c->hash_state.release();
    HIP_TRY(c->hash_state.alloc((size_t)b.ncl * 25 * n));
  }
  const uint32_t full_blocks = W / 17;
  uint32_t ci = 0;
  for (uint32_t col0 = 0, nc = 0; col0 < W; col0 += nc, ci++) {
    if (scanning && col0 + chunk > c->R) {
      // the first chunk that reaches beyond the routed wires: the host scan decides what is left to upload.  Columns
      // already enqueued stay as they are (ncols never drops below col0)
      g_hp.mark("host:enq");
      scan_thread.join();
      g_hp.mark("host:WAIT(scan)");
      scanning = false;
      if (scan.ncols < W) {
        ncols = std::max(scan.ncols, col0);
        // the 2-D copy below is asynchronous: its source must outlive this frame AND prove_impl's reset of the pinned arena
        if (!c->tail_stage) HIP_TRY(hipHostMalloc((void **)&c->tail_stage, 8 * (size_t)W, hipHostMallocDefault));
        tail_pinned = c->tail_stage;
        memcpy(tail_pinned, scan.tail.data() + (ncols - scan.ncols), 8 * (size_t)(W - ncols));
        tail = tail_pinned;
        if (int rc = make_tail()) return rc;
      }
    }
    // the chunk that holds the last column coming from the host also takes every column behind it (they are already
    // in HBM: nothing to wait for, and each extra absorb launch is a round trip of the 200 B sponge state per row)
    nc = col0 + chunk >= ncols ? W - col0 : chunk;
    if (ci >= c->copy_events.size()) {
      hipEvent_t e;
      HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
      c->copy_events.push_back(e);
    }
    gl_t *vals = c->wires_vals.p + (size_t)col0 * n;
    const uint32_t nh = col0 < ncols ? std::min(nc, ncols - col0) : 0;  // columns of this chunk that come from the host
    if (nh) {
      g_hp.mark("host:enq");
      HIP_TRY(hipMemcpyAsync(vals, wires + (size_t)col0 * n, 8 * (size_t)nh * n, hipMemcpyHostToDevice, c->copy_stream));
      g_hp.mark("host:h2d");
      HIP_TRY(hipEventRecord(c->copy_events[ci], c->copy_stream));
      HIP_TRY(hipStreamWaitEvent(c->stream, c->copy_events[ci], 0));
    }
    const uint32_t *nz = batch_colnz(c, b) ? c->wire_nz.p + col0 : nullptr;
    uint32_t *cl = nz ? c->wire_clean.p + col0 : nullptr;
    if (nz) {
      column_flags(c->stream, vals, nc, c->d, c->sparse_rows, c->wire_nz.p + col0, c->wire_scalar.p + col0, c->W);
      column_clean_update(c->stream, nz, nc, cl, false);
    }
    const ColHints hi = nz ? wire_hints(c, col0, false) : ColHints(), hl = nz ? wire_hints(c, col0, true) : ColHints();
    ntt_batch(c->stream, c->plan_inv, vals, b.coeffs.p + (size_t)col0 * n, nc, 1, nullptr, ninv, false, CosetMap(), 0,
              nz ? &hi : nullptr);
    ntt_batch(c->stream, c->plan_fwd, b.coeffs.p + (size_t)col0 * n, b.lde.p + (size_t)col0 * n, nc, b.ncl, c->scale.p, 1,
              false, b.cm, W, nz ? &hl : nullptr);
    if (nz) column_clean_update(c->stream, nz, nc, cl, true);
    if (incremental) {
      const bool last = col0 + nc >= W;
      const uint32_t blk0 = col0 / 17;
      const uint32_t nblk = last ? full_blocks - blk0 : chunk / 17;
      const VirtCols v = batch_virt(c, b);
      hash_lde_absorb(c->stream, b.lde.p, W, c->d, b.ncl, blk0, nblk, col0 == 0, last, c->hash_state.p, b.dig.p, &v);
    }
  }
  const double h2d = now_ms() - t0;  // host time spent feeding PCIe (the transforms overlap with it)
  c->wires_ntt_done = true;
  c->wires_hash_done = incremental;
  int rc = prove_impl(c, c->wires_vals.p, pis, n_pi, proof_out, proof_len, tm, h2d);
  c->wires_ntt_done = false;
  c->wires_hash_done = false;
  return rc;
}

}  // namespace p2
