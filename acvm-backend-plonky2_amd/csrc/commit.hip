// commit.hip -- the commitment operators of libp2gpu.so: values / coefficients / LDE of a polynomial batch -> leaf digests ->
// Merkle tree -> cap on the host (plonky2 0.2.2 fri/oracle.rs PolynomialBatch::from_values / from_coeffs,
// hash/merkle_tree.rs), the classes of the wire columns that go with them, and the transcript's sync point.  Called by the
// proof (prover.hip), by the upload pipeline of a host witness (upload.hip) and by the stage-level operators of handle.hip.
#include "prover_internal.hpp"

using namespace p2;

namespace {

// leaf digests of a batch (+ the first two tree levels when the layout has them: the return value)
uint32_t leaf_hash(p2gpu_circuit *c, Batch &b, const VirtCols &v) {
  const bool two = b.level_off.size() >= 3;  // levels with n/2 and n/4 nodes per coset exist
  return hash_lde_leaves(c->stream, b.lde.p, b.cols, c->d, b.ncl, b.dig.p, hprc(c), &v, two ? b.dig.p + b.level_off[1] : nullptr,
                         two ? b.dig.p + b.level_off[2] : nullptr);
}

// hash + tree of a batch whose LDE is already in place
int batch_commit_from_lde(p2gpu_circuit *c, Batch &b) {
  const VirtCols v = batch_virt(c, b);
  const uint32_t lv = leaf_hash(c, b, v);
  TRACE(c, "  leaf hash");
  return tree_build(c, b, c->n, lv);
}

}  // namespace

namespace p2 {

int pin_exhausted() {
  set_err("internal: pinned staging arena exhausted");
  return P2GPU_E_DEVICE;
}

// device copy of the Poseidon round constants when the circuit's hasher is PoseidonHash, nullptr for Keccak
const gl_t *hprc(const p2gpu_circuit *c) { return c->hasher == 1 ? c->d_prc_hash.p : nullptr; }

// The transcript sync points of a proof.  Default: hipStreamSynchronize, which spins on the host (lowest latency: the
// eleven round trips of a lone proof).  Knob "blocking_sync" = 1: record an event created with hipEventBlockingSync and
// sleep on it instead -- a woken thread costs ~10-30 us more per round trip, but a process with several proofs in
// flight no longer burns one CPU per host thread while the GPU works (4 spinning threads per GPU are 32 CPUs on an
// 8-GPU node: more than the 16-CPU cgroup quota of the MI355X boxes, where the spinning would throttle the ranks).
int wait_stream(p2gpu_circuit *c) {
  if (!c->blocking_sync) {
    HIP_TRY(hipStreamSynchronize(c->stream));
    return 0;
  }
  if (!c->sync_event) HIP_TRY(hipEventCreateWithFlags(&c->sync_event, hipEventBlockingSync | hipEventDisableTiming));
  HIP_TRY(hipEventRecord(c->sync_event, c->stream));
  HIP_TRY(hipEventSynchronize(c->sync_event));
  return 0;
}

// level offsets of a tree over [cosets][m0] leaf digests reduced to cap_per nodes per coset
void tree_layout(Batch &b, uint32_t cosets, size_t m0, size_t cap_per) {
  b.level_off.clear();
  size_t off = 0;
  for (size_t m = m0;; m >>= 1) {
    b.level_off.push_back(off);
    off += (size_t)cosets * m;
    if (m <= cap_per) break;
  }
}

// allocate tree storage for [C][m0] leaf digests reduced to cap_per nodes per coset
int tree_alloc(Batch &b, uint32_t C, size_t m0, size_t cap_per) {
  tree_layout(b, C, m0, cap_per);
  // the last level holds C * cap_per digests (or C * m0 when the leaves already are the cap)
  size_t last_m = m0;
  while (last_m > cap_per) last_m >>= 1;
  const size_t total = b.level_off.back() + (size_t)C * last_m;
  b.ncl = C;
  HIP_TRY(b.dig.alloc(total));
  return 0;
}

// levels_done: tree levels above the leaf digests that are in place already (the leaf-hash launch builds two: merkle.hip)
int tree_build(p2gpu_circuit *c, Batch &b, size_t m0, uint32_t levels_done) {
  const uint32_t C = c->C, CL = b.ncl;
  const size_t m = m0 >> levels_done;
  const size_t cap_target = ((size_t)1 << c->cap_h) >> c->rate_bits;
  const size_t cap_per = std::min(m, cap_target);  // (leaves fewer than the cap: they are the cap)
  // a tree every rank holds completely (constants/sigmas, FRI steps >= 1) needs no exchange -- except in
  // the one-rank plumbing test, where every tree goes through the transport
  const bool local = CL == C && !(c->shard_world == 1 && sharded(c));
  // the kernel that computes the cap level stores it in page-locked host memory as well when it can (tree_levels): no
  // copy kernel between the last level and the transcript's sync
  dig_t *mirror = local && m0 > cap_target ? c->pin.take<dig_t>(C * cap_target) : nullptr;
  const bool mirrored = tree_levels(c->stream, b.dig.p + b.level_off[levels_done], CL, (uint32_t)m, (uint32_t)cap_target, hprc(c), mirror);
  dig_t *raw = mirrored ? mirror : c->pin.take<dig_t>(C * cap_per);  // [global coset][cap_per]; pinned: the D2H below is a true async copy
  if (!raw) return pin_exhausted();
  if (local) {
    if (!mirrored)
      HIP_TRY(hipMemcpyAsync(raw, b.dig.p + b.level_off.back(), C * cap_per * sizeof(dig_t), hipMemcpyDeviceToHost,
                             c->stream));
    g_hp.mark("enq(cap)");
    if (int rc_ = wait_stream(c)) return rc_;
    g_hp.mark("WAIT(cap)");
  } else {
    // coset r owns whole cap subtrees: exchange the CL * cap_per local roots (the path's only
    // commitment-time collective: 16 x 25 B in total)
    const size_t bytes = (size_t)CL * cap_per * sizeof(dig_t);
    if (int rc = shard_allgather(c, b.dig.p + b.level_off.back(), c->xchg_recv.p, bytes)) return rc;
    dig_t *all = c->pin.take<dig_t>((size_t)c->shard_world * CL * cap_per);
    if (!all) return pin_exhausted();
    HIP_TRY(hipMemcpyAsync(all, c->xchg_recv.p, (size_t)c->shard_world * CL * cap_per * sizeof(dig_t), hipMemcpyDeviceToHost, c->stream));
    if (int rc_ = wait_stream(c)) return rc_;
    shard_assemble_cap(c->shard_world, c->rate_bits, cap_per, all, b.cap);
    return 0;
  }
  shard_assemble_cap(1, c->rate_bits, cap_per, raw, b.cap);
  return 0;
}

// the column classes of a batch: only the wires have them (valid for the proof in progress)
const uint32_t *batch_colnz(const p2gpu_circuit *c, const Batch &b) {
  return (&b == &c->wires && c->zero_columns && !c->structured_off && c->wire_nz.p) ? c->wire_nz.p : nullptr;
}

// First wire column whose LDE is not materialised when it is structured (class 0 / 1): no gate reads a wire >=
// gate_wires and the permutation argument stops at R, so the only readers of those LDE columns are the leaf hash
// and the query gather, which recompute val * LDE(unit column) instead (VirtCols).  UINT32_MAX: off.
uint32_t virt_first(const p2gpu_circuit *c) {
  if (!c->virtual_columns || !batch_colnz(c, c->wires)) return UINT32_MAX;
  const uint32_t f = std::max(c->R, c->gate_wires);
  return f < c->W ? f : UINT32_MAX;
}

// hints for the transforms of the wire columns [col0, ...): lde = false: values -> coefficients, true: the LDE
ColHints wire_hints(const p2gpu_circuit *c, uint32_t col0, bool lde) {
  ColHints h;
  h.cls = c->wire_nz.p + col0;
  h.clean = c->wire_clean.p + col0;
  h.val = c->wire_scalar.p + col0;
  h.basis = lde ? c->sparse_lde.p : c->sparse_coeffs.p;
  h.basis_per_coset = lde;
  h.nrows = c->sparse_rows.count;
  h.val_stride = c->W;
  h.basis_stride = lde ? (size_t)c->C * c->n : c->n;
  const uint32_t vf = virt_first(c);
  if (lde && vf != UINT32_MAX) h.virt_first = vf > col0 ? vf - col0 : 0;
  h.dense_hint = col0 == 0 ? c->last_dense : 0;
  return h;
}

// the unmaterialised columns of batch b for its leaf hash (only the wires have any)
VirtCols batch_virt(const p2gpu_circuit *c, const Batch &b) {
  VirtCols v;
  const uint32_t vf = &b == &c->wires ? virt_first(c) : UINT32_MAX;
  if (vf == UINT32_MAX) return v;
  v.cls = c->wire_nz.p;
  v.val = c->wire_scalar.p;
  v.basis = c->sparse_lde.p;
  v.first = vf;
  v.coset_first = b.cm.first;
  v.coset_stride = b.cm.stride;
  return v;
}

// coefficients (bit-reversed storage) -> LDE on the 2^rate_bits cosets -> leaf digests -> tree
int batch_commit_from_coeffs(p2gpu_circuit *c, Batch &b) {
  const uint32_t *nz = batch_colnz(c, b);
  const ColHints h = nz ? wire_hints(c, 0, true) : ColHints();
  ntt_batch(c->stream, c->plan_fwd, b.coeffs.p, b.lde.p, b.cols, b.ncl, c->scale.p, 1, false, b.cm, 0, nz ? &h : nullptr);
  if (nz) column_clean_update(c->stream, nz, b.cols, c->wire_clean.p, true);
  const VirtCols v = batch_virt(c, b);
  const uint32_t lv = leaf_hash(c, b, v);
  TRACE(c, "  lde + leaf hash");
  return tree_build(c, b, c->n, lv);
}

// values -> coefficients (inverse transform), then as above; the wires of a host witness arrive with their transforms
// (and, when hashed chunk by chunk, their leaf digests) already enqueued by upload.hip
int batch_commit_from_values(p2gpu_circuit *c, Batch &b, const gl_t *vals_dev) {
  if (&b == &c->wires && c->wires_ntt_done) return c->wires_hash_done ? tree_build(c, b, c->n) : batch_commit_from_lde(c, b);
  // unused wires are zero in every row (wires 80..233 of the 234-wire configuration in circuits without ECC
  // gates): one pass over the witness finds them, and their inverse transform and LDE become stores of zeros
  const uint32_t *nz = batch_colnz(c, b);
  if (nz) {
    column_flags(c->stream, vals_dev, b.cols, c->d, c->sparse_rows, c->wire_nz.p, c->wire_scalar.p, c->W);
    column_clean_update(c->stream, nz, b.cols, c->wire_clean.p, false);
  }
  const gl_t ninv = gl_inv((gl_t)c->n);
  const ColHints h = nz ? wire_hints(c, 0, false) : ColHints();
  if (c->shard_intt && sharded(c)) {
    // SURVEY 8(e) steps 1-2 (knob "shard_intt"): rank q transforms only ITS block of the dense columns and the coefficient
    // blocks are all-gathered in place; structured columns are written locally on every rank (no exchange for them).
    // The ranks agree on the blocks without talking: the witness is replicated, so the column classes are too.
    const uint32_t G = (uint32_t)c->shard_world, q = (uint32_t)c->shard_rank, cols = b.cols;
    std::vector<uint32_t> dense;
    dense.reserve(cols);
    if (nz) {
      uint32_t *hc = c->pin.take<uint32_t>(cols);
      if (!hc) return pin_exhausted();
      HIP_TRY(hipMemcpyAsync(hc, nz, 4 * (size_t)cols, hipMemcpyDeviceToHost, c->stream));
      if (int rc_ = wait_stream(c)) return rc_;
      for (uint32_t j = 0; j < cols; j++)
        if (hc[j] == 2u) dense.push_back(j);
    } else {
      for (uint32_t j = 0; j < cols; j++) dense.push_back(j);
    }
    uint32_t lo[8], hi[8];
    size_t off[8], sz[8];
    intt_blocks(dense.data(), (uint32_t)dense.size(), G, lo, hi);
    for (uint32_t p = 0; p < G; p++) {
      off[p] = 8 * (size_t)lo[p] * c->n;
      sz[p] = 8 * (size_t)(hi[p] - lo[p]) * c->n;
    }
    auto part = [&](uint32_t c0, uint32_t c1, bool fill_only) {
      if (c1 <= c0 || (fill_only && !nz)) return;
      ColHints hp = nz ? wire_hints(c, c0, false) : ColHints();
      hp.fill_only = fill_only;
      hp.dense_hint = 0;
      ntt_batch(c->stream, c->plan_inv, vals_dev + (size_t)c0 * c->n, b.coeffs.p + (size_t)c0 * c->n, c1 - c0, 1, nullptr, ninv, false,
                CosetMap(), 0, nz ? &hp : nullptr);
    };
    if (hi[q] > lo[q]) {
      part(0, lo[q], true);
      part(lo[q], hi[q], false);
      part(hi[q], cols, true);
    } else {
      part(0, cols, true);
    }
    TRACE(c, "  inverse ntt (own block)");
    if (int rc = shard_allgatherv(c, (uint8_t *)b.coeffs.p, off, sz)) return rc;
    TRACE(c, "  coefficient blocks exchanged");
    return batch_commit_from_coeffs(c, b);
  }
  ntt_batch(c->stream, c->plan_inv, vals_dev, b.coeffs.p, b.cols, 1, nullptr, ninv, false, CosetMap(), 0, nz ? &h : nullptr);
  TRACE(c, "  inverse ntt");
  return batch_commit_from_coeffs(c, b);
}

int batch_alloc(p2gpu_circuit *c, Batch &b, uint32_t cols) {
  b.cols = cols;
  b.d = c->d;
  b.ncl = c->C;
  b.cm = CosetMap();
  HIP_TRY(b.coeffs.alloc((size_t)cols * c->n));
  HIP_TRY(b.lde.alloc((size_t)cols * c->N));
  size_t cap_per = ((size_t)1 << c->cap_h) >> c->rate_bits;
  return tree_alloc(b, c->C, c->n, cap_per);
}

}  // namespace p2
