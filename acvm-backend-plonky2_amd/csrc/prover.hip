// prover.hip -- the proof: its phases, `prove_impl` and the `p2gpu_prove*` entry points of libp2gpu.so (see include/p2gpu.h;
// the commitment operators are commit.hip, the upload pipeline of a host witness upload.hip, the circuit handle handle.hip,
// the exchanges of a sharded proof transport.hip).
//
// Drop-in for the one call `circuit_data.prove(witnesses)` at
// plonky2-backend/src/actions/prove_action.rs:96 (after witness generation):
// plonky2 0.2.2 plonk/prover.rs prove_with_partition_witness restated as a
// sequence of HIP kernel launches on one stream, with the Fiat-Shamir
// transcript (iop/challenger.rs, Keccak duplex) run on the host between
// phases -- each challenge needs only a 16 x 25 B Merkle cap or a few hundred
// opening values back from the device.  Transcript order: SURVEY.md C.4; the
// transcript, the hasher and the proof's byte layout are the verifier core's
// (verifycore.hpp: vc::Transcript<HK>, vc::Layout), chosen once per proof by
// the handle's hasher (prove_impl).
// The product path never touches oracle/; without a HIP device every entry
// point fails with P2GPU_E_DEVICE.
#include "hostproof.hpp"
#include "prover_internal.hpp"
#include <chrono>

using namespace p2;

namespace {

bool hostprof_on() {
  static const bool on = env_flag("P2GPU_HOSTPROF", false);
  return on;
}

// What one proof carries from phase to phase (everything else is a local of the phase that uses it, or lives in the handle;
// the transcript is prove_phases' own and goes to the two phases that touch it as a parameter)
struct Proof {
  const gl_t *wires_dev;  // the witness [W][n]
  const uint64_t *pis;
  uint32_t n_pi;
  gl_t pih[4];  // public_inputs_hash = InnerHasher(Poseidon).hash_no_pad(public_inputs); [] -> 0^4
  gl_t betas[MAX_CHALLENGES] = {0, 0}, gammas[MAX_CHALLENGES] = {0, 0}, alphas[MAX_CHALLENGES] = {0, 0};
  ext_t zeta;
  Batch *oracles[4];       // constants / sigmas, wires, Z / partial products, quotient chunks: the order of every batched step
  std::vector<ext_t> op;   // the openings: every column of the four oracles at zeta, then the K columns of Z at g * zeta
  // which structured wire columns go without an LDE in memory is fixed at the start for the whole proof (structured_off may
  // flip at the openings; the query gather must see what the commitment saw)
  uint32_t vfirst;
  const uint32_t *h_cls = nullptr;  // host copies of the column classes / scalars (read back with the openings)
  const gl_t *h_val = nullptr;
  std::vector<ext_t> final_poly;
  uint64_t pow_witness;
  std::vector<size_t> qidx;        // the query indices, in [0, N)
  const gl_t *gathered = nullptr;  // the words of every query answer, in proof order (pinned arena)
  p2gpu_timings T;
  double t_lap;
  Proof(p2gpu_circuit *c, const gl_t *wires_dev_, const uint64_t *pis_, uint32_t n_pi_, double h2d_ms)
      : wires_dev(wires_dev_), pis(pis_), n_pi(n_pi_), oracles{&c->cs, &c->wires, &c->zp, &c->quot}, t_lap(now_ms()) {
    memset(&T, 0, sizeof T);
    T.h2d_ms = h2d_ms;
  }
};

// milliseconds since the previous lap (the phase boundaries of p2gpu_timings)
double lap(Proof &P) {
  const double t = now_ms(), dt = t - P.t_lap;
  P.t_lap = t;
  return dt;
}

// columns of the four oracles together
uint32_t committed_cols(const p2gpu_circuit *c) { return c->NC + c->R + c->W + c->K * (1 + c->PP) + c->K * c->QF; }

// ---- 1. wires commitment ----
int commit_wires(p2gpu_circuit *c, Proof &P) {
  g_hp.mark("start");
  TRACE(c, "enter");
  if (int rc = batch_commit_from_values(c, c->wires, P.wires_dev)) return rc;
  TRACE(c, "wires commit");
  return 0;
}

// ---- 2. partial products and Z ----
// the values over the subgroup -> c->zp_vals [K (1 + PP)][n] (enqueued)
int zs_values(p2gpu_circuit *c, Proof &P) {
  hipStream_t st = c->stream;
  const uint32_t d = c->d, K = c->K;
  ZsArgs a;
  a.wires = P.wires_dev;
  a.sigmas = c->d_sigmas.p;
  a.k_is = c->d_kis.p;
  a.sub_tw = c->tw_fwd.p;
  a.tw_shift = 0;
  a.d = d; a.R = c->R; a.QF = c->QF; a.nchunks = c->nchunks; a.K = K;
  for (uint32_t k = 0; k < 2; k++) { a.betas[k] = P.betas[k]; a.gammas[k] = P.gammas[k]; }
  a.cp = c->cp.p;
  a.zp = c->zp_vals.p;
  a.sb = d;
  a.row0 = 0;
  a.rows = (uint32_t)c->n;
  uint32_t lgG = 0;
  while ((1u << lgG) < (uint32_t)c->shard_world) lgG++;
  if (c->shard_zs && sharded(c) && (1u << lgG) == (uint32_t)c->shard_world && d >= lgG) {
    // SURVEY 8(e) step 5 (knob "shard_zs"): the expensive half -- 160 factors, the batch inversion and the chunk quotients of every
    // row -- split by rows; rank q writes its n / G rows as one contiguous block of the scratch ([rank][column][n / G], zs_idx) and
    // the blocks are all-gathered in place.  The scan and the products along the chunks then run on every rank (two cheap passes).
    a.sb = d - lgG;
    a.rows = (uint32_t)(c->n >> lgG);
    a.row0 = a.rows * (uint32_t)c->shard_rank;
    zs_chunks(st, a);
    const size_t blk = (size_t)K * (c->nchunks + 1) * a.rows;
    if (int rc = shard_allgather(c, c->cp.p + blk * (size_t)c->shard_rank, c->cp.p, blk * sizeof(gl_t))) return rc;
    zs_scan_finish(st, a, c->scan_tmp.p);
  } else {
    zs_partial_products(st, a, c->scan_tmp.p);
  }
  TRACE(c, "zs_partial_products");
  return 0;
}
int commit_zs(p2gpu_circuit *c, Proof &P) {
  if (int rc = zs_values(c, P)) return rc;
  return batch_commit_from_values(c, c->zp, c->zp_vals.p);
}

// ---- 3. quotient: alpha powers, the gate sums of the half-domain gates, the quotient values, their chunk polynomials ----
// the quotient values of every LDE point -> c->qvals [K][cosets][n] (enqueued)
int quotient_values(p2gpu_circuit *c, Proof &P) {
  hipStream_t st = c->stream;
  const uint32_t d = c->d, K = c->K, nterms = c->nterms;
  const size_t n = c->n;
  gl_t *ap = c->pin.take<gl_t>((size_t)2 * nterms);
  if (!ap) return pin_exhausted();
  memset(ap, 0, 16 * (size_t)nterms);
  for (uint32_t k = 0; k < K; k++) {
    gl_t a = 1;
    for (uint32_t t = 0; t < nterms; t++) {
      ap[(size_t)k * nterms + t] = a;
      a = gl_mul(a, P.alphas[k]);
    }
  }
  HIP_TRY(hipMemcpyAsync(c->apow.p, ap, 16 * (size_t)nterms, hipMemcpyHostToDevice, st));
  QuotArgs q;
  memset(&q, 0, sizeof q);
  q.cs_lde = c->cs.lde.p;
  q.wires_lde = c->wires.lde.p;
  q.zp_lde = c->zp.lde.p;
  q.k_is = c->d_kis.p;
  q.tw = c->tw_fwd.p;
  q.apow = c->apow.p;
  q.gates = c->d_gates.p;
  q.host_gates = c->gates.data();
  q.out = c->qvals.p;
  q.tw_shift = 0; q.d = d; q.rate_bits = c->rate_bits; q.W = c->W; q.R = c->R; q.NC = c->NC;
  q.num_selectors = c->num_selectors; q.K = K; q.QF = c->QF; q.nchunks = c->nchunks; q.PP = c->PP;
  q.num_gates = c->num_gates; q.nterms = nterms;
  q.coset_first = c->wires.cm.first;
  q.coset_stride = c->wires.cm.stride;
  q.ncosets = c->wires.ncl;
  q.gate_groups = c->gate_groups;
  q.has_poseidon = 0;
  for (auto &g : c->gates)
    if (g.kind == G_POSEIDON) q.has_poseidon = 1;
  for (uint32_t k = 0; k < 2; k++) { q.betas[k] = P.betas[k]; q.gammas[k] = P.gammas[k]; }
  for (int i = 0; i < 4; i++) q.pi_hash[i] = P.pih[i];
  q.qconst = c->qconst.p;
  q.n_inv = gl_inv((gl_t)n);
  q.l0 = c->l0_lde.p;
  // gates of degree <= 4: folded sums on the even cosets, extended to the odd ones (only with every coset on this device)
  q.gate_groups_half = c->gate_groups_half;
  q.nsk = c->half_slots * K;
  q.hsum = c->hsum.p;
  q.use_half = (c->half_gates == 2 || (c->half_gates == 1 && c->half_auto)) && c->half_slots && c->wires.ncl == c->C && c->wires.cm.stride == 1 &&
               c->wires.cm.first == 0;
  if (q.use_half) {
    const size_t per = (size_t)4 * q.nsk * n;
    gate_sums_eval(st, q, n >= 64 ? c->sums_groups : 1u);
    ntt_batch(st, c->plan_inv, c->hsum.p, c->htmp_a.p, 4 * q.nsk, 1, nullptr, q.n_inv, false);
    gate_sums_cross(st, c->htmp_a.p, c->inv_scale.p, c->htmp_b.p, d, q.nsk, c->half_cross);
    CosetMap odd;
    odd.first = 1;
    odd.stride = 2;
    ntt_batch(st, c->plan_fwd, c->htmp_b.p, c->hsum.p + per, q.nsk, 4, c->scale.p, 1, true, odd);
    TRACE(c, "gate sums (half domain)");
  }
  quotient_eval(st, q);
  TRACE(c, "quotient_eval");
  return 0;
}
// c->qvals -> the chunk polynomials, committed
int quotient_chunks_commit(p2gpu_circuit *c) {
  hipStream_t st = c->stream;
  const uint32_t d = c->d, K = c->K;
  const size_t n = c->n;
  // coset_ifft of size N = per-coset inverse transforms + cross-coset butterflies
  ntt_batch(st, c->plan_inv, c->qvals.p, c->qtmp.p, K * c->wires.ncl, 1, nullptr, gl_inv((gl_t)n), false);
  const gl_t *pr = c->qtmp.p;
  if (sharded(c)) {
    // every rank needs all cosets' interpolants for the cross-coset butterflies: all-gather
    // [K][C/world][n] per rank (2 * N * 8 B in total) straight between device buffers
    if (int rc = shard_allgather(c, c->qtmp.p, c->qvals.p, (size_t)K * c->wires.ncl * n * sizeof(gl_t))) return rc;
    pr = c->qvals.p;
  }
  const gl_t wC = gl_root(c->rate_bits), gn = gl_pow(GL_GEN, n);
  quotient_chunks(st, pr, c->inv_scale.p, c->quot.coeffs.p, d, K, c->rate_bits, gl_inv(wC), gl_inv(gn), gl_inv((gl_t)c->C),
                  (uint32_t)c->shard_world);
  TRACE(c, "quotient_chunks");
  return batch_commit_from_coeffs(c, c->quot);
}
int commit_quotient(p2gpu_circuit *c, Proof &P) {
  if (int rc = quotient_values(c, P)) return rc;
  return quotient_chunks_commit(c);
}

// ---- 4. openings: the four batches at zeta and Z at g * zeta in one launch, summed on the host ----
int open_at_zeta(p2gpu_circuit *c, Proof &P) {
  hipStream_t st = c->stream;
  const uint32_t d = c->d, K = c->K, W = c->W, nall = committed_cols(c);
  const size_t n = c->n;
  ext_t zn = P.zeta;
  for (uint32_t i = 0; i < d; i++) zn = ext_mul(zn, zn);
  if (ext_eq(zn, ext_from(1))) {
    set_err("Opening point is in the subgroup.");
    return P2GPU_E_OPENING_IN_SUBGROUP;
  }
  P.op.resize(nall + K);
  uint32_t parts = 1;
  while (parts < 16 && (n / (parts * 2)) >= 1024) parts *= 2;
  ext_powers_bitrev2(st, P.zeta, ext_scale(P.zeta, gl_root(d)), d, c->pw.p, c->pw.p + 2 * n);
  const bool structured = batch_colnz(c, c->wires) != nullptr;
  const ColHints wh = structured ? wire_hints(c, 0, false) : ColHints();
  if (structured) {
    compact_nonzero(st, c->wire_nz.p, c->W, c->wire_nzlist.p);
    if (c->sparse_coeffs.p) eval_columns(st, c->sparse_coeffs.p, 1, d, c->pw.p, parts, c->sparse_partial.p);
  }
  size_t base = 0;
  EvalSegs es;
  for (int o = 0; o < 4; o++) {
    if (structured && P.oracles[o] == &c->wires) {
      es.hinted = es.count;
      es.cls = wh.cls;
      es.val = wh.val;
      es.basis_partial = c->sparse_partial.p;
    }
    es.seg[es.count++] = {P.oracles[o]->coeffs.p, c->pw.p, c->partial.p + base * parts * 2, P.oracles[o]->cols};
    base += P.oracles[o]->cols;
  }
  es.seg[es.count++] = {c->zp.coeffs.p, c->pw.p + 2 * n, c->partial.p + base * parts * 2, K};
  if (sharded(c) && c->shard_world > 1) {
    // SURVEY 8(e) step 8, the openings: every rank holds every coefficient (the inverse transforms are replicated), so rank q
    // evaluates the q-th block of the concatenated columns only and the partial sums (16 x 16 B per column) are all-gathered
    // in place -- 70 KB instead of 7/8 of a 0.09 ms kernel on every rank
    const uint32_t total = (uint32_t)(nall + K), G = (uint32_t)c->shard_world, cpr = (total + G - 1) / G;
    eval_columns_multi(st, es, d, parts, cpr * (uint32_t)c->shard_rank, cpr);
    const size_t blk = (size_t)cpr * parts * 2;
    if (int rc = shard_allgather(c, c->partial.p + blk * (size_t)c->shard_rank, c->partial.p, blk * 8)) return rc;
  } else {
    eval_columns_multi(st, es, d, parts);
  }
  const size_t npart = (size_t)(nall + K) * parts * 2;
  gl_t *part = c->pin.take<gl_t>(npart);
  if (!part) return pin_exhausted();
  HIP_TRY(hipMemcpyAsync(part, c->partial.p, npart * 8, hipMemcpyDeviceToHost, st));
  uint32_t *dense_count = structured ? c->pin.take<uint32_t>(1) : nullptr;
  if (dense_count) HIP_TRY(hipMemcpyAsync(dense_count, c->wire_nzlist.p, 4, hipMemcpyDeviceToHost, st));
  if (P.vfirst != UINT32_MAX) {
    uint32_t *hc = c->pin.take<uint32_t>(W);
    gl_t *hv = c->pin.take<gl_t>(W);
    if (!hc || !hv) return pin_exhausted();
    HIP_TRY(hipMemcpyAsync(hc, c->wire_nz.p, 4 * (size_t)W, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(hv, c->wire_scalar.p, 8 * (size_t)W, hipMemcpyDeviceToHost, st));
    P.h_cls = hc;
    P.h_val = hv;
  }
  g_hp.mark("enq(openings)");
  if (int rc_ = wait_stream(c)) return rc_;
  g_hp.mark("WAIT(openings)");
  // Which wires a circuit leaves unused does not change from proof to proof.  A handle whose witness turned
  // out (almost) fully dense stops looking: the class pass over the witness and the fill launches cost ~0.1 ms
  // at 2^20 rows, what fewer than 5 % structured columns give back; the knob "zero_columns" = 1 makes it look
  // again.  (Every column is then transformed like a dense one, which is always correct.)
  if (dense_count && (uint64_t)(c->W - *dense_count) * 20u < c->W) c->structured_off = true;
  if (dense_count) c->last_dense = *dense_count;
  for (size_t j = 0; j < nall + K; j++) {
    gl_t a0 = 0, a1 = 0;
    for (uint32_t p = 0; p < parts; p++) {
      a0 = gl_add(a0, part[(j * parts + p) * 2]);
      a1 = gl_add(a1, part[(j * parts + p) * 2 + 1]);
    }
    P.op[j] = ext_make(a0, a1);
  }
  TRACE(c, "openings");
  return 0;
}

// ---- 5. FRI: batch reduction with the powers of alpha to the FRI polynomial, its coefficients and its first LDE ----
int fri_reduce(p2gpu_circuit *c, Proof &P, ext_t alpha) {
  hipStream_t st = c->stream;
  const uint32_t d = c->d, K = c->K, nall = committed_cols(c);
  const size_t n = c->n;
  gl_t *apw = c->pin.take<gl_t>((size_t)2 * nall);
  if (!apw) return pin_exhausted();
  ext_t a = ext_from(1);
  ext_t f0z = ext_from(0), f1z = ext_from(0);
  for (uint32_t j = 0; j < nall; j++) {
    apw[2 * j] = a.c0;
    apw[2 * j + 1] = a.c1;
    f0z = ext_add(f0z, ext_mul(a, P.op[j]));
    if (j < K) f1z = ext_add(f1z, ext_mul(a, P.op[nall + j]));
    a = ext_mul(a, alpha);
  }
  HIP_TRY(hipMemcpyAsync(c->ext_apow.p, apw, 16 * (size_t)nall, hipMemcpyHostToDevice, st));
  gl_t *F0 = c->f01.p, *F1 = c->f01.p + 2 * n;
  uint32_t j0 = 0;
  bool reduced = false;
  if (c->shard_reduce && sharded(c)) {
    // SURVEY 8(e) step 8, the FRI batch reduction (knob "shard_reduce"): every rank holds every coefficient, so rank q sums only
    // its block of the 354 concatenated columns (plain loop: structured columns' coefficients are in memory like anybody's) and
    // the partial sums F0_q [2][n] are all-gathered and added -- field addition is exact, the sum does not depend on the split
    const uint32_t G = (uint32_t)c->shard_world, cpr = (nall + G - 1) / G;
    const uint32_t c0 = std::min(cpr * (uint32_t)c->shard_rank, nall), c1 = std::min(c0 + cpr, nall);
    bool first = true;
    uint32_t jo = 0;
    for (int o = 0; o < 4; o++) {
      const uint32_t co = P.oracles[o]->cols;
      const uint32_t lo = std::max(c0, jo) - jo, hi = std::min(c1, jo + co) > jo ? std::min(c1, jo + co) - jo : 0;
      if (hi > lo) {
        reduce_columns(st, P.oracles[o]->coeffs.p + (size_t)lo * n, hi - lo, d, c->ext_apow.p, jo + lo, F0, !first);
        first = false;
      }
      jo += co;
    }
    if (first) HIP_TRY(hipMemsetAsync(F0, 0, 16 * n, st));
    if (int rc = shard_allgather(c, F0, c->xchg_recv.p, 16 * n)) return rc;
    sum_parts(st, c->xchg_recv.p, G, 2 * n, F0);
    reduced = true;
  }
  for (int o = reduced ? 4 : 0; o < 4; o++) {
    const bool hw = batch_colnz(c, *P.oracles[o]) != nullptr;
    const bool unit = hw && c->sparse_coeffs.p != nullptr;
    if (unit) class1_fold(st, wire_hints(c, 0, false), c->W, c->ext_apow.p, j0, c->sparse_partial.p + 32);
    reduce_columns(st, P.oracles[o]->coeffs.p, P.oracles[o]->cols, d, c->ext_apow.p, j0, F0, o != 0,
                   hw ? c->wire_nzlist.p : nullptr, unit ? c->sparse_coeffs.p : nullptr, unit ? c->sparse_partial.p + 32 : nullptr);
    j0 += P.oracles[o]->cols;
  }
  reduce_columns(st, c->zp.coeffs.p, K, d, c->ext_apow.p, 0, F1, false);
  ntt_batch(st, c->plan_fwd, c->f01.p, c->f01v.p, 4, 1, nullptr, 1, false);
  fri_quotient_values(st, c->f01v.p, c->f01v.p + 2 * n, d, c->tw_fwd.p, 0, P.zeta, ext_scale(P.zeta, gl_root(d)), f0z, f1z, ext_pow(alpha, K),
                      c->fv.p);
  ntt_batch(st, c->plan_inv, c->fv.p, c->fri_coef[0].p, 2, 1, nullptr, gl_inv((gl_t)n), false);
  if (c->n_steps > 0) {  // no reduction step (degree <= 2^5): the values are never committed
    ntt_batch(st, c->plan_fwd, c->fri_coef[0].p, c->fri_vals[0].p, 2, c->fri_trees[0].ncl, c->scale.p, 1, false,
              c->fri_trees[0].cm);
  }
  TRACE(c, "fri final poly lde");
  return 0;
}

// the self-check needs only the openings and the challenges: it runs on the host while the GPU is
// busy with the batch reduction and the FRI LDE enqueued by fri_reduce, off the critical path
int self_check(p2gpu_circuit *c, Proof &P) {
  if (c->self_check && !plonk_identity_holds(c, P.op, P.betas, P.gammas, P.alphas, P.zeta, P.pih)) {
    (void)hipStreamSynchronize(c->stream);
    set_err("witness does not satisfy the circuit: the plonk identity fails at zeta (vanishing != Z_H * quotient)");
    return P2GPU_E_UNSATISFIED;
  }
  g_hp.mark("selfcheck");
  return 0;
}

// FRI commit phase: per reduction step the tree of the step's values, its cap into the transcript, the fold with the
// step's challenge and the next LDE; then the final polynomial back to the host
template <int HK>
int fri_commit_steps(p2gpu_circuit *c, Proof &P, vc::Transcript<HK> &ch) {
  hipStream_t st = c->stream;
  uint32_t ds = c->d;
  gl_t shift = GL_GEN;
  for (uint32_t s = 0; s < c->n_steps; s++) {
    const uint32_t ab = c->arity[s];
    Batch &tr = c->fri_trees[s];
    hash_fri_leaves(st, c->fri_vals[s].p, ds, tr.ncl, ab, tr.dig.p, hprc(c));
    if (int rc = tree_build(c, tr, ((size_t)1 << ds) >> ab)) return rc;
    observe_cap(ch, tr.cap);
    const ext_t beta = ch.get_ext();
    fri_fold(st, c->fri_coef[s].p, ds, ab, beta, c->fri_coef[s + 1].p);
    for (uint32_t q = 0; q < ab; q++) shift = gl_sqr(shift);
    ds -= ab;
    if (s + 1 < c->n_steps) {
      fill_coset_scale(st, c->fri_scale.p, shift, gl_root(ds + c->rate_bits), ds, c->C, 1);
      ntt_batch(st, c->fri_plans[s + 1], c->fri_coef[s + 1].p, c->fri_vals[s + 1].p, 2, c->C, c->fri_scale.p, 1, false);
    }
  }
  const size_t n_final = (size_t)1 << ds;
  P.final_poly.resize(n_final);
  gl_t *raw = c->pin.take<gl_t>(2 * n_final);
  if (!raw) return pin_exhausted();
  HIP_TRY(hipMemcpyAsync(raw, c->fri_coef[c->n_steps].p, 16 * n_final, hipMemcpyDeviceToHost, st));
  g_hp.mark("enq(final_poly)");
  if (int rc_ = wait_stream(c)) return rc_;
  g_hp.mark("WAIT(final_poly)");
  for (size_t j = 0; j < n_final; j++) {
    const size_t p = bitrev32((uint32_t)j, ds);
    P.final_poly[j] = ext_make(raw[p], raw[n_final + p]);
  }
  return 0;
}

// PoW: minimum-witness policy (upstream's parallel find_any is not deterministic).  The kernel continues from the
// transcript's sponge as it stands: the n_in pending observations already lie in the state (vc::Transcript).
template <int HK>
int grind(p2gpu_circuit *c, Proof &P, const vc::Transcript<HK> &ch) {
  P.pow_witness = c->pow_hint;
  if (P.pow_witness != UINT64_MAX) return 0;
  hipStream_t st = c->stream;
  // expected minimum witness ~2^pow_bits: start with 2^(pow_bits+1) candidates, then double
  uint64_t batch = 1ull << (c->pow_bits + 1 < 20 ? c->pow_bits + 1 : 20);
  // sharded: the ranks grind disjoint slices of [base, base + batch) and take the minimum of what
  // they found; every rank ends with the same, globally minimal witness
  const bool split = sharded(c);
  const uint64_t ranks = split ? (uint64_t)c->shard_world : 1;
  // staging words taken once: the loop may run for thousands of batches at high pow_bits
  // (pw[0]: the "nothing found" word that resets the device's result; an unsharded proof reads its result into pw[1])
  unsigned long long *pw = c->pin.take<unsigned long long>(2), *found = split ? c->pin.take<unsigned long long>(ranks) : pw + 1;
  if (!pw || !found) return pin_exhausted();
  for (uint64_t base = 0;; base += batch, batch = batch < (1ull << 22) ? batch * 2 : batch) {
    pw[0] = ~0ull;
    HIP_TRY(hipMemcpyAsync(c->pow_result.p, &pw[0], 8, hipMemcpyHostToDevice, st));
    const uint64_t per = (batch + ranks - 1) / ranks;
    const uint64_t my0 = base + per * (uint64_t)(split ? c->shard_rank : 0);
    const uint64_t myn = my0 >= base + batch ? 0 : std::min(per, base + batch - my0);
    if (myn) pow_search(st, ch.st.p, ch.n_in, c->pow_bits, my0, myn, c->pow_result.p, hprc(c));
    const unsigned long long *result = c->pow_result.p;
    if (split) {
      if (int rc = shard_allgather(c, c->pow_result.p, c->xchg_recv.p, 8)) return rc;
      result = (const unsigned long long *)c->xchg_recv.p;
    }
    HIP_TRY(hipMemcpyAsync(found, result, 8 * ranks, hipMemcpyDeviceToHost, st));
    g_hp.mark("enq(pow)");
    if (int rc_ = wait_stream(c)) return rc_;
    g_hp.mark("WAIT(pow)");
    const unsigned long long res = *std::min_element(found, found + ranks);
    if (res != ~0ull) {
      P.pow_witness = res;
      return 0;
    }
    if (base > (1ull << 40)) {
      set_err("proof of work failed");
      return P2GPU_E_DEVICE;
    }
  }
}

// The device addresses of the four words of every sibling digest on the path of leaf `j` (plonky2 order) of tree `b` over
// [cosets][m0] leaf digests, for the rank that holds the leaf's coset; zeros (the gather reads them as 0) for every other rank
void push_path(std::vector<uint64_t> &ptrs, const Batch &b, unsigned lgC, size_t m0, unsigned lgm0, size_t j, bool mine) {
  const size_t levels = b.level_off.size() - 1;
  if (!mine) {
    ptrs.insert(ptrs.end(), 4 * levels, 0);
    return;
  }
  const uint32_t r = bitrev32((uint32_t)(j >> lgm0), lgC), k = bitrev32((uint32_t)(j & (m0 - 1)), lgm0);
  const uint32_t z = (r - b.cm.first) / b.cm.stride;  // local coset
  size_t m = m0;
  for (size_t l = 0; l < levels; l++, m >>= 1) {
    const size_t sib = (k & (m - 1)) ^ (m >> 1);
    const uint64_t base = (uint64_t)(uintptr_t)(b.dig.p + b.level_off[l] + (size_t)z * m + sib);
    for (int w = 0; w < 4; w++) ptrs.push_back(base + 8 * w);
  }
}

// ---- query answers: one pointer list, one gather launch, one D2H (sharded: an exchange, every query from its owner) ----
int answer_queries(p2gpu_circuit *c, Proof &P) {
  hipStream_t st = c->stream;
  const uint32_t d = c->d;
  const size_t n = c->n;
  const unsigned lgC = c->rate_bits;
  std::vector<uint64_t> &ptrs = c->h_ptrs;  // (the handle's: its capacity survives the proof -- one prove per handle at a time)
  ptrs.clear();
  ptrs.reserve(c->gather_cap);
  const int world = c->shard_world, me = c->shard_rank;
  size_t per_query = 0;
  std::vector<std::pair<size_t, uint32_t>> virt_fix;  // (slot of the gather, wire column): slot holds LDE(unit column), wants val * it
  for (size_t x : P.qidx) {
    // every piece of query x lives in coset r = bitrev(top bits of x): one rank owns the query
    const uint32_t r = bitrev32((uint32_t)(x >> d), lgC), k = bitrev32((uint32_t)(x & (n - 1)), d);
    const bool mine = (int)(r % (uint32_t)world) == me;
    const size_t start = ptrs.size();
    for (int o = 0; o < 4; o++) {
      const Batch &b = *P.oracles[o];
      const uint32_t z = (r - b.cm.first) / b.cm.stride;
      for (uint32_t col = 0; col < b.cols; col++) {
        if (o == 1 && col >= P.vfirst && P.h_cls[col] < 2u) {
          // unmaterialised column: class 0 opens to 0, class 1 to val * LDE(unit column)[r][k] (product taken on the host)
          const bool c1 = P.h_cls[col] == 1u && c->sparse_lde.p;
          if (c1) virt_fix.emplace_back(ptrs.size(), col);
          ptrs.push_back(c1 && mine ? (uint64_t)(uintptr_t)(c->sparse_lde.p + (size_t)r * n + k) : 0);
          continue;
        }
        ptrs.push_back(mine ? (uint64_t)(uintptr_t)(b.lde.p + ((size_t)z * b.cols + col) * n + k) : 0);
      }
      push_path(ptrs, b, lgC, n, d, x, mine);
    }
    size_t xi = x;
    uint32_t dcur = d;
    for (uint32_t s = 0; s < c->n_steps; s++) {
      const uint32_t ab = c->arity[s];
      const Batch &tr = c->fri_trees[s];
      const size_t npc = (size_t)1 << dcur, per = npc >> ab;  // per-coset leaves
      const size_t li = xi >> ab;                              // leaf index (plonky2 order) in tree s
      const unsigned lgper = dcur - ab;
      const uint32_t rs = bitrev32((uint32_t)(li >> lgper), lgC), kl = bitrev32((uint32_t)(li & (per - 1)), lgper);
      const uint32_t z = (rs - tr.cm.first) / tr.cm.stride;
      const gl_t *v0 = c->fri_vals[s].p + (size_t)z * 2 * npc;
      for (uint32_t t = 0; t < (1u << ab); t++) {
        const size_t kt = (size_t)bitrev32(t, ab) * per + kl;
        ptrs.push_back(mine ? (uint64_t)(uintptr_t)(v0 + kt) : 0);
        ptrs.push_back(mine ? (uint64_t)(uintptr_t)(v0 + npc + kt) : 0);
      }
      push_path(ptrs, tr, lgC, per, lgper, li, mine);
      xi = li;
      dcur -= ab;
    }
    per_query = ptrs.size() - start;
  }
  g_hp.mark("ptrs");
  if (ptrs.size() > c->gather_cap) {
    set_err("internal: gather buffer too small");
    return P2GPU_E_DEVICE;
  }
  gl_t *gathered = c->pin.take<gl_t>(ptrs.size());
  uint64_t *pptrs = c->pin.take<uint64_t>(ptrs.size());
  if (!gathered || !pptrs) return pin_exhausted();
  memcpy(pptrs, ptrs.data(), ptrs.size() * 8);
  HIP_TRY(hipMemcpyAsync(c->gather_ptrs.p, pptrs, ptrs.size() * 8, hipMemcpyHostToDevice, st));
  gather_u64(st, c->gather_ptrs.p, (uint32_t)ptrs.size(), c->gather_out.p);
  g_hp.mark("launch(gather)");
  if (!sharded(c)) {
    HIP_TRY(hipMemcpyAsync(gathered, c->gather_out.p, ptrs.size() * 8, hipMemcpyDeviceToHost, st));
    g_hp.mark("enq(gather)");
    if (int rc_ = wait_stream(c)) return rc_;
    g_hp.mark("WAIT(gather)");
  } else {
    // each rank gathered the queries that fall into its cosets: exchange and pick every query
    // from its owner
    g_hp.mark("enq(gather)");
    if (int rc = shard_allgather(c, c->gather_out.p, c->xchg_recv.p, ptrs.size() * 8)) return rc;
    g_hp.mark("xchg(gather)");
    std::vector<gl_t> all((size_t)world * ptrs.size());
    HIP_TRY(hipMemcpyAsync(all.data(), c->xchg_recv.p, all.size() * 8, hipMemcpyDeviceToHost, st));
    if (int rc_ = wait_stream(c)) return rc_;
    g_hp.mark("WAIT(gather)");
    for (size_t qi = 0; qi < P.qidx.size(); qi++) {
      const uint32_t owner = bitrev32((uint32_t)(P.qidx[qi] >> d), lgC) % (uint32_t)world;
      memcpy(&gathered[qi * per_query], &all[(size_t)owner * ptrs.size() + qi * per_query], per_query * 8);
    }
  }
  for (auto &f : virt_fix) gathered[f.first] = gl_mul(P.h_val[f.second], gathered[f.first]);
  P.gathered = gathered;
  return 0;
}

// proof bytes, written through a cursor straight into the caller's buffer, which holds the layout's `want` bytes (serialise).
// A write past `cap` is counted, not made: the finished length says whether the proof is the layout's.
struct Buf {
  uint8_t *base;
  size_t len, cap, hb;  // hb: bytes of a digest (Layout::hb)
  void put(const void *p, size_t n) {
    if (len <= cap && n <= cap - len) memcpy(base + len, p, n);
    len += n;
  }
  void u64(uint64_t x) { put(&x, 8); }
  void ext(ext_t e) {
    u64(e.c0);
    u64(e.c1);
  }
  void dig(const dig_t &d) { put(d.w, hb); }
};

// plonky2 ProofWithPublicInputs::to_bytes
void write_proof(const p2gpu_circuit *c, const Proof &P, Buf &out) {
  const uint32_t K = c->K, nall = committed_cols(c), nzs = c->NC + c->R + c->W + K;  // constants, sigmas, wires, Z
  for (auto &dg : c->wires.cap) out.dig(dg);
  for (auto &dg : c->zp.cap) out.dig(dg);
  for (auto &dg : c->quot.cap) out.dig(dg);
  // OpeningSet: constants, plonk_sigmas, wires, plonk_zs, plonk_zs_next, partial_products, quotient_polys
  for (size_t j = 0; j < nzs; j++) out.ext(P.op[j]);
  for (size_t k = 0; k < K; k++) out.ext(P.op[nall + k]);
  for (size_t j = nzs; j < nall; j++) out.ext(P.op[j]);
  for (uint32_t s = 0; s < c->n_steps; s++)
    for (auto &dg : c->fri_trees[s].cap) out.dig(dg);
  size_t g = 0;
  auto put_path = [&](size_t nsib) {
    uint8_t l = (uint8_t)nsib;
    out.put(&l, 1);
    for (size_t i = 0; i < nsib; i++) {
      dig_t dg;
      for (int w = 0; w < 4; w++) dg.w[w] = P.gathered[g++];
      out.dig(dg);
    }
  };
  for (size_t qi = 0; qi < P.qidx.size(); qi++) {
    for (int o = 0; o < 4; o++) {
      const Batch &b = *P.oracles[o];
      out.put(&P.gathered[g], 8 * (size_t)b.cols);
      g += b.cols;
      put_path(b.level_off.size() - 1);
    }
    for (uint32_t s = 0; s < c->n_steps; s++) {
      size_t words = 2u << c->arity[s];
      out.put(&P.gathered[g], 8 * words);
      g += words;
      put_path(c->fri_trees[s].level_off.size() - 1);
    }
  }
  for (auto &e : P.final_poly) out.ext(e);
  out.u64(P.pow_witness);
  for (uint32_t i = 0; i < P.n_pi; i++) out.u64(P.pis[i]);
}

// ---- serialise: the proof bytes to the caller, the timings closed behind them ----
// Every proof of the circuit has the layout's length (vc::Layout::want, what p2gpu_proof_size_bound returns): a shorter buffer
// is refused with that length, a buffer at least as long is written in place.
int serialise(p2gpu_circuit *c, Proof &P, uint8_t *proof_out, size_t *proof_len, p2gpu_timings *tm) {
  const vc::Layout L = layout_of(c);
  const bool fits = *proof_len >= L.want;
  Buf out{proof_out, 0, L.want, L.hb};
  if (fits) write_proof(c, P, out);
  P.T.fri_ms = lap(P);
  P.T.total_ms = P.T.wires_commit_ms + P.T.zs_commit_ms + P.T.quotient_ms + P.T.openings_ms + P.T.fri_ms;
  // event pairs are read back lazily (p2gpu_kernel_stats), so profiling adds no synchronisation to
  // the proof itself; bound the backlog
  if (c->profile && c->pending.size() > 16384) flush_kstats(c);
  if (tm) *tm = P.T;
  if (!fits) {
    *proof_len = L.want;
    set_err("proof buffer too small: need %zu bytes", L.want);
    return P2GPU_E_BUFFER;
  }
  if (out.len != L.want) {
    set_err("internal: serialised %zu proof bytes, the circuit's layout has %zu", out.len, L.want);
    return P2GPU_E_DEVICE;
  }
  *proof_len = out.len;
  g_hp.mark("serialise");
  g_hp.dump();
  return P2GPU_OK;
}

int prove_routed_one(p2gpu_circuit *c, const uint64_t *routed, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out,
                     size_t *proof_len, p2gpu_timings *tm) try {
  HIP_TRY(hipSetDevice(c->device));
  double t0 = now_ms();
  // only the routed columns cross PCIe; every other column is gate-internal and derived on the GPU
  HIP_TRY(hipMemcpyAsync(c->wires_vals.p, routed, 8 * (size_t)c->R * c->n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(c->wires_vals.p + (size_t)c->R * c->n, 0, 8 * (size_t)(c->W - c->R) * c->n, c->stream));
  fill_witness(c->stream, c->wires_vals.p, c->d_row_gate.p, c->d_gates.p, c->d_gconsts.p, c->d_prc.p, c->d,
               c->NC - c->num_selectors, c->W);
  HIP_TRY(hipStreamSynchronize(c->stream));
  double h2d = now_ms() - t0;
  return prove_impl(c, c->wires_vals.p, pis, n_pi, proof_out, proof_len, tm, h2d);
} P2GPU_CATCH

// A device group proves by running the same entry point on every rank, one host thread each; every rank returns the
// same bytes, rank 0's go to the caller.
template <class F>
int group_prove(p2gpu_circuit *c, uint8_t *proof_out, size_t *proof_len, p2gpu_timings *tm, F f) {
  const size_t cap = *proof_len;
  std::vector<std::vector<uint8_t>> local(c->peer ? 0 : c->group.size() + 1);
  std::vector<std::vector<uint8_t>> &scratch = c->peer ? c->peer->proof_scratch : local;  // one prove per handle at a time
  std::vector<size_t> lens(c->group.size() + 1, cap);
  return group_run(c, [&](p2gpu_circuit *m, int q) {
    if (q == 0) return f(m, q, proof_out, proof_len, tm);
    if (scratch[q].size() < cap) scratch[q].resize(cap);
    return f(m, q, scratch[q].data(), &lens[q], (p2gpu_timings *)nullptr);
  });
}

}  // namespace

namespace p2 {

thread_local Prof *g_prof = nullptr;
thread_local HostProf g_hp;

bool trace_on() {
  static const bool on = env_flag("P2GPU_TRACE", false);
  return on;
}

double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

void HostProf::mark(const char *label) {
  if (hostprof_on()) ev.push_back({label, now_ms()});
}
void HostProf::dump() {
  if (!hostprof_on() || ev.empty()) return;
  fprintf(stderr, "[p2gpu hostprof]");
  for (size_t i = 1; i < ev.size(); i++) fprintf(stderr, " %s %+.1fus |", ev[i].first, (ev[i].second - ev[i - 1].second) * 1e3);
  fprintf(stderr, " total %.3f ms\n", ev.back().second - ev.front().second);
  ev.clear();
}

hipEvent_t EventProf::get() {
  hipEvent_t e;
  if (!c->event_pool.empty()) {
    e = c->event_pool.back();
    c->event_pool.pop_back();
  } else {
    (void)hipEventCreate(&e);
  }
  return e;
}
// profile = 1 brackets only the launches that move >= 32 MB (the kernels a roofline is about:
// every event is a marker packet that costs the queue ~3 us, ~190 launches per proof);
// profile = 2 brackets every launch
void EventProf::begin(const char *k, double by) {
  // (all launches of the transform kernel are kept so that its average agrees with rocprofv3's)
  active = c->profile >= 2 || by >= 32e6 || strncmp(k, "ntt_", 4) == 0;
  if (!active) return;
  name = k;
  bytes = by;
  a = get();
  b = get();
  (void)hipEventRecord(a, c->stream);
}
void EventProf::end() {
  if (!active) return;
  (void)hipEventRecord(b, c->stream);
  c->pending.push_back({name, bytes, a, b});
}

void flush_kstats(p2gpu_circuit *c) {
  for (auto &pe : c->pending) {
    float ms = 0;
    (void)hipEventSynchronize(pe.b);
    (void)hipEventElapsedTime(&ms, pe.a, pe.b);
    auto &s = c->kstats[pe.name];
    s.ms += ms;
    s.launches++;
    s.bytes += pe.bytes;
    c->event_pool.push_back(pe.a);
    c->event_pool.push_back(pe.b);
  }
  c->pending.clear();
}

// The proof of one witness on one handle: the phases above in the order of SURVEY.md C.4, the transcript between them
template <int HK>
static int prove_phases(p2gpu_circuit *c, const gl_t *wires_dev, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out, size_t *proof_len,
                        p2gpu_timings *tm, double h2d_ms) {
  if (int rc = check_public_inputs(c, pis, n_pi)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  ProfGuard prof(c);
  Proof P(c, wires_dev, pis, n_pi, h2d_ms);
  // the core permutes with the round constants in their poseidon_device_constants form (CircuitView::prc); poseidon_permute_host
  // adds all twelve words of a round, so that form and poseidon_rc give the same permutation on the host
  gl_t sponge[12];
  vc::Transcript<HK> ch{vc::Strided<gl_t>{sponge, 1}, c->poseidon_rc_gate};
  ch.init();
  const uint32_t K = c->K;
  poseidon_hash_no_pad_host(pis, n_pi, P.pih, c->poseidon_rc);
  c->pin.reset();
  P.vfirst = virt_first(c);

  if (int rc = commit_wires(c, P)) return rc;
  ch.observe_digest(c->circuit_digest);
  for (int i = 0; i < 4; i++) ch.observe(P.pih[i]);
  observe_cap(ch, c->wires.cap);
  for (uint32_t k = 0; k < K; k++) P.betas[k] = ch.get();
  for (uint32_t k = 0; k < K; k++) P.gammas[k] = ch.get();
  P.T.wires_commit_ms = lap(P);

  if (int rc = commit_zs(c, P)) return rc;
  observe_cap(ch, c->zp.cap);
  for (uint32_t k = 0; k < K; k++) P.alphas[k] = ch.get();
  P.T.zs_commit_ms = lap(P);

  if (int rc = commit_quotient(c, P)) return rc;
  observe_cap(ch, c->quot.cap);
  P.zeta = ch.get_ext();
  P.T.quotient_ms = lap(P);

  if (int rc = open_at_zeta(c, P)) return rc;
  for (const ext_t &e : P.op) ch.observe_ext(e);
  g_hp.mark("observe(openings)");
  P.T.openings_ms = lap(P);

  const ext_t fri_alpha = ch.get_ext();
  if (int rc = fri_reduce(c, P, fri_alpha)) return rc;
  if (int rc = self_check(c, P)) return rc;
  if (int rc = fri_commit_steps(c, P, ch)) return rc;  // observes each step's cap, draws each step's beta
  for (const ext_t &e : P.final_poly) ch.observe_ext(e);
  TRACE(c, "fri commit phase");

  if (int rc = grind(c, P, ch)) return rc;
  ch.observe(P.pow_witness);
  const gl_t pow_resp = ch.get();
  if (c->pow_bits && (pow_resp >> (64 - c->pow_bits)) != 0) {
    set_err("proof-of-work witness does not satisfy the leading-zero check");
    return P2GPU_E_ARG;
  }
  P.T.pow_witness = P.pow_witness;
  TRACE(c, "pow");

  P.qidx.resize(c->num_queries);
  for (auto &x : P.qidx) x = (size_t)(ch.get() % c->N);
  if (int rc = answer_queries(c, P)) return rc;

  return serialise(c, P, proof_out, proof_len, tm);
}
int prove_impl(p2gpu_circuit *c, const gl_t *wires_dev, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out, size_t *proof_len,
               p2gpu_timings *tm, double h2d_ms) {
  return c->hasher ? prove_phases<1>(c, wires_dev, pis, n_pi, proof_out, proof_len, tm, h2d_ms)
                   : prove_phases<0>(c, wires_dev, pis, n_pi, proof_out, proof_len, tm, h2d_ms);
}

// p2gpu_plonk_stages behind its argument checks: phases 1-3 of prove_impl -- the same phase functions -- with the caller's
// challenges where the transcript's would be, and the raw results of phases 2 and 3 read back between them
int plonk_stages_impl(p2gpu_circuit *c, const uint64_t *wires, const uint64_t *pi_hash, const uint64_t *betas, const uint64_t *gammas,
                      const uint64_t *alphas, const uint64_t *zp_in, uint64_t *zp_out, uint64_t *qvals_out, uint64_t *quot_out,
                      uint8_t *caps_out) {
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = c->n, nzp = (size_t)c->K * (1 + c->PP), nq = (size_t)c->K * c->C;
  HIP_TRY(hipMemcpyAsync(c->wires_vals.p, wires, 8 * (size_t)c->W * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  ProfGuard prof(c);
  Proof P(c, c->wires_vals.p, nullptr, 0, 0.0);
  for (int i = 0; i < 4; i++) P.pih[i] = pi_hash[i];
  for (uint32_t k = 0; k < c->K; k++) { P.betas[k] = betas[k]; P.gammas[k] = gammas[k]; P.alphas[k] = alphas[k]; }
  c->pin.reset();
  P.vfirst = virt_first(c);
  const vc::Layout L = layout_of(c);
  const size_t hb = L.hb, ncap = L.ncap;
  auto put_cap = [&](int which, const Batch &b) {
    for (size_t i = 0; i < ncap; i++) memcpy(caps_out + (which * ncap + i) * hb, b.cap[i].w, hb);
  };

  if (int rc = commit_wires(c, P)) return rc;
  put_cap(0, c->wires);

  if (int rc = zs_values(c, P)) return rc;
  HIP_TRY(hipMemcpyAsync(zp_out, c->zp_vals.p, 8 * nzp * n, hipMemcpyDeviceToHost, c->stream));
  if (zp_in) HIP_TRY(hipMemcpyAsync(c->zp_vals.p, zp_in, 8 * nzp * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (int rc = batch_commit_from_values(c, c->zp, c->zp_vals.p)) return rc;
  put_cap(1, c->zp);

  if (int rc = quotient_values(c, P)) return rc;
  HIP_TRY(hipMemcpyAsync(qvals_out, c->qvals.p, 8 * nq * n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (int rc = quotient_chunks_commit(c)) return rc;
  put_cap(2, c->quot);
  // the library stores coefficients at bit-reversed positions; the caller gets plonky2's natural order
  std::vector<uint64_t> br(nq * n);
  HIP_TRY(hipMemcpy(br.data(), c->quot.coeffs.p, 8 * nq * n, hipMemcpyDeviceToHost));
  for (size_t col = 0; col < nq; col++)
    for (size_t p = 0; p < n; p++) {
      size_t e = 0;
      for (uint32_t b = 0; b < c->d; b++) e |= ((p >> b) & 1) << (c->d - 1 - b);
      quot_out[col * n + e] = br[col * n + p];
    }
  if (c->profile && c->pending.size() > 16384) flush_kstats(c);
  return P2GPU_OK;
}

}  // namespace p2

extern "C" {

int p2gpu_plonk_stages(p2gpu_circuit *c, const uint64_t *wires, const uint64_t *pi_hash, const uint64_t *betas, const uint64_t *gammas,
                       const uint64_t *alphas, const uint64_t *zp_in, uint64_t *zp_out, uint64_t *qvals_out, uint64_t *quot_out,
                       uint8_t *caps_out) try {
  // every refusal is decided here, before any device call
  if (!c || !wires || !pi_hash || !betas || !gammas || !alphas || !zp_out || !qvals_out || !quot_out || !caps_out) {
    set_err("p2gpu_plonk_stages: a null pointer (only zp_in may be null)");
    return P2GPU_E_ARG;
  }
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty() || sharded(c) || c->shard_world > 1) {
    set_err("p2gpu_plonk_stages: a plain handle is needed, not a device group or a sharded handle");
    return P2GPU_E_ARG;
  }
  auto canonical = [](const uint64_t *v, size_t cnt) {
    uint64_t big = 0;
    for (size_t i = 0; i < cnt; i++) big |= (uint64_t)(v[i] >= GL_P);
    return !big;
  };
  const size_t nzp = (size_t)c->K * (1 + c->PP);
  if (!canonical(wires, (size_t)c->W * c->n) || !canonical(pi_hash, 4) || !canonical(betas, c->K) || !canonical(gammas, c->K) ||
      !canonical(alphas, c->K) || (zp_in && !canonical(zp_in, nzp * c->n))) {
    set_err("p2gpu_plonk_stages: a word that is not a canonical field element");
    return P2GPU_E_ARG;
  }
  return plonk_stages_impl(c, wires, pi_hash, betas, gammas, alphas, zp_in, zp_out, qvals_out, quot_out, caps_out);
} P2GPU_CATCH

int p2gpu_fill_witness(p2gpu_circuit *c, uint64_t *wires_dev) try {
  if (!c || !wires_dev) return P2GPU_E_ARG;
  if (int rc = prover_handle(c)) return rc;
  HIP_TRY(hipSetDevice(c->device));
  fill_witness(c->stream, wires_dev, c->d_row_gate.p, c->d_gates.p, c->d_gconsts.p, c->d_prc.p, c->d, c->NC - c->num_selectors,
               c->W);
  HIP_TRY(hipStreamSynchronize(c->stream));
  return P2GPU_OK;
} P2GPU_CATCH

int p2gpu_prove_routed(p2gpu_circuit *c, const uint64_t *routed, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out,
                       size_t *proof_len, p2gpu_timings *tm) try {
  if (!c || !routed || !proof_out || !proof_len) return P2GPU_E_ARG;
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty())
    return group_prove(c, proof_out, proof_len, tm, [&](p2gpu_circuit *m, int, uint8_t *po, size_t *pl, p2gpu_timings *t) {
      return prove_routed_one(m, routed, pis, n_pi, po, pl, t);
    });
  return prove_routed_one(c, routed, pis, n_pi, proof_out, proof_len, tm);
} P2GPU_CATCH

int p2gpu_prove_dev(p2gpu_circuit *c, const uint64_t *wires_dev, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out,
                    size_t *proof_len, p2gpu_timings *tm) try {
  if (!c || !wires_dev || !proof_out || !proof_len) return P2GPU_E_ARG;
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty())
    // the witness is resident on rank 0's device: the other ranks pull it over the peer link into their own staging
    // buffer (the host-witness entry points shard the upload instead: each rank fetches 1/world of it over its own PCIe link)
    return group_prove(c, proof_out, proof_len, tm, [&](p2gpu_circuit *m, int, uint8_t *po, size_t *pl, p2gpu_timings *t) {
      const uint64_t *w = wires_dev;
      if (m->device != c->device) {
        HIP_TRY(hipSetDevice(m->device));
        HIP_TRY(hipMemcpyPeerAsync(m->wires_vals.p, m->device, wires_dev, c->device, 8 * (size_t)m->W * m->n, m->stream));
        w = m->wires_vals.p;
      }
      return prove_impl(m, w, pis, n_pi, po, pl, t, 0.0);
    });
  return prove_impl(c, wires_dev, pis, n_pi, proof_out, proof_len, tm, 0.0);
} P2GPU_CATCH

int p2gpu_prove(p2gpu_circuit *c, const uint64_t *wires, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out,
                size_t *proof_len, p2gpu_timings *tm) try {
  if (!c || !wires || !proof_out || !proof_len) return P2GPU_E_ARG;
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty())
    return group_prove(c, proof_out, proof_len, tm, [&](p2gpu_circuit *m, int, uint8_t *po, size_t *pl, p2gpu_timings *t) {
      return prove_host(m, wires, m->W, nullptr, 0, pis, n_pi, po, pl, t);
    });
  return prove_host(c, wires, c->W, nullptr, 0, pis, n_pi, proof_out, proof_len, tm);
} P2GPU_CATCH

int p2gpu_prove_sparse(p2gpu_circuit *c, const uint64_t *wires, uint32_t ncols, const uint64_t *tail, uint32_t row,
                       const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out, size_t *proof_len, p2gpu_timings *tm) try {
  if (!c || !proof_out || !proof_len || (ncols && !wires)) return P2GPU_E_ARG;
  if (int rc = prover_handle(c)) return rc;
  if (ncols > c->W || (ncols < c->W && !tail) || row >= c->n) {
    set_err("p2gpu_prove_sparse: %u dense columns of %u wires, row %u of %zu%s", ncols, c->W, row, c->n, (ncols < c->W && !tail) ? ", no tail values" : "");
    return P2GPU_E_ARG;
  }
  if (!c->group.empty())
    return group_prove(c, proof_out, proof_len, tm, [&](p2gpu_circuit *m, int, uint8_t *po, size_t *pl, p2gpu_timings *t) {
      return prove_host(m, wires, ncols, tail, row, pis, n_pi, po, pl, t);
    });
  return prove_host(c, wires, ncols, tail, row, pis, n_pi, proof_out, proof_len, tm);
} P2GPU_CATCH

}  // extern "C"
