// provebatchcore.hpp -- the proofs of a slab of witnesses of one small circuit (degree_bits <= P2GPU_PROVE_BATCH_MAX_DEGREE_BITS),
// every step with a proof index: the bodies of the kernels of provebatch.hip and the one sequence that launches them.
//
// A second, plain prover beside prover.hip: the same phase order (prove_phases there; oracle/prover.c is the compact
// restatement), no tuning.  Everything a proof draws from its transcript -- betas, gammas, alphas, zeta, the FRI alpha and
// betas, the proof-of-work witness, the query indices -- and its status stay in device memory in a Record per proof; the
// transcript is vc::Transcript<HK> run by one lane per proof, its sponge kept in the Record between phases.  So the host
// enqueues one fixed sequence of launches per slab (prove_slab below; their number does not depend on the number of proofs) and
// synchronises once, behind the copy of the finished proof bytes.
//
// The bodies are host-and-device functions of (arguments, item index) or (arguments, block, thread, threads, LDS), like
// verifycore.hpp's: a runner launches them as kernels (provebatch.hip), and a host runner that calls them in loops with one
// thread per block runs the same sequence without a device (tests/provebatch_check.cpp).
//
// Storage of a proof's own oracles (wires, Z | partial products, quotient chunks, FRI step values): coefficients in natural
// order [cols][n]; the LDE row-major in leaf order, rows[x][col] with x = bitrev(natural LDE index) -- a leaf is one contiguous
// row (vc::leaf_digest_at hashes it where it lies, the query answer is a copy); trees level by level in plonky2's order, level
// l + 1 node j = H(level l node 2 j, node 2 j + 1), down to the 2^cap_h cap.  Constants and sigmas are read from the handle's
// own coefficients, LDE ([coset][col][n]) and tree (commit.hip's layout), with the handle's twiddle and coset-scale tables.
#pragma once
#include "verifycore.hpp"
#include <type_traits>

#if defined(__HIP_DEVICE_COMPILE__)
#define PB_SYNC() __syncthreads()
#else
#define PB_SYNC() ((void)0)
#endif

namespace p2 {
namespace pb {

constexpr uint32_t MAX_DEGREE_BITS = 12;  // P2GPU_PROVE_BATCH_MAX_DEGREE_BITS
constexpr uint32_t MAX_CHUNKS = 16;       // ceil(MAX_ROUTED / quotient_degree_factor) at the factor 8 of every configuration
constexpr uint32_t MAX_TREE_LEVELS = 24;
constexpr uint32_t POW_GROUPS = 16;       // workgroups per proof in the proof-of-work search
constexpr uint32_t POW_THREADS = 256;

constexpr int32_t ST_OK = 0, ST_INTERNAL = -3, ST_OPENING_IN_SUBGROUP = -4, ST_UNSATISFIED = -5;  // the P2GPU_E_* codes (p2gpu.h)

// what one proof carries from phase to phase
struct Record {
  gl_t sponge[12];
  uint32_t n_in, n_out;
  gl_t pih[4];
  gl_t betas[vc::VC_MAX_CHALLENGES], gammas[vc::VC_MAX_CHALLENGES], alphas[vc::VC_MAX_CHALLENGES];
  ext_t zeta, g_zeta, fri_alpha, alpha_k;
  ext_t fri_beta[vc::VC_MAX_STEPS];
  unsigned long long pow_witness;
  uint32_t qidx[vc::VC_MAX_QUERIES];
  int32_t status;
};

// one committed batch of a slab
struct Oracle {
  gl_t *coef;   // [B][cols][n] natural order
  gl_t *rows;   // [B][N][cols] leaf order
  dig_t *dig;   // [B][tree_size(N)]
  uint32_t cols;
};

// what a launch works on besides the slab (set per launch)
struct Job {
  // lde: coefficients or values [cols][2^lg] per proof -> rows [2^(lg + rate_bits)][cols] per proof
  const gl_t *src;
  size_t src_stride;   // words between proofs
  gl_t *coef_out;      // from values: the coefficients, natural order (same strides as src); else null
  gl_t *rows;
  uint32_t cols, lg, shift_lg, from_values;  // shift_lg: the coset shifts are (g w_N^r)^(2^shift_lg)
  // leaves / tree: `leaves` leaves of leaf_len words each per proof, contiguous
  const gl_t *leaf_src;
  size_t leaf_stride;  // words between proofs
  uint32_t leaf_len, lg_leaves;
  dig_t *dig;
  uint32_t step;       // FRI step
};

struct Args {
  vc::CircuitView c;  // pointers in the memory of whoever runs the bodies
  vc::Layout L;
  uint32_t B, nterms, self_check, dh;  // dh: the handle's degree bits (= c.d; the tables' size)
  size_t want8;                        // bytes between proofs in `proofs`: L.want rounded up to 8
  // the handle's tables
  const gl_t *tw_fwd, *tw_inv;     // w_n^i, w_n^-i, i < n / 2
  const gl_t *scale, *inv_scale;   // [C][n]: (g w_N^r)^(+-bitrev_d(p))
  const gl_t *sigmas;              // [R][n] values
  const gl_t *cs_coef;             // [ncs][n], bit-reversed positions
  const gl_t *cs_lde;              // [C][ncs][n]
  const dig_t *cs_dig;             // levels [C][n >> l] at cs_level_off[l]
  size_t cs_level_off[MAX_TREE_LEVELS];
  // the slab
  const gl_t *wires;  // [B][W][n]
  const gl_t *pis;    // [B][num_pi]
  Record *rec;
  gl_t *apow;         // [B][K][nterms]
  ext_t *eapow;       // [B][nall]
  ext_t *op;          // [B][nall + K]
  ext_t *terms;       // [identity_terms][B]
  gl_t *zp_vals;      // [B][nzp][n]
  gl_t *cp;           // [B][K][n][nchunks]
  Oracle o[4];        // o[0]: unused (the handle's); wires, Z | partial products, quotient
  gl_t *qv;           // [B][K][C][n]
  ext_t *f01;         // [B][2][n]: F0, F1, then their quotients by (X - zeta), (X - g zeta)
  gl_t *fri_coef[vc::VC_MAX_STEPS + 1];  // [B][2][n_s] coordinate planes, natural order
  gl_t *fri_rows[vc::VC_MAX_STEPS];      // [B][8 n_s][2]
  dig_t *fri_dig[vc::VC_MAX_STEPS];
  uint8_t *proofs;    // [B][want8]
  Job j;
};

// ---- sizes -----------------------------------------------------------------------------------------------------------------
P2_HD size_t tree_size(uint32_t lg_leaves) { return (size_t)2 << lg_leaves; }  // every level, rounded up
P2_HD size_t level_off(uint32_t lg_leaves, uint32_t l) {                        // sum_{i < l} leaves >> i
  return ((size_t)2 << lg_leaves) - ((size_t)2 << (lg_leaves - l));
}
P2_HD uint32_t fri_lg(const Args &a, uint32_t s) {  // log2 of the coefficient count before step s
  uint32_t lg = a.c.d;
  for (uint32_t i = 0; i < s; i++) lg -= a.c.arity[i];
  return lg;
}
P2_HD gl_t cs_at(const Args &a, uint32_t r, uint32_t k, uint32_t col) {
  return a.cs_lde[(((size_t)r * a.L.ncs + col) << a.c.d) + k];
}
// natural LDE index i = k C + r of leaf x
P2_HD uint32_t leaf_coset(const Args &a, uint32_t x, uint32_t *k) {
  const uint32_t i = bitrev32(x, a.L.lgN);
  *k = i >> a.c.rate_bits;
  return i & ((1u << a.c.rate_bits) - 1);
}
P2_HD void put64(uint8_t *p, size_t at, uint64_t v) {
  for (int i = 0; i < 8; i++) p[at + i] = (uint8_t)(v >> (8 * i));
}
P2_HD void put_dig(uint8_t *p, size_t at, const dig_t &d, uint32_t hb) {
  for (uint32_t i = 0; i < hb; i++) p[at + i] = (uint8_t)(d.w[i >> 3] >> (8 * (i & 7)));
}
template <int HK>
P2_HD vc::Transcript<HK> transcript_of(const Args &a, Record &r) {
  vc::Transcript<HK> ch{vc::Strided<gl_t>{r.sponge, 1}, a.c.prc};
  ch.n_in = r.n_in;
  ch.n_out = r.n_out;
  return ch;
}
template <int HK>
P2_HD void transcript_keep(const vc::Transcript<HK> &ch, Record &r) {
  r.n_in = ch.n_in;
  r.n_out = ch.n_out;
}
template <int HK>
P2_HD void observe_cap(vc::Transcript<HK> &ch, const dig_t *dig, uint32_t lg_leaves, uint32_t cap_h) {
  const dig_t *cap = dig + level_off(lg_leaves, lg_leaves - cap_h);
  for (uint32_t i = 0; i < (1u << cap_h); i++) ch.observe_digest(cap[i]);
}

// ---- transforms: one block per (proof, column) -----------------------------------------------------------------------------
// radix-2 decimation in time in x[0 .. 2^lg): bit-reversed in, natural out; roots w^e = tw[e << (dh - lg)], e < 2^(lg - 1)
P2_HD void dit(gl_t *x, uint32_t lg, const gl_t *tw, uint32_t dh, uint32_t tid, uint32_t nt) {
  const uint32_t half = (1u << lg) >> 1;
  for (uint32_t s = 0; s < lg; s++) {
    const uint32_t hm = 1u << s;
    for (uint32_t t = tid; t < half; t += nt) {
      const uint32_t jj = t & (hm - 1), i0 = ((t >> s) << (s + 1)) + jj, i1 = i0 + hm;
      const gl_t w = tw[((size_t)jj << (lg - 1 - s)) << (dh - lg)];
      const gl_t u = x[i0], v = gl_mul(x[i1], w);
      x[i0] = gl_add(u, v);
      x[i1] = gl_sub(u, v);
    }
    PB_SYNC();
  }
}
// values over the subgroup -> coefficients, natural order, in x
P2_HD void to_coeffs(const Args &a, const gl_t *vals, gl_t *x, uint32_t lg, uint32_t tid, uint32_t nt) {
  const uint32_t n = 1u << lg;
  for (uint32_t i = tid; i < n; i += nt) x[bitrev32(i, lg)] = vals[i];
  PB_SYNC();
  dit(x, lg, a.tw_inv, a.dh, tid, nt);
  const gl_t ninv = gl_inv((gl_t)n);
  for (uint32_t i = tid; i < n; i += nt) x[i] = gl_mul(x[i], ninv);
  PB_SYNC();
}
// lds: 2 * 2^lg words
P2_HD void lde_body(const Args &a, uint32_t blk, uint32_t tid, uint32_t nt, gl_t *lds) {
  const Job &j = a.j;
  const uint32_t b = blk / j.cols, col = blk - b * j.cols, lg = j.lg, n = 1u << lg, rb = a.c.rate_bits, C = 1u << rb;
  gl_t *coef = lds, *x = lds + n;
  const gl_t *src = j.src + (size_t)b * j.src_stride + ((size_t)col << lg);
  if (j.from_values) {
    to_coeffs(a, src, coef, lg, tid, nt);
    gl_t *out = j.coef_out + (size_t)b * j.src_stride + ((size_t)col << lg);
    for (uint32_t i = tid; i < n; i += nt) out[i] = coef[i];
  } else {
    for (uint32_t i = tid; i < n; i += nt) coef[i] = src[i];
    PB_SYNC();
  }
  gl_t *rows = j.rows + (((size_t)b << (lg + rb)) * j.cols) + col;
  for (uint32_t r = 0; r < C; r++) {
    for (uint32_t i = tid; i < n; i += nt) {
      const gl_t s = a.scale[((size_t)r << a.dh) + bitrev32(i << j.shift_lg, a.dh)];
      x[bitrev32(i, lg)] = gl_mul(coef[i], s);
    }
    PB_SYNC();
    dit(x, lg, a.tw_fwd, a.dh, tid, nt);
    for (uint32_t k = tid; k < n; k += nt) rows[(size_t)bitrev32((k << rb) + r, lg + rb) * j.cols] = x[k];
    PB_SYNC();
  }
}

// ---- commitments -------------------------------------------------------------------------------------------------------------
template <int HK>
P2_HD void leaf_body(const Args &a, uint32_t g) {
  const Job &j = a.j;
  const uint32_t b = g >> j.lg_leaves, leaf = g & ((1u << j.lg_leaves) - 1);
  const uint8_t *p = (const uint8_t *)(j.leaf_src + (size_t)b * j.leaf_stride);
  j.dig[(size_t)b * tree_size(j.lg_leaves) + leaf] = vc::leaf_digest_at<HK>(p, 8 * (size_t)leaf * j.leaf_len, j.leaf_len, a.c.prc);
}
// one block per (proof, cap entry): the subtree below it, level by level
template <int HK>
P2_HD void tree_body(const Args &a, uint32_t blk, uint32_t tid, uint32_t nt, gl_t *) {
  const Job &j = a.j;
  const uint32_t cap_h = a.c.cap_h, b = blk >> cap_h, e = blk & ((1u << cap_h) - 1), lgs = j.lg_leaves - cap_h;
  dig_t *dig = j.dig + (size_t)b * tree_size(j.lg_leaves);
  for (uint32_t l = 1; l <= lgs; l++) {
    const dig_t *below = dig + level_off(j.lg_leaves, l - 1);
    dig_t *lvl = dig + level_off(j.lg_leaves, l);
    const uint32_t cnt = 1u << (lgs - l);
    for (uint32_t i = tid; i < cnt; i += nt) {
      const size_t node = (size_t)e * cnt + i;
      lvl[node] = vc::node_digest_hk<HK>(below[2 * node], below[2 * node + 1], a.c.prc);
    }
    PB_SYNC();
  }
}

// ---- transcript steps: one lane per proof --------------------------------------------------------------------------------------
template <int HK>
P2_HD void t_wires(const Args &a, uint32_t b) {
  Record &r = a.rec[b];
  {
    gl_t st[12];
    for (int i = 0; i < 12; i++) st[i] = 0;
    for (uint32_t off = 0; off < a.c.num_pi; off += 8) {
      for (uint32_t i = 0; i < 8; i++)
        if (off + i < a.c.num_pi) st[i] = a.pis[(size_t)b * a.c.num_pi + off + i];
      vc::poseidon_permute_hd(st, a.c.prc);
    }
    for (int i = 0; i < 4; i++) r.pih[i] = st[i];
  }
  r.status = ST_OK;
  r.pow_witness = ~0ull;
  vc::Transcript<HK> ch{vc::Strided<gl_t>{r.sponge, 1}, a.c.prc};
  ch.init();
  ch.observe_digest(a.c.circuit_digest);
  for (int i = 0; i < 4; i++) ch.observe(r.pih[i]);
  observe_cap(ch, a.o[1].dig + (size_t)b * tree_size(a.L.lgN), a.L.lgN, a.c.cap_h);
  for (uint32_t k = 0; k < vc::VC_MAX_CHALLENGES; k++) r.betas[k] = r.gammas[k] = r.alphas[k] = 0;
  for (uint32_t k = 0; k < a.c.K; k++) r.betas[k] = ch.get();
  for (uint32_t k = 0; k < a.c.K; k++) r.gammas[k] = ch.get();
  transcript_keep(ch, r);
}
template <int HK>
P2_HD void t_zs(const Args &a, uint32_t b) {
  Record &r = a.rec[b];
  vc::Transcript<HK> ch = transcript_of<HK>(a, r);
  observe_cap(ch, a.o[2].dig + (size_t)b * tree_size(a.L.lgN), a.L.lgN, a.c.cap_h);
  for (uint32_t k = 0; k < a.c.K; k++) {
    r.alphas[k] = ch.get();
    gl_t p = 1, *ap = a.apow + ((size_t)b * a.c.K + k) * a.nterms;
    for (uint32_t t = 0; t < a.nterms; t++) {
      ap[t] = p;
      p = gl_mul(p, r.alphas[k]);
    }
  }
  transcript_keep(ch, r);
}
template <int HK>
P2_HD void t_quotient(const Args &a, uint32_t b) {
  Record &r = a.rec[b];
  vc::Transcript<HK> ch = transcript_of<HK>(a, r);
  observe_cap(ch, a.o[3].dig + (size_t)b * tree_size(a.L.lgN), a.L.lgN, a.c.cap_h);
  r.zeta = ch.get_ext();
  r.g_zeta = ext_scale(r.zeta, gl_root(a.c.d));
  ext_t zn = r.zeta;
  for (uint32_t i = 0; i < a.c.d; i++) zn = ext_mul(zn, zn);
  if (zn.c0 == 1 && zn.c1 == 0) r.status = ST_OPENING_IN_SUBGROUP;
  transcript_keep(ch, r);
}
template <int HK>
P2_HD void t_openings(const Args &a, uint32_t b) {
  Record &r = a.rec[b];
  vc::Transcript<HK> ch = transcript_of<HK>(a, r);
  const uint32_t nall = a.L.nall, K = a.c.K;
  const ext_t *op = a.op + (size_t)b * (nall + K);
  for (uint32_t jx = 0; jx < nall + K; jx++) ch.observe_ext(op[jx]);
  r.fri_alpha = ch.get_ext();
  ext_t p = ext_from(1), *ea = a.eapow + (size_t)b * nall;
  for (uint32_t jx = 0; jx < nall; jx++) {
    ea[jx] = p;
    p = ext_mul(p, r.fri_alpha);
  }
  r.alpha_k = ext_pow(r.fri_alpha, K);
  transcript_keep(ch, r);
  if (a.self_check && r.status == ST_OK) {
    const vc::Openings o{op, nullptr, 0, 0, nall, K};
    if (!vc::plonk_identity_at(a.c, o, vc::Strided<ext_t>{a.terms + b, a.B}, r.betas, r.gammas, r.alphas, r.zeta, r.pih)) r.status = ST_UNSATISFIED;
  }
}
template <int HK>
P2_HD void t_step(const Args &a, uint32_t b) {
  Record &r = a.rec[b];
  vc::Transcript<HK> ch = transcript_of<HK>(a, r);
  const uint32_t s = a.j.step, lgl = fri_lg(a, s) + a.c.rate_bits - a.c.arity[s];
  observe_cap(ch, a.fri_dig[s] + (size_t)b * tree_size(lgl), lgl, a.c.cap_h);
  r.fri_beta[s] = ch.get_ext();
  transcript_keep(ch, r);
}
template <int HK>
P2_HD void t_final(const Args &a, uint32_t b) {
  Record &r = a.rec[b];
  vc::Transcript<HK> ch = transcript_of<HK>(a, r);
  const uint32_t lg = fri_lg(a, a.c.n_steps), nf = 1u << lg;
  const gl_t *f = a.fri_coef[a.c.n_steps] + ((size_t)b * 2 << lg);
  for (uint32_t i = 0; i < nf; i++) ch.observe_ext(ext_make(f[i], f[nf + i]));
  transcript_keep(ch, r);
}
// blocks [b * POW_GROUPS + g]: group g searches the windows g, g + G, ... (of `nt` candidates each) and stops once a hit lies
// below its window: every candidate below the smallest hit has been tried, the result is the minimum
template <int HK>
P2_HD void pow_body(const Args &a, uint32_t blk, uint32_t tid, uint32_t nt, gl_t *) {
  const uint32_t groups = a.j.cols, b = blk / groups, g = blk - b * groups, pb = a.c.pow_bits;
  Record &r = a.rec[b];
  gl_t base[12];
  for (int i = 0; i < 12; i++) base[i] = r.sponge[i];
  const uint32_t pos = r.n_in;
  const unsigned long long limit = 1ull << (pb + 8 < 40 ? pb + 8 : 40);  // a miss of all of them: e^-256
  for (unsigned long long win = g;; win += groups) {
    const unsigned long long start = win * nt;
#if defined(__HIP_DEVICE_COMPILE__)
    const unsigned long long best = __atomic_load_n(&r.pow_witness, __ATOMIC_RELAXED);
#else
    const unsigned long long best = r.pow_witness;
#endif
    if (best < start || start >= limit) break;
    const unsigned long long cand = start + tid;
    gl_t st[12];
    for (int i = 0; i < 12; i++) st[i] = base[i];
    st[pos] = cand;
    vc::sponge_permute<HK>(st, a.c.prc);
    if (pb == 0 || (st[7] >> (64 - pb)) == 0) {
#if defined(__HIP_DEVICE_COMPILE__)
      atomicMin(&r.pow_witness, cand);
#else
      if (cand < r.pow_witness) r.pow_witness = cand;
#endif
    }
  }
}
template <int HK>
P2_HD void t_queries(const Args &a, uint32_t b) {
  Record &r = a.rec[b];
  vc::Transcript<HK> ch = transcript_of<HK>(a, r);
  if (r.pow_witness == ~0ull) {
    r.status = ST_INTERNAL;
    r.pow_witness = 0;
  }
  ch.observe((gl_t)r.pow_witness);
  const gl_t resp = ch.get();
  if (a.c.pow_bits && (resp >> (64 - a.c.pow_bits)) != 0 && r.status == ST_OK) r.status = ST_INTERNAL;
  const uint32_t mask = (1u << a.L.lgN) - 1;
  for (uint32_t q = 0; q < a.c.num_queries; q++) r.qidx[q] = (uint32_t)(ch.get() & mask);  // N is a power of two: % N
  transcript_keep(ch, r);
}

// ---- Z and partial products -------------------------------------------------------------------------------------------------------
// lane per (proof, challenge, row): the chunk quotients, one inversion per row
P2_HD void zs_chunks(const Args &a, uint32_t g) {
  const uint32_t d = a.c.d, n = 1u << d, K = a.c.K, R = a.c.R, QF = a.c.QF, nch = a.c.nchunks;
  const uint32_t i = g & (n - 1), bk = g >> d, b = bk / K, k = bk - b * K;
  const Record &r = a.rec[b];
  const gl_t beta = r.betas[k], gamma = r.gammas[k];
  const gl_t x = i < n / 2 ? a.tw_fwd[i] : gl_neg(a.tw_fwd[i - n / 2]);
  const gl_t *w = a.wires + ((size_t)b * a.c.W << d) + i;
  gl_t np[MAX_CHUNKS], dp[MAX_CHUNKS], pre[MAX_CHUNKS];
  gl_t acc = 1;
  for (uint32_t m = 0; m < MAX_CHUNKS; m++) {
    if (m >= nch) break;
    gl_t pn = 1, pd = 1;
    for (uint32_t jx = m * QF; jx < (m + 1) * QF && jx < R; jx++) {
      const gl_t wg = gl_add(w[(size_t)jx << d], gamma);
      pn = gl_mul(pn, gl_add(wg, gl_mul(beta, gl_mul(a.c.k_is[jx], x))));
      pd = gl_mul(pd, gl_add(wg, gl_mul(beta, a.sigmas[((size_t)jx << d) + i])));
    }
    np[m] = pn;
    dp[m] = pd;
    pre[m] = acc;
    acc = gl_mul(acc, pd);
  }
  gl_t inv = gl_inv(acc);
  gl_t *cp = a.cp + ((size_t)bk * n + i) * nch;
  for (uint32_t m = MAX_CHUNKS; m-- > 0;) {
    if (m >= nch) continue;
    cp[m] = gl_mul(np[m], gl_mul(inv, pre[m]));
    inv = gl_mul(inv, dp[m]);
  }
}
// block per (proof, challenge): the running product over the rows; lds: nt words
P2_HD void zs_scan(const Args &a, uint32_t bk, uint32_t tid, uint32_t nt, gl_t *lds) {
  const uint32_t d = a.c.d, n = 1u << d, K = a.c.K, nch = a.c.nchunks, PP = a.c.PP;
  const uint32_t b = bk / K, k = bk - b * K, seg = (n + nt - 1) / nt;
  const gl_t *cp = a.cp + (size_t)bk * n * nch;
  gl_t *zp = a.zp_vals + ((size_t)b * a.L.nzp << d);
  const uint32_t i0 = tid * seg < n ? tid * seg : n, i1 = i0 + seg < n ? i0 + seg : n;
  gl_t p = 1;
  for (uint32_t i = i0; i < i1; i++)
    for (uint32_t m = 0; m < nch; m++) p = gl_mul(p, cp[(size_t)i * nch + m]);
  lds[tid] = p;
  PB_SYNC();
  if (tid == 0) {
    gl_t run = 1;
    for (uint32_t t = 0; t < nt; t++) {
      const gl_t v = lds[t];
      lds[t] = run;
      run = gl_mul(run, v);
    }
  }
  PB_SYNC();
  gl_t z = lds[tid];
  for (uint32_t i = i0; i < i1; i++) {
    zp[((size_t)k << d) + i] = z;
    for (uint32_t m = 0; m < nch; m++) {
      z = gl_mul(z, cp[(size_t)i * nch + m]);
      if (m < PP) zp[((size_t)(K + k * PP + m) << d) + i] = z;
    }
  }
}

// ---- quotient ---------------------------------------------------------------------------------------------------------------------
// the constraints of one gate, folded with the alpha powers of each challenge as they come (any u64 congruent to a constraint is
// taken: BaseOps::mul_out)
struct Fold {
  const gl_t *ap0, *ap1;
  gl_t acc0, acc1;
  uint32_t t;
  P2_HD void emit(gl_t c) {
    acc0 = gl_add(acc0, gl_mul(c, ap0[t]));
    if (ap1) acc1 = gl_add(acc1, gl_mul(c, ap1[t]));
    t++;
  }
};
// lane per (proof, LDE point): every term, folded, divided by Z_H -> qv [B][K][C][n]
P2_HD void quotient_body(const Args &a, uint32_t g) {
  const uint32_t d = a.c.d, n = 1u << d, rb = a.c.rate_bits, lgN = d + rb, K = a.c.K, R = a.c.R, QF = a.c.QF, nch = a.c.nchunks, PP = a.c.PP;
  const uint32_t b = g >> lgN, i = g & ((1u << lgN) - 1), k = i >> rb, r = i & ((1u << rb) - 1), W = a.c.W, nzp = a.L.nzp;
  const Record &rec = a.rec[b];
  const gl_t sr = a.scale[((size_t)r << d) + (n >> 1)];  // g w_N^r
  const gl_t x = gl_mul(sr, k < n / 2 ? a.tw_fwd[k] : gl_neg(a.tw_fwd[k - n / 2]));
  gl_t xn = sr;
  for (uint32_t q = 0; q < d; q++) xn = gl_sqr(xn);
  const gl_t zh = gl_sub(xn, 1);
  const gl_t inv = gl_inv(gl_mul(zh, gl_mul((gl_t)n, gl_sub(x, 1))));  // 1 / (Z_H n (x - 1))
  const gl_t zhi = gl_mul(inv, gl_mul((gl_t)n, gl_sub(x, 1))), l0 = gl_mul(gl_mul(zh, zh), inv);
  const size_t N = (size_t)1 << lgN;
  const gl_t *wrow = a.o[1].rows + ((size_t)b * N + bitrev32(i, lgN)) * W;
  const gl_t *zrow = a.o[2].rows + ((size_t)b * N + bitrev32(i, lgN)) * nzp;
  const gl_t *znext = a.o[2].rows + ((size_t)b * N + bitrev32((i + (1u << rb)) & (uint32_t)(N - 1), lgN)) * nzp;
  const gl_t *ap = a.apow + (size_t)b * K * a.nterms;
  gl_t tot[vc::VC_MAX_CHALLENGES] = {0, 0};
  uint32_t t = 0;
  for (uint32_t c = 0; c < K; c++, t++)
    for (uint32_t cc = 0; cc < K; cc++) tot[cc] = gl_add(tot[cc], gl_mul(gl_mul(l0, gl_sub(zrow[c], 1)), ap[cc * a.nterms + t]));
  for (uint32_t c = 0; c < K; c++)
    for (uint32_t m = 0; m < nch; m++, t++) {
      const gl_t prev = m == 0 ? zrow[c] : zrow[K + c * PP + m - 1];
      const gl_t next = m == nch - 1 ? znext[c] : zrow[K + c * PP + m];
      gl_t pn = 1, pd = 1;
      for (uint32_t jx = m * QF; jx < (m + 1) * QF && jx < R; jx++) {
        const gl_t wg = gl_add(wrow[jx], rec.gammas[c]);
        pn = gl_mul(pn, gl_add(wg, gl_mul(rec.betas[c], gl_mul(a.c.k_is[jx], x))));
        pd = gl_mul(pd, gl_add(wg, gl_mul(rec.betas[c], cs_at(a, r, k, a.c.NC + jx))));
      }
      const gl_t term = gl_sub(gl_mul(prev, pn), gl_mul(next, pd));
      for (uint32_t cc = 0; cc < K; cc++) tot[cc] = gl_add(tot[cc], gl_mul(term, ap[cc * a.nterms + t]));
    }
  auto Wf = [&](uint32_t col) { return wrow[col]; };
  auto LC = [&](uint32_t ci) { return cs_at(a, r, k, a.c.num_selectors + ci); };
  for (uint32_t gi = 0; gi < a.c.num_gates; gi++) {
    const GateDesc gd = a.c.gates[gi];
    if (!gd.num_constraints) continue;
    const gl_t f = gate_filter<BaseOps>(gd, gi, a.c.num_selectors, cs_at(a, r, k, gd.sel_index));
    Fold out{ap + t, K > 1 ? ap + a.nterms + t : nullptr, 0, 0, 0};
    eval_gate<BaseOps, true>(gd, Wf, LC, rec.pih, a.c.prc, out);
    tot[0] = gl_add(tot[0], gl_mul(f, out.acc0));
    if (K > 1) tot[1] = gl_add(tot[1], gl_mul(f, out.acc1));
  }
  for (uint32_t c = 0; c < K; c++) a.qv[(((((size_t)b * K + c) << rb) + r) << d) + k] = gl_mul(tot[c], zhi);
}
// block per (proof, challenge, coset): the coset's interpolant, in place; lds: n words
P2_HD void quotient_intt(const Args &a, uint32_t blk, uint32_t tid, uint32_t nt, gl_t *lds) {
  const uint32_t d = a.c.d, n = 1u << d, r = blk & ((1u << a.c.rate_bits) - 1);
  gl_t *v = a.qv + ((size_t)blk << d);
  to_coeffs(a, v, lds, d, tid, nt);
  for (uint32_t i = tid; i < n; i += nt) v[i] = gl_mul(lds[i], a.inv_scale[((size_t)r << d) + bitrev32(i, d)]);
}
// lane per (proof, challenge, coefficient): Q_m = g^(-n m) / C sum_r w_C^(-r m) P_r, the chunk polynomials
P2_HD void quotient_chunks(const Args &a, uint32_t g) {
  const uint32_t d = a.c.d, n = 1u << d, rb = a.c.rate_bits, C = 1u << rb, QF = a.c.QF, K = a.c.K;
  const uint32_t jx = g & (n - 1), bk = g >> d, b = bk / K, k = bk - b * K;
  const gl_t *P = a.qv + (((size_t)bk << rb) << d) + jx;
  const gl_t wi = gl_inv(gl_root(rb)), gni = gl_inv(gl_pow(GL_GEN, n)), ci = gl_inv((gl_t)C);
  gl_t wm = 1, gm = ci;  // w_C^-m, g^(-n m) / C
  for (uint32_t m = 0; m < QF && m < C; m++) {
    gl_t acc = 0, wr = 1;
    for (uint32_t r = 0; r < C; r++) {
      acc = gl_add(acc, gl_mul(P[(size_t)r << d], wr));
      wr = gl_mul(wr, wm);
    }
    a.o[3].coef[(((size_t)b * a.L.nq + k * QF + m) << d) + jx] = gl_mul(acc, gm);
    wm = gl_mul(wm, wi);
    gm = gl_mul(gm, gni);
  }
}

// ---- openings and the FRI polynomial -------------------------------------------------------------------------------------------------
// coefficient p of column jx of the four oracles together
P2_HD gl_t coef_at(const Args &a, uint32_t b, uint32_t jx, uint32_t p) {
  const uint32_t d = a.c.d;
  if (jx < a.L.ncs) return a.cs_coef[((size_t)jx << d) + bitrev32(p, d)];
  jx -= a.L.ncs;
  for (int o = 1; o < 4; o++) {
    if (jx < a.o[o].cols) return a.o[o].coef[(((size_t)b * a.o[o].cols + jx) << d) + p];
    jx -= a.o[o].cols;
  }
  return 0;
}
// lane per (proof, opening): the column at zeta; the K columns of Z at g zeta behind them
P2_HD void open_body(const Args &a, uint32_t g) {
  const uint32_t nall = a.L.nall, tot = nall + a.c.K, b = g / tot, jx = g - b * tot, n = 1u << a.c.d;
  const Record &r = a.rec[b];
  const ext_t z = jx < nall ? r.zeta : r.g_zeta;
  const uint32_t col = jx < nall ? jx : a.L.ncs + a.c.W + (jx - nall);
  ext_t acc = ext_from(0);
  for (uint32_t p = n; p-- > 0;) acc = ext_add(ext_mul(acc, z), ext_from(coef_at(a, b, col, p)));
  a.op[g] = acc;
}
// lane per (proof, coefficient): F0 = sum_j alpha^j column_j, F1 = sum_k alpha^k Z_k
P2_HD void reduce_body(const Args &a, uint32_t g) {
  const uint32_t d = a.c.d, n = 1u << d, b = g >> d, p = g & (n - 1), nall = a.L.nall;
  const ext_t *ea = a.eapow + (size_t)b * nall;
  ext_t a0 = ext_from(0), a1 = ext_from(0);
  for (uint32_t jx = 0; jx < nall; jx++) a0 = ext_add(a0, ext_scale(ea[jx], coef_at(a, b, jx, p)));
  for (uint32_t k = 0; k < a.c.K; k++) a1 = ext_add(a1, ext_scale(ea[k], coef_at(a, b, a.L.ncs + a.c.W + k, p)));
  a.f01[((size_t)b * 2 << d) + p] = a0;
  a.f01[(((size_t)b * 2 + 1) << d) + p] = a1;
}
// lane per (proof, which): divide_by_linear, q[j - 1] = c[j] + z q[j], remainder dropped.  In place: q[j - 1] takes the place
// of c[j], which is spent
P2_HD void divide_body(const Args &a, uint32_t g) {
  const uint32_t d = a.c.d, n = 1u << d, b = g >> 1;
  const ext_t z = (g & 1) ? a.rec[b].g_zeta : a.rec[b].zeta;
  ext_t *f = a.f01 + ((size_t)g << d);
  ext_t acc = ext_from(0);
  for (uint32_t jx = n; jx-- > 1;) {
    acc = ext_add(ext_mul(acc, z), f[jx]);
    f[jx] = acc;
  }
}
// lane per (proof, coefficient): alpha^K q0 + q1 -> the first FRI polynomial (coefficient j of it is f[j + 1] after divide_body)
P2_HD void combine_body(const Args &a, uint32_t g) {
  const uint32_t d = a.c.d, n = 1u << d, b = g >> d, jx = g & (n - 1);
  ext_t v = ext_from(0);
  if (jx + 1 < n) {
    const ext_t q0 = a.f01[((size_t)b * 2 << d) + jx + 1], q1 = a.f01[(((size_t)b * 2 + 1) << d) + jx + 1];
    v = ext_add(ext_mul(a.rec[b].alpha_k, q0), q1);
  }
  gl_t *out = a.fri_coef[0] + ((size_t)b * 2 << d);
  out[jx] = v.c0;
  out[n + jx] = v.c1;
}
// lane per (proof, coefficient of the folded polynomial)
P2_HD void fold_body(const Args &a, uint32_t g) {
  const uint32_t s = a.j.step, ab = a.c.arity[s], lg = fri_lg(a, s), lg2 = lg - ab, n2 = 1u << lg2, nn = 1u << lg;
  const uint32_t b = g >> lg2, m = g & (n2 - 1);
  const gl_t *in = a.fri_coef[s] + ((size_t)b * 2 << lg);
  const ext_t beta = a.rec[b].fri_beta[s];
  ext_t acc = ext_from(0);
  for (uint32_t q = 1u << ab; q-- > 0;) acc = ext_add(ext_mul(acc, beta), ext_make(in[(m << ab) + q], in[nn + (m << ab) + q]));
  gl_t *out = a.fri_coef[s + 1] + ((size_t)b * 2 << lg2);
  out[m] = acc.c0;
  out[n2 + m] = acc.c1;
}

// ---- the proof bytes -----------------------------------------------------------------------------------------------------------------
// lane per proof: everything outside the query section
P2_HD void write_head(const Args &a, uint32_t b) {
  const vc::Layout &L = a.L;
  const Record &r = a.rec[b];
  uint8_t *p = a.proofs + (size_t)b * a.want8;
  const uint32_t K = a.c.K, ncap = L.ncap, hb = L.hb, front = L.ncs + a.c.W + K;
  for (uint32_t o = 1; o < 4; o++) {
    const dig_t *cap = a.o[o].dig + (size_t)b * tree_size(L.lgN) + level_off(L.lgN, L.lgN - a.c.cap_h);
    for (uint32_t i = 0; i < ncap; i++) put_dig(p, ((size_t)(o - 1) * ncap + i) * hb, cap[i], hb);
  }
  // OpeningSet: constants, sigmas, wires, zs, zs_next, partial products, quotient
  const ext_t *op = a.op + (size_t)b * (L.nall + K);
  for (uint32_t jx = 0; jx < L.nall + K; jx++) {
    const uint32_t pos = jx < front ? jx : (jx < L.nall ? jx + K : front + (jx - L.nall));
    put64(p, L.open_at + 16 * (size_t)pos, op[jx].c0);
    put64(p, L.open_at + 16 * (size_t)pos + 8, op[jx].c1);
  }
  for (uint32_t s = 0; s < a.c.n_steps; s++) {
    const uint32_t lgl = fri_lg(a, s) + a.c.rate_bits - a.c.arity[s];
    const dig_t *cap = a.fri_dig[s] + (size_t)b * tree_size(lgl) + level_off(lgl, lgl - a.c.cap_h);
    for (uint32_t i = 0; i < ncap; i++) put_dig(p, L.step_caps_at + ((size_t)s * ncap + i) * hb, cap[i], hb);
  }
  const uint32_t lgf = fri_lg(a, a.c.n_steps), nf = 1u << lgf;
  const gl_t *f = a.fri_coef[a.c.n_steps] + ((size_t)b * 2 << lgf);
  for (uint32_t i = 0; i < nf; i++) {
    put64(p, L.tail_at + 16 * (size_t)i, f[i]);
    put64(p, L.tail_at + 16 * (size_t)i + 8, f[nf + i]);
  }
  put64(p, L.pow_at, r.pow_witness);
  for (uint32_t i = 0; i < a.c.num_pi; i++) put64(p, L.pis_at + 8 * (size_t)i, a.pis[(size_t)b * a.c.num_pi + i]);
}
// lane per (proof, query, part): part o < 4 the opening of initial oracle o, part 4 + s that of fold step s
P2_HD void write_query(const Args &a, uint32_t g) {
  const vc::Layout &L = a.L;
  const uint32_t parts = 4 + a.c.n_steps, part = g % parts, bq = g / parts, q = bq % a.c.num_queries, b = bq / a.c.num_queries;
  const uint32_t hb = L.hb, x0 = a.rec[b].qidx[q];
  uint8_t *p = a.proofs + (size_t)b * a.want8;
  if (part == 0) {
    uint32_t k;
    const uint32_t r = leaf_coset(a, x0, &k), d = a.c.d;
    size_t at = L.leaf_at(q, 0);
    for (uint32_t col = 0; col < L.ncs; col++, at += 8) put64(p, at, cs_at(a, r, k, col));
    p[at++] = (uint8_t)L.init_len;
    for (uint32_t l = 0; l < L.init_len; l++, at += hb) {
      const uint32_t m = (1u << d) >> l, sib = (k & (m - 1)) ^ (m >> 1);
      put_dig(p, at, a.cs_dig[a.cs_level_off[l] + (size_t)r * m + sib], hb);
    }
    return;
  }
  const gl_t *leaf;
  const dig_t *dig;
  uint32_t words, lgl, index;
  size_t at;
  if (part < 4) {
    const Oracle &o = a.o[part];
    words = o.cols; lgl = L.lgN; index = x0;
    leaf = o.rows + (((size_t)b << L.lgN) + x0) * o.cols;
    dig = o.dig + (size_t)b * tree_size(lgl);
    at = L.leaf_at(q, part);
  } else {
    const uint32_t s = part - 4;
    uint32_t shift = 0;
    for (uint32_t i = 0; i <= s; i++) shift += a.c.arity[i];
    const uint32_t lgrows = fri_lg(a, s) + a.c.rate_bits;
    words = 2u << a.c.arity[s]; lgl = lgrows - a.c.arity[s]; index = x0 >> shift;
    leaf = a.fri_rows[s] + (((size_t)b << lgrows) * 2) + (size_t)index * words;
    dig = a.fri_dig[s] + (size_t)b * tree_size(lgl);
    at = L.vals_at(q, s);
  }
  for (uint32_t w = 0; w < words; w++, at += 8) put64(p, at, leaf[w]);
  const uint32_t levels = lgl - a.c.cap_h;
  p[at++] = (uint8_t)levels;
  for (uint32_t l = 0; l < levels; l++, at += hb) put_dig(p, at, dig[level_off(lgl, l) + ((index >> l) ^ 1)], hb);
}

// ---- the slab's buffers ---------------------------------------------------------------------------------------------------------------
// Every buffer of a slab of B proofs, through take(bytes) -> pointer (null: none left); with a counting `take` the same walk
// gives the bytes a slab needs.  a.c, a.L and a.nterms are set; a.wires is the caller's.
template <class TAKE>
bool slab_buffers(Args &a, uint32_t B, TAKE &take) {
  const uint32_t d = a.c.d, rb = a.c.rate_bits, lgN = d + rb, K = a.c.K;
  const size_t n = (size_t)1 << d, N = (size_t)1 << lgN;
  bool ok = true;
  auto get = [&](auto *&p, size_t count) {
    typedef typename std::remove_reference<decltype(*p)>::type T;
    p = (T *)take((count ? count : 1) * sizeof(T));
    ok = ok && p;
  };
  a.B = B;
  a.want8 = (a.L.want + 7) & ~(size_t)7;
  gl_t *pis = nullptr;
  get(pis, (size_t)B * a.c.num_pi);
  a.pis = pis;
  get(a.rec, B);
  get(a.apow, (size_t)B * K * a.nterms);
  get(a.eapow, (size_t)B * a.L.nall);
  get(a.op, (size_t)B * (a.L.nall + K));
  get(a.terms, (size_t)B * vc::identity_terms(a.c));
  get(a.zp_vals, (size_t)B * a.L.nzp * n);
  get(a.cp, (size_t)B * K * n * a.c.nchunks);
  a.o[0] = Oracle{nullptr, nullptr, nullptr, a.L.ncs};
  for (int o = 1; o < 4; o++) {
    a.o[o].cols = a.L.cols[o];
    get(a.o[o].coef, (size_t)B * a.L.cols[o] * n);
    get(a.o[o].rows, (size_t)B * a.L.cols[o] * N);
    get(a.o[o].dig, (size_t)B * tree_size(lgN));
  }
  get(a.qv, (size_t)B * K * N);
  get(a.f01, (size_t)B * 2 * n);
  uint32_t lg = d;
  for (uint32_t s = 0; s <= a.c.n_steps; s++) {
    get(a.fri_coef[s], ((size_t)B * 2) << lg);
    if (s == a.c.n_steps) break;
    get(a.fri_rows[s], ((size_t)B * 2) << (lg + rb));
    get(a.fri_dig[s], (size_t)B * tree_size(lg + rb - a.c.arity[s]));
    lg -= a.c.arity[s];
  }
  get(a.proofs, (size_t)B * a.want8);
  return ok;
}

// ---- the sequence ---------------------------------------------------------------------------------------------------------------------
// One slab: every launch, in order.  RUN::lanes<F>(args, items, name) runs F(args, item) for every item; RUN::blocks<F>(args,
// blocks, threads, lds_words, name) runs F(args, block, thread, threads, lds) for every thread of every block.
template <int HK, class RUN>
void prove_slab(RUN &run, const Args &base) {
  Args a = base;
  const uint32_t B = a.B, d = a.c.d, n = 1u << d, rb = a.c.rate_bits, lgN = d + rb, K = a.c.K;
  const uint32_t nt = n / 2 < 256 ? (n / 2 ? n / 2 : 1) : 256;
  auto commit = [&](int o, bool from_values, const gl_t *src) {
    const Oracle &ob = a.o[o];
    a.j.src = src; a.j.src_stride = (size_t)ob.cols << d; a.j.coef_out = from_values ? ob.coef : nullptr;
    a.j.rows = ob.rows; a.j.cols = ob.cols; a.j.lg = d; a.j.shift_lg = 0; a.j.from_values = from_values;
    run.template blocks<lde_body>(a, B * ob.cols, nt, 2 * n, "pb_lde");
    a.j.leaf_src = ob.rows; a.j.leaf_stride = ((size_t)ob.cols) << lgN; a.j.leaf_len = ob.cols; a.j.lg_leaves = lgN; a.j.dig = ob.dig;
    run.template lanes<leaf_body<HK>>(a, B << lgN, "pb_leaves");
    run.template blocks<tree_body<HK>>(a, B << a.c.cap_h, 64, 0, "pb_tree");
  };
  commit(1, true, a.wires);
  run.template lanes<t_wires<HK>>(a, B, "pb_t_wires");
  run.template lanes<zs_chunks>(a, (B * K) << d, "pb_zs_chunks");
  run.template blocks<zs_scan>(a, B * K, nt, nt, "pb_zs_scan");
  commit(2, true, a.zp_vals);
  run.template lanes<t_zs<HK>>(a, B, "pb_t_zs");
  run.template lanes<quotient_body>(a, B << lgN, "pb_quotient");
  run.template blocks<quotient_intt>(a, (B * K) << rb, nt, n, "pb_quotient_intt");
  run.template lanes<quotient_chunks>(a, (B * K) << d, "pb_quotient_chunks");
  commit(3, false, a.o[3].coef);
  run.template lanes<t_quotient<HK>>(a, B, "pb_t_quotient");
  run.template lanes<open_body>(a, B * (a.L.nall + K), "pb_open");
  run.template lanes<t_openings<HK>>(a, B, "pb_t_openings");
  run.template lanes<reduce_body>(a, B << d, "pb_reduce");
  run.template lanes<divide_body>(a, B * 2, "pb_divide");
  run.template lanes<combine_body>(a, B << d, "pb_combine");
  uint32_t lg = d, shift_lg = 0;
  for (uint32_t s = 0; s < a.c.n_steps; s++) {
    const uint32_t ab = a.c.arity[s], ns = 1u << lg;
    a.j.step = s;
    a.j.src = a.fri_coef[s]; a.j.src_stride = (size_t)2 << lg; a.j.coef_out = nullptr; a.j.rows = a.fri_rows[s];
    a.j.cols = 2; a.j.lg = lg; a.j.shift_lg = shift_lg; a.j.from_values = 0;
    run.template blocks<lde_body>(a, B * 2, ns / 2 < 256 ? (ns / 2 ? ns / 2 : 1) : 256, 2 * ns, "pb_lde");
    a.j.leaf_src = a.fri_rows[s]; a.j.leaf_stride = (size_t)2 << (lg + rb); a.j.leaf_len = 2u << ab; a.j.lg_leaves = lg + rb - ab;
    a.j.dig = a.fri_dig[s];
    run.template lanes<leaf_body<HK>>(a, B << a.j.lg_leaves, "pb_leaves");
    run.template blocks<tree_body<HK>>(a, B << a.c.cap_h, 64, 0, "pb_tree");
    run.template lanes<t_step<HK>>(a, B, "pb_t_step");
    run.template lanes<fold_body>(a, B << (lg - ab), "pb_fold");
    lg -= ab;
    shift_lg += ab;
  }
  run.template lanes<t_final<HK>>(a, B, "pb_t_final");
  a.j.cols = run.pow_groups();
  run.template blocks<pow_body<HK>>(a, B * a.j.cols, run.pow_threads(), 0, "pb_pow");
  run.template lanes<t_queries<HK>>(a, B, "pb_t_queries");
  run.template lanes<write_head>(a, B, "pb_write_head");
  run.template lanes<write_query>(a, B * a.c.num_queries * (4 + a.c.n_steps), "pb_write_query");
}

}  // namespace pb
}  // namespace p2
