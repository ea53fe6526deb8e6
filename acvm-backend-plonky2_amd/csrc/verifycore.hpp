// verifycore.hpp -- the checks of a plonky2 0.2.2 verifier (plonk/verifier.rs verify_with_challenges, fri/verifier.rs
// verify_fri_proof), once, for the host and for the device: p2gpu_verify (verify.hip), the host loop of
// p2gpu_verify_batch_host and the kernels of p2gpu_verify_batch (verifydev.hip) all run the functions of this file.
//   verify_head   per proof:            canonicity of every field element in a fixed position, the public-input hash, the
//                                       transcript, zeta^n != 1, the plonk identity at zeta, the proof-of-work bits; leaves a
//                                       HeadRecord (challenges, reduced openings, query indices) behind
//   verify_query  per proof and query:  the four initial Merkle paths, the combined quotient value, every fold, the final
//                                       polynomial at the folded point
// Both return a reason code (0: passed); reason_text() below holds the wording of every code, once.  Their parts that the proof
// formats need too (proofio.hip) have names of their own: well_formed, head_challenges, query_initial, fold_step.
// The prover (prover.hip) writes what these functions read: its Fiat-Shamir transcript is Transcript<HK> below, it serialises
// against make_layout (digest width `hb`, finished length `want` = p2gpu_proof_size_bound), and the handle's circuit digest is
// leaf_digest_at<HK> (handle.hip, through hostproof.hpp) -- one statement of hasher, transcript and layout for both sides.
//
// WHAT NO PROOF BYTE CAN DO: move a read.  The length of a proof is fixed by its circuit (make_layout: `want`), and a proof
// of another length never reaches these functions (shape_reason answers for it).  After that every read of the proof is at
// an offset make_layout computed from the circuit alone -- caps, openings, step caps, final polynomial, PoW witness and public
// inputs at fixed positions; inside query q, at queries_at + q * query_bytes, the four initial openings and the fold steps at
// fixed positions too: the path-length bytes are COMPARED with the length the circuit fixes, never used as one.  The only
// value of the proof (of the transcript, that is) that enters an address is a query index, masked to N - 1 before anything
// uses it: it selects a cap entry (index >> (lgN - cap_h) < 2^cap_h entries, the size of every cap) and a slot of a fold leaf
// (masked to the arity).  So every read lies in [0, want); ld64() on the device reads the aligned words that cover its eight
// bytes, i.e. within [0, want rounded up to 8) from an 8-aligned base, which is how verifydev.hip uploads a batch.
// No std::vector, no cursor, no thread-local hasher: the hasher is the template parameter HK (0 KeccakHash<25>, 1
// PoseidonHash).  Arrays a lane would index at run time are not on its stack: the transcript state and the constraint terms
// live in caller-provided scratch (Strided: element i of lane b at [i * lanes + b] on the device), the rest is read from the
// proof where it lies.
#pragma once
#include "gates.hpp"
#include "keccak.hpp"
#include <cstdio>
#include <cstring>

// The long pieces -- a transcript step (a sponge permutation inside), a leaf hash, a Merkle walk, the plonk identity -- are
// real functions, not inlined into each of their many call sites: one copy per hasher in a translation unit, on the host and
// on the device (P2_HD alone would paste a Keccak-f or a Poseidon permutation into every observe() of verify_head).
#if defined(__HIPCC__)
#define VC_FN __host__ __device__ inline __attribute__((noinline))
#else
#define VC_FN inline __attribute__((noinline))
#endif

namespace p2 {
namespace vc {

// ---- reasons ---------------------------------------------------------------------------------------------------------
// one per reject site of the verifier, in its order
enum : uint32_t {
  VR_OK = 0,
  VR_HEADER = 1,        // truncated or non-canonical header
  VR_ARITY = 2,         // the circuit's reduction arities do not fit its size
  VR_LENGTH = 3,        // a = length given, b = length the circuit fixes
  VR_TAIL = 4,          // non-canonical final polynomial / PoW witness / public input
  VR_ZETA = 5,
  VR_IDENTITY = 6,
  VR_POW = 7,
  VR_Q_INIT_SHAPE = 8,  // a = query, b = oracle
  VR_Q_LEAF = 9,        // a = query
  VR_Q_INIT_PATH = 10,  // a = query, b = oracle
  VR_Q_STEP_SHAPE = 11, // a = query, b = step
  VR_Q_FOLD = 12,       // a = query, b = step
  VR_Q_STEP_PATH = 13,  // a = query, b = step
  VR_Q_FINAL = 14,      // a = query
  VR_Q_SIZE = 15,
  VR_COUNT
};
constexpr uint32_t VR_NONE = 0xFFFFFFFFu;  // "names no query / oracle / step"

// The wording behind "proof rejected: ".  Returns what snprintf returns.
inline int reason_text(uint32_t reason, size_t a, size_t b, char *out, size_t cap) {
  switch (reason) {
  case VR_OK: return snprintf(out, cap, "accepted");
  case VR_HEADER: return snprintf(out, cap, "truncated or non-canonical header (caps / openings)");
  case VR_ARITY: return snprintf(out, cap, "bad reduction arity in circuit");
  case VR_LENGTH: return snprintf(out, cap, "length %zu, expected %zu for this circuit", a, b);
  case VR_TAIL: return snprintf(out, cap, "non-canonical field element in final polynomial / public inputs");
  case VR_ZETA: return snprintf(out, cap, "zeta lies in the subgroup");
  case VR_IDENTITY: return snprintf(out, cap, "vanishing(zeta) != Z_H(zeta) * quotient(zeta)");
  case VR_POW: return snprintf(out, cap, "proof-of-work response has too few leading zeros");
  case VR_Q_INIT_SHAPE: return snprintf(out, cap, "query %u: malformed initial opening %d", (unsigned)a, (int)b);
  case VR_Q_LEAF: return snprintf(out, cap, "query %u: non-canonical leaf element", (unsigned)a);
  case VR_Q_INIT_PATH: return snprintf(out, cap, "query %u: Merkle path of initial oracle %d does not lead to its cap", (unsigned)a, (int)b);
  case VR_Q_STEP_SHAPE: return snprintf(out, cap, "query %u: malformed fold step %u", (unsigned)a, (unsigned)b);
  case VR_Q_FOLD: return snprintf(out, cap, "query %u: fold step %u does not continue the previous value", (unsigned)a, (unsigned)b);
  case VR_Q_STEP_PATH: return snprintf(out, cap, "query %u: Merkle path of fold step %u does not lead to its cap", (unsigned)a, (unsigned)b);
  case VR_Q_FINAL: return snprintf(out, cap, "query %u: final polynomial disagrees with the folded value", (unsigned)a);
  case VR_Q_SIZE: return snprintf(out, cap, "query section has the wrong size");
  }
  return snprintf(out, cap, "unknown reason %u", reason);
}

// ---- the verifier's share of a circuit, flat ---------------------------------------------------------------------------
// The pointers are in the memory of whoever runs the functions below.
constexpr uint32_t VC_MAX_STEPS = 8, VC_MAX_QUERIES = 64, VC_MAX_CHALLENGES = 2;
struct CircuitView {
  uint32_t d, W, R, NC, num_selectors, K, QF, PP, nchunks, rate_bits, cap_h, pow_bits, num_queries, n_steps, arity[VC_MAX_STEPS];
  uint32_t num_gates, num_pi, max_gate_constraints, hasher;
  const GateDesc *gates;  // [num_gates]
  const gl_t *k_is;       // [R]
  const dig_t *cs_cap;    // [2^cap_h] the constants_sigmas cap
  const gl_t *prc;        // [360] Poseidon round constants, poseidon_device_constants form (the gate's and, equally, the permutation's)
  dig_t circuit_digest;
};

// every offset of a proof of the circuit: caps | openings | step caps | queries | final polynomial | PoW | public inputs
struct Layout {
  uint32_t hb;          // bytes of a digest: 25 or 32
  uint32_t ncs, nzp, nq, nall, lgN, ncap;
  uint32_t cols[4];     // columns of the four initial oracles: constants_sigmas, wires, zs | partial products, quotient
  uint32_t init_len;    // siblings of an initial path: lgN - cap_h
  uint32_t step_lg[VC_MAX_STEPS];  // log2 of the domain a step folds
  size_t open_at, step_caps_at, queries_at, query_bytes, tail_at, final_len, pow_at, pis_at, want;
  size_t init_at[4];             // inside a query: leaf | length byte | siblings, per oracle
  size_t step_at[VC_MAX_STEPS];  // inside a query: 2^arity values | length byte | siblings, per step
  uint32_t bad_arity;
  // inside the proof: query q's opening of oracle o (cols[o] words) or of fold step s (2^ab values) | length byte | siblings
  P2_HD size_t leaf_at(size_t q, uint32_t o) const { return queries_at + query_bytes * q + init_at[o]; }
  P2_HD size_t leaf_len_at(size_t q, uint32_t o) const { return leaf_at(q, o) + 8 * (size_t)cols[o]; }
  P2_HD size_t vals_at(size_t q, uint32_t s) const { return queries_at + query_bytes * q + step_at[s]; }
  P2_HD size_t vals_len_at(size_t q, uint32_t s, unsigned ab) const { return vals_at(q, s) + ((size_t)16 << ab); }
};

inline Layout make_layout(const CircuitView &c) {
  Layout L;
  memset(&L, 0, sizeof L);
  L.hb = c.hasher ? 32 : 25;
  L.ncs = c.NC + c.R;
  L.nzp = c.K * (1 + c.PP);
  L.nq = c.K * c.QF;
  L.nall = L.ncs + c.W + L.nzp + L.nq;
  L.lgN = c.d + c.rate_bits;
  L.ncap = 1u << c.cap_h;
  L.cols[0] = L.ncs; L.cols[1] = c.W; L.cols[2] = L.nzp; L.cols[3] = L.nq;
  L.init_len = L.lgN - c.cap_h;
  const size_t hb = L.hb;
  L.open_at = 3 * hb * (size_t)L.ncap;
  L.step_caps_at = L.open_at + 16 * (size_t)(L.nall + c.K);
  L.queries_at = L.step_caps_at + (size_t)c.n_steps * hb * L.ncap;
  size_t at = 0;
  for (int o = 0; o < 4; o++) {
    L.init_at[o] = at;
    at += 8 * (size_t)L.cols[o] + 1 + hb * (size_t)L.init_len;
  }
  L.final_len = (size_t)1 << c.d;
  unsigned lg = L.lgN;
  for (uint32_t s = 0; s < c.n_steps && s < VC_MAX_STEPS; s++) {
    const unsigned ab = c.arity[s];
    if (ab < 1 || ab > 4 || lg < ab + c.cap_h || (L.final_len >> ab) == 0) {
      L.bad_arity = 1;
      break;
    }
    L.step_lg[s] = lg;
    L.step_at[s] = at;
    lg -= ab;
    L.final_len >>= ab;
    at += ((size_t)16 << ab) + 1 + hb * (size_t)(lg - c.cap_h);
  }
  L.query_bytes = at;
  L.tail_at = L.queries_at + L.query_bytes * c.num_queries;
  L.pow_at = L.tail_at + 16 * L.final_len;
  L.pis_at = L.pow_at + 8;
  L.want = L.pis_at + 8 * (size_t)c.num_pi;
  return L;
}

// ---- reading the proof -------------------------------------------------------------------------------------------------
P2_HD uint64_t ld64(const uint8_t *p, size_t at) {
#if defined(__HIP_DEVICE_COMPILE__)
  const uintptr_t a = (uintptr_t)(p + at);
  const uint64_t *w = (const uint64_t *)(a & ~(uintptr_t)7);
  const unsigned sh = (unsigned)(a & 7) * 8;
  const uint64_t lo = w[0];
  if (sh == 0) return lo;
  return (lo >> sh) | (w[1] << (64 - sh));
#else
  uint64_t v;
  memcpy(&v, p + at, 8);
  return v;
#endif
}
P2_HD ext_t ld_ext(const uint8_t *p, size_t at) {
  const gl_t a = ld64(p, at), b = ld64(p, at + 8);
  return ext_make(a, b);
}
// are the `count` words at `at` canonical field elements
P2_HD bool canonical_words(const uint8_t *p, size_t at, size_t count) {
  bool ok = true;
  for (size_t i = 0; i < count; i++) ok &= ld64(p, at + 8 * i) < GL_P;
  return ok;
}

// element i of this lane's scratch
template <class T>
struct Strided {
  T *p;
  size_t stride;
  P2_HD T &operator[](size_t i) const { return p[i * stride]; }
};

// ---- the hasher HK ------------------------------------------------------------------------------------------------------
P2_HD void poseidon_permute_hd(gl_t st[12], const gl_t *prc) {
#if defined(__HIP_DEVICE_COMPILE__)
  poseidon_permute_dev(st, prc);
#else
  poseidon_permute_host(st, prc);
#endif
}
template <int HK>
P2_HD void sponge_permute(gl_t st[12], const gl_t *prc) {
  if constexpr (HK) poseidon_permute_hd(st, prc);
  else keccak_permutation12(st);
}
// a digest of the proof; *canon is cleared when a PoseidonHash word is no field element (w and w + p hash alike)
template <int HK>
P2_HD dig_t ld_digest(const uint8_t *p, size_t at, bool *canon) {
  dig_t d;
  d.w[0] = ld64(p, at);
  d.w[1] = ld64(p, at + 8);
  d.w[2] = ld64(p, at + 16);
  if constexpr (HK) {
    d.w[3] = ld64(p, at + 24);
    if (d.w[0] >= GL_P || d.w[1] >= GL_P || d.w[2] >= GL_P || d.w[3] >= GL_P) *canon = false;
  } else {
    d.w[3] = p[at + 24];
  }
  return d;
}
template <int HK>
P2_HD bool dig_same(const dig_t &a, const dig_t &b) {
  return a.w[0] == b.w[0] && a.w[1] == b.w[1] && a.w[2] == b.w[2] && (HK ? a.w[3] == b.w[3] : (a.w[3] & 0xFF) == (b.w[3] & 0xFF));
}
// H::hash_or_noop of the n field elements at `at`
template <int HK>
VC_FN dig_t leaf_digest_at(const uint8_t *p, size_t at, uint32_t n, const gl_t *prc) {
  dig_t d;
  d.w[0] = d.w[1] = d.w[2] = d.w[3] = 0;
  if (n <= (HK ? 4u : 3u)) {
    if (n > 0) d.w[0] = ld64(p, at);
    if (n > 1) d.w[1] = ld64(p, at + 8);
    if (n > 2) d.w[2] = ld64(p, at + 16);
    if (n > 3) d.w[3] = ld64(p, at + 24);
    return d;
  }
  if constexpr (HK) {
    gl_t st[12];
    for (int i = 0; i < 12; i++) st[i] = 0;
    for (uint32_t off = 0; off < n; off += 8) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t i = 0; i < 8; i++)
        if (off + i < n) st[i] = ld64(p, at + 8 * (size_t)(off + i));
      poseidon_permute_hd(st, prc);
    }
    for (int i = 0; i < 4; i++) d.w[i] = st[i];
    return d;
  } else {
    uint64_t st[25];
    for (int i = 0; i < 25; i++) st[i] = 0;
    uint32_t off = 0;
    while (n - off >= 17) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t i = 0; i < 17; i++) st[i] ^= ld64(p, at + 8 * (size_t)(off + i));
      keccak_f1600(st);
      off += 17;
    }
    const uint32_t rem = n - off;  // < 17: the padding 0x01 goes to word `rem`, 0x80 to the top of word 16
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
    for (uint32_t i = 0; i < 17; i++) {
      uint64_t v = 0;
      if (i < rem) v = ld64(p, at + 8 * (size_t)(off + i));
      else if (i == rem) v = 0x01ULL;
      st[i] ^= v;
    }
    st[16] ^= 0x8000000000000000ULL;
    keccak_f1600(st);
    return dig_from_state(st);
  }
}
template <int HK>
P2_HD dig_t node_digest_hk(const dig_t &l, const dig_t &r, const gl_t *prc) {
  if constexpr (HK) {
    gl_t st[12] = {l.w[0], l.w[1], l.w[2], l.w[3], r.w[0], r.w[1], r.w[2], r.w[3], 0, 0, 0, 0};
    poseidon_permute_hd(st, prc);
    dig_t d;
    for (int i = 0; i < 4; i++) d.w[i] = st[i];
    return d;
  } else {
    return keccak_two_to_one(l, r);
  }
}
// hash/merkle_proofs.rs verify_merkle_proof_to_cap, up to the cap: the digest `levels` siblings (at sib_at) above leaf digest
// `cur`; *canon is cleared by a sibling that is no PoseidonHash digest
template <int HK>
VC_FN dig_t merkle_walk(const uint8_t *p, const dig_t &leaf, size_t index, size_t sib_at, uint32_t levels, uint32_t hb, const gl_t *prc, bool *canon) {
  dig_t cur = leaf;
  for (uint32_t l = 0; l < levels; l++) {
    const dig_t s = ld_digest<HK>(p, sib_at + (size_t)hb * l, canon);
    const bool odd = index & 1;
    const dig_t left = odd ? s : cur, right = odd ? cur : s;
    cur = node_digest_hk<HK>(left, right, prc);
    index >>= 1;
  }
  return cur;
}

// ---- transcript (iop/challenger.rs): the sponge state in scratch, inputs written where duplexing would put them ------------
// (an observed element lands in state[n_in] at once: nothing reads the state between an observation and the next
// permutation, and the pending outputs are dropped by the observation either way)
template <int HK>
struct Transcript {
  Strided<gl_t> st;  // [12]
  const gl_t *prc;
  uint32_t n_in = 0, n_out = 0;
  P2_HD void init() {
    for (int i = 0; i < 12; i++) st[i] = 0;
  }
  P2_HD void duplex() {
    gl_t s[12];
    for (int i = 0; i < 12; i++) s[i] = st[i];
    sponge_permute<HK>(s, prc);
    for (int i = 0; i < 12; i++) st[i] = s[i];
    n_in = 0;
    n_out = 8;
  }
  VC_FN void observe(gl_t e) {
    n_out = 0;
    st[n_in++] = e;
    if (n_in == 8) duplex();
  }
  P2_HD void observe_digest(const dig_t &d) {
    gl_t e[4];
    if constexpr (HK) {
      for (int i = 0; i < 4; i++) e[i] = d.w[i];
    } else {
      dig_to_elems(d, e);
    }
    for (int i = 0; i < 4; i++) observe(e[i]);
  }
  P2_HD void observe_cap(const uint8_t *p, size_t at, uint32_t ncap, uint32_t hb) {
    bool canon = true;  // (checked before the transcript starts)
    for (uint32_t i = 0; i < ncap; i++) observe_digest(ld_digest<HK>(p, at + (size_t)hb * i, &canon));
  }
  P2_HD void observe_ext(ext_t e) {
    observe(e.c0);
    observe(e.c1);
  }
  VC_FN gl_t get() {
    if (n_in != 0 || n_out == 0) duplex();
    return st[--n_out];
  }
  P2_HD ext_t get_ext() {
    const gl_t a = get();
    const gl_t b = get();
    return ext_make(a, b);
  }
};

// ---- the plonk identity at zeta ------------------------------------------------------------------------------------------
// vanishing_c(zeta) == Z_H(zeta) * sum_m zeta^(n m) * t_{c,m}(zeta) for each challenge c (plonk/verifier.rs
// verify_with_challenges + vanishing_poly.rs eval_vanishing_poly over the extension).  op(j): opened value j in the PROVER's
// order -- constants, sigmas, wires, zs, partial products, quotient chunks, then zs_next; terms: K + K * nchunks +
// max_gate_constraints extension elements of scratch.  The prover's self-check runs this too (verify.hip plonk_identity_holds).
template <class TERMS>
struct GateSum {
  TERMS t;
  uint32_t base, cap, k;
  ext_t f;
  P2_HD void emit(ext_t c) {
    if (k < cap) t[base + k] = ext_add(t[base + k], ext_mul(f, c));
    k++;
  }
};
template <class OP, class TERMS>
P2_HD bool plonk_identity_core(const CircuitView &c, OP op, TERMS terms, const gl_t *betas, const gl_t *gammas, const gl_t *alphas, ext_t zeta,
                               const gl_t pih[4]) {
  const uint32_t K = c.K, R = c.R, W = c.W, NC = c.NC, QF = c.QF, PP = c.PP, nchunks = c.nchunks;
  const uint32_t ncs = NC + R, nzp = K * (1 + PP), nall = ncs + W + nzp + K * QF;
  const uint32_t o_sig = NC, o_wires = ncs, o_zs = ncs + W, o_pp = o_zs + K, o_quot = o_pp + K * PP, o_zs_next = nall;
  ext_t zn = zeta;
  for (uint32_t i = 0; i < c.d; i++) zn = ext_mul(zn, zn);
  const ext_t z_h = ext_sub(zn, ext_from(1));
  const ext_t l0 = ext_mul(z_h, ext_inv(ext_scale(ext_sub(zeta, ext_from(1)), (gl_t)1 << c.d)));
  uint32_t nt = 0;
  for (uint32_t k = 0; k < K; k++) terms[nt++] = ext_mul(l0, ext_sub(op(o_zs + k), ext_from(1)));
  for (uint32_t k = 0; k < K; k++)
    for (uint32_t m = 0; m < nchunks; m++) {
      const ext_t prev = m == 0 ? op(o_zs + k) : op(o_pp + k * PP + m - 1);
      const ext_t next = m == nchunks - 1 ? op(o_zs_next + k) : op(o_pp + k * PP + m);
      ext_t np = ext_from(1), dp = ext_from(1);
      for (uint32_t j = m * QF; j < (m + 1) * QF && j < R; j++) {
        const ext_t s_id = ext_scale(zeta, c.k_is[j]);
        const ext_t w = op(o_wires + j);
        np = ext_mul(np, ext_add(ext_add(w, ext_scale(s_id, betas[k])), ext_from(gammas[k])));
        dp = ext_mul(dp, ext_add(ext_add(w, ext_scale(op(o_sig + j), betas[k])), ext_from(gammas[k])));
      }
      terms[nt++] = ext_sub(ext_mul(prev, np), ext_mul(next, dp));
    }
  const uint32_t gate_base = nt, mgc = c.max_gate_constraints;
  for (uint32_t k = 0; k < mgc; k++) terms[gate_base + k] = ext_from(0);
  nt += mgc;
  ext_t pih_e[4];
  for (int i = 0; i < 4; i++) pih_e[i] = ext_from(pih[i]);
  auto Wf = [&](uint32_t col) { return op(o_wires + col); };
  auto LC = [&](uint32_t i) { return op(c.num_selectors + i); };
  for (uint32_t gi = 0; gi < c.num_gates; gi++) {
    const GateDesc g = c.gates[gi];
    if (!g.num_constraints) continue;
    GateSum<TERMS> out{terms, gate_base, mgc, 0, gate_filter<ExtOps>(g, gi, c.num_selectors, op(g.sel_index))};
    eval_gate<ExtOps, true>(g, Wf, LC, pih_e, c.prc, out);
  }
  bool holds = true;
  for (uint32_t k = 0; k < K; k++) {
    ext_t van = ext_from(0), qz = ext_from(0);
    for (uint32_t t = nt; t-- > 0;) van = ext_add(ext_scale(van, alphas[k]), terms[t]);
    for (uint32_t m = QF; m-- > 0;) qz = ext_add(ext_mul(qz, zn), op(o_quot + k * QF + m));
    holds &= ext_eq(van, ext_mul(z_h, qz));
  }
  return holds;
}
// The opened values wherever they are: an array in the prover's order (its self-check), or the proof, which serialises
// constants, sigmas, wires, zs, zs_next, partial products, quotient.  One type, so that one copy of the identity serves both.
struct Openings {
  const ext_t *arr;  // non-null: arr[j]
  const uint8_t *p;  // else the proof, its openings at open_at
  size_t open_at;
  uint32_t front, nall, K;  // front: constants .. zs
  P2_HD ext_t operator()(uint32_t j) const {
    if (arr) return arr[j];
    const uint32_t pos = j < front ? j : (j < nall ? j + K : front + (j - nall));
    return ld_ext(p, open_at + 16 * (size_t)pos);
  }
};
// the opened values of proof p
P2_HD Openings proof_openings(const CircuitView &c, const Layout &L, const uint8_t *p) {
  return Openings{nullptr, p, L.open_at, L.nall - L.nq - L.nzp + c.K, L.nall, c.K};
}
VC_FN bool plonk_identity_at(const CircuitView &c, const Openings &op, Strided<ext_t> terms, const gl_t *betas, const gl_t *gammas, const gl_t *alphas,
                             ext_t zeta, const gl_t *pih) {
  return plonk_identity_core(c, op, terms, betas, gammas, alphas, zeta, pih);
}
P2_HD uint32_t identity_terms(const CircuitView &c) { return c.K + c.K * c.nchunks + c.max_gate_constraints; }

// Value at beta of the degree < a interpolant through (s g^j, y(j)), j < a = 2^ab, g of order a.
// The nodes are the roots of X^a - s^a, so the barycentric weights are x_j / (a s^a):
//   P(beta) = (beta^a - s^a) / (a s^a) * sum_j y_j x_j / (beta - x_j).
// (fri/verifier.rs compute_evaluation does the same interpolation with a generic routine.)
template <class Y>
P2_HD ext_t interpolate_coset_fn(gl_t s, unsigned ab, Y y_natural, ext_t beta) {
  const uint32_t a = 1u << ab;
  const gl_t g = gl_root(ab);
  gl_t sa = s;
  ext_t ba = beta;
  for (unsigned i = 0; i < ab; i++) {
    sa = gl_sqr(sa);
    ba = ext_mul(ba, ba);
  }
  ext_t acc = ext_from(0);
  gl_t x = s;
  for (uint32_t j = 0; j < a; j++) {
    const ext_t diff = ext_sub(beta, ext_from(x));
    if (diff.c0 == 0 && diff.c1 == 0) return y_natural(j);
    acc = ext_add(acc, ext_mul(ext_scale(y_natural(j), x), ext_inv(diff)));
    x = gl_mul(x, g);
  }
  const gl_t scale = gl_inv(gl_mul((gl_t)a, sa));
  return ext_mul(ext_scale(ext_sub(ba, ext_from(sa)), scale), acc);
}

// ---- per proof -----------------------------------------------------------------------------------------------------------
struct HeadRecord {
  ext_t zeta, alpha, alpha_k, g_zeta, opened0, opened1;  // opened0: the batch at zeta, opened1: Z at g zeta, reduced with alpha
  ext_t beta[VC_MAX_STEPS];
  uint32_t qidx[VC_MAX_QUERIES];
};

// caps (under PoseidonHash), openings and step caps, all before `avail`; false: truncated or non-canonical
template <int HK>
P2_HD bool header_canonical(const CircuitView &c, const Layout &L, const uint8_t *p, size_t avail) {
  if (avail < L.queries_at) return false;
  bool ok = canonical_words(p, L.open_at, 2 * (size_t)(L.nall + c.K));
  if constexpr (HK) {
    ok &= canonical_words(p, 0, 12 * (size_t)L.ncap);
    ok &= canonical_words(p, L.step_caps_at, 4 * (size_t)L.ncap * c.n_steps);
  }
  return ok;
}

// the verdict of a proof by its shape alone: VR_OK means "its length is the circuit's", and only then may verify_head and
// verify_query see it.  A header that is cut short or not canonical speaks before the length does.
template <int HK>
P2_HD uint32_t shape_reason(const CircuitView &c, const Layout &L, const uint8_t *p, size_t len) {
  if (!L.bad_arity && len == L.want) return VR_OK;  // (verify_head looks at the header)
  if (!header_canonical<HK>(c, L, p, len)) return VR_HEADER;
  return L.bad_arity ? VR_ARITY : VR_LENGTH;
}

// "These bytes are a proof of this circuit's shape", without cryptography: the length, and every check of verify_head and
// verify_query that needs no challenge -- what the proof formats (proofio.hip) ask before they take a proof apart.  The PoW
// witness is a u64 to them, so it alone may be no field element here (verify_head answers VR_TAIL for it).
template <int HK>
P2_HD bool well_formed(const CircuitView &c, const Layout &L, const uint8_t *p, size_t len) {
  if (L.bad_arity || len != L.want || !header_canonical<HK>(c, L, p, len)) return false;
  bool ok = canonical_words(p, L.tail_at, 2 * L.final_len) && canonical_words(p, L.pis_at, c.num_pi);
  for (uint32_t qi = 0; qi < c.num_queries; qi++) {
    for (uint32_t o = 0; o < 4; o++) {
      const size_t len_at = L.leaf_len_at(qi, o);
      ok &= p[len_at] == L.init_len && canonical_words(p, L.leaf_at(qi, o), L.cols[o]);
      if constexpr (HK) ok &= canonical_words(p, len_at + 1, 4 * (size_t)L.init_len);
    }
    for (uint32_t s = 0; s < c.n_steps; s++) {
      const uint32_t ab = c.arity[s], levels = L.step_lg[s] - ab - c.cap_h;
      const size_t len_at = L.vals_len_at(qi, s, ab);
      ok &= canonical_words(p, L.vals_at(qi, s), (size_t)2 << ab) && p[len_at] == levels;
      if constexpr (HK) ok &= canonical_words(p, len_at + 1, 4 * (size_t)levels);
    }
  }
  return ok;
}

// Steps 2 and 3 of verify_head: the public-input hash and the transcript.  Everything the transcript yields goes to betas,
// gammas, alphas ([VC_MAX_CHALLENGES] each), pih and *rec; returns the proof-of-work response.  Checks nothing: the header
// and the tail are read as they lie.
template <int HK>
P2_HD gl_t head_challenges(const CircuitView &c, const Layout &L, const uint8_t *p, Strided<gl_t> sponge, gl_t *betas, gl_t *gammas, gl_t *alphas,
                           gl_t pih[4], HeadRecord *rec) {
  const uint32_t K = c.K, nall = L.nall;
  for (uint32_t k = 0; k < VC_MAX_CHALLENGES; k++) betas[k] = gammas[k] = alphas[k] = 0;
  // 2. the public-input hash (hash_n_to_m_no_pad, PoseidonHash whatever the circuit's hasher is)
  {
    gl_t st[12];
    for (int i = 0; i < 12; i++) st[i] = 0;
    for (uint32_t off = 0; off < c.num_pi; off += 8) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
#endif
      for (uint32_t i = 0; i < 8; i++)
        if (off + i < c.num_pi) st[i] = ld64(p, L.pis_at + 8 * (size_t)(off + i));
      poseidon_permute_hd(st, c.prc);
    }
    for (int i = 0; i < 4; i++) pih[i] = st[i];
  }
  // 3. transcript (plonk/get_challenges.rs; order: SURVEY.md C.4)
  Transcript<HK> ch{sponge, c.prc};
  ch.init();
  ch.observe_digest(c.circuit_digest);
  for (int i = 0; i < 4; i++) ch.observe(pih[i]);
  const size_t cap_bytes = (size_t)L.hb * L.ncap;
  ch.observe_cap(p, 0, L.ncap, L.hb);
  for (uint32_t k = 0; k < VC_MAX_CHALLENGES; k++)
    if (k < K) betas[k] = ch.get();
  for (uint32_t k = 0; k < VC_MAX_CHALLENGES; k++)
    if (k < K) gammas[k] = ch.get();
  ch.observe_cap(p, cap_bytes, L.ncap, L.hb);
  for (uint32_t k = 0; k < VC_MAX_CHALLENGES; k++)
    if (k < K) alphas[k] = ch.get();
  ch.observe_cap(p, 2 * cap_bytes, L.ncap, L.hb);
  const ext_t zeta = ch.get_ext();
  const Openings op = proof_openings(c, L, p);
  for (uint32_t j = 0; j < nall + K; j++) ch.observe_ext(op(j));
  const ext_t alpha = ch.get_ext();
  for (uint32_t s = 0; s < c.n_steps; s++) {
    ch.observe_cap(p, L.step_caps_at + cap_bytes * s, L.ncap, L.hb);
    rec->beta[s] = ch.get_ext();
  }
  for (size_t i = 0; i < L.final_len; i++) ch.observe_ext(ld_ext(p, L.tail_at + 16 * i));
  ch.observe(ld64(p, L.pow_at));
  const gl_t pow_response = ch.get();
  const uint32_t mask = (uint32_t)(((size_t)1 << L.lgN) - 1);  // N is a power of two: same as % N
  for (uint32_t q = 0; q < c.num_queries; q++) rec->qidx[q] = (uint32_t)ch.get() & mask;
  // the openings reduced with alpha, as fri_combine_initial subtracts them
  ext_t o0 = ext_from(0), o1 = ext_from(0);
  for (uint32_t j = nall; j-- > 0;) o0 = ext_add(ext_mul(o0, alpha), op(j));
  for (uint32_t j = K; j-- > 0;) o1 = ext_add(ext_mul(o1, alpha), op(nall + j));
  rec->zeta = zeta;
  rec->alpha = alpha;
  rec->alpha_k = ext_pow(alpha, K);
  rec->g_zeta = ext_scale(zeta, gl_root(c.d));
  rec->opened0 = o0;
  rec->opened1 = o1;
  return pow_response;
}

template <int HK>
P2_HD uint32_t verify_head(const CircuitView &c, const Layout &L, const uint8_t *p, Strided<gl_t> sponge, Strided<ext_t> terms, HeadRecord *rec) {
  // 1. canonicity of everything in a fixed position
  if (!header_canonical<HK>(c, L, p, L.want)) return VR_HEADER;
  if (!canonical_words(p, L.tail_at, 2 * L.final_len + 1 + c.num_pi)) return VR_TAIL;
  // 2, 3. the public-input hash and the transcript
  gl_t betas[VC_MAX_CHALLENGES], gammas[VC_MAX_CHALLENGES], alphas[VC_MAX_CHALLENGES], pih[4];
  const gl_t pow_response = head_challenges<HK>(c, L, p, sponge, betas, gammas, alphas, pih, rec);
  // 4. zeta^n != 1
  {
    ext_t zn = rec->zeta;
    for (uint32_t i = 0; i < c.d; i++) zn = ext_mul(zn, zn);
    if (zn.c0 == 1 && zn.c1 == 0) return VR_ZETA;
  }
  // 5. the plonk identity at zeta
  if (!plonk_identity_at(c, proof_openings(c, L, p), terms, betas, gammas, alphas, rec->zeta, pih)) return VR_IDENTITY;
  // 6. proof-of-work
  if (c.pow_bits && (pow_response >> (64 - c.pow_bits)) != 0) return VR_POW;
  return VR_OK;
}

// ---- per proof and query ---------------------------------------------------------------------------------------------------
// fri_combine_initial for query qi, from its four leaves: the value the first fold must continue.  *e_out: the exponent of
// the queried point g w_N^e (leaf x0 holds natural LDE row bitrev(x0), g = GL_GEN)
P2_HD ext_t query_initial(const CircuitView &c, const Layout &L, const uint8_t *p, const HeadRecord *rec, uint32_t qi, size_t *e_out) {
  const uint32_t K = c.K, lgN = L.lgN;
  const size_t x0 = rec->qidx[qi] & (uint32_t)(((size_t)1 << lgN) - 1);
  const ext_t alpha = rec->alpha;
  size_t e = 0;
  for (unsigned b = 0; b < lgN; b++) e |= ((x0 >> b) & 1) << (lgN - 1 - b);
  const gl_t x_pt = gl_mul(GL_GEN, gl_pow(gl_root(lgN), e));
  // (F0(x) - F0(zeta)) / (x - zeta) * alpha^K + (F1(x) - F1(g zeta)) / (x - g zeta)
  ext_t acc0 = ext_from(0), acc1 = ext_from(0);
  for (uint32_t o = 4; o-- > 0;) {
    const size_t leaf_at = L.leaf_at(qi, o);
    for (uint32_t j = L.cols[o]; j-- > 0;) acc0 = ext_add(ext_mul(acc0, alpha), ext_from(ld64(p, leaf_at + 8 * (size_t)j)));
  }
  for (uint32_t j = K; j-- > 0;) acc1 = ext_add(ext_mul(acc1, alpha), ext_from(ld64(p, L.leaf_at(qi, 2) + 8 * (size_t)j)));
  ext_t cur = ext_mul(ext_sub(acc0, rec->opened0), ext_inv(ext_sub(ext_from(x_pt), rec->zeta)));
  cur = ext_add(ext_mul(cur, rec->alpha_k), ext_mul(ext_sub(acc1, rec->opened1), ext_inv(ext_sub(ext_from(x_pt), rec->g_zeta))));
  *e_out = e;
  return cur;
}
// One fold (fri/verifier.rs compute_evaluation): the 2^ab values at vals_at, a leaf of the tree over the domain of 2^lg points
// with coset shift `shift`, interpolated at beta.  Leaf slot i holds the point s g^bitrev(i), s = shift * w^(e mod 2^(lg-ab));
// *e is reduced to that exponent.
P2_HD ext_t fold_step(const uint8_t *p, size_t vals_at, unsigned ab, unsigned lg, gl_t shift, size_t *e, ext_t beta) {
  auto y_nat = [&](uint32_t j) { return ld_ext(p, vals_at + 16 * (size_t)bitrev32(j, ab)); };
  *e &= ((size_t)1 << (lg - ab)) - 1;
  const gl_t s_pt = gl_mul(shift, gl_pow(gl_root(lg), *e));
  return interpolate_coset_fn(s_pt, ab, y_nat, beta);
}

// *index: the oracle or the step the reason names (VR_NONE: none)
template <int HK>
P2_HD uint32_t verify_query(const CircuitView &c, const Layout &L, const uint8_t *p, const HeadRecord *rec, uint32_t qi, uint32_t *index) {
  *index = VR_NONE;
  const uint32_t lgN = L.lgN, hb = L.hb;
  const size_t x0 = rec->qidx[qi] & (uint32_t)(((size_t)1 << lgN) - 1);
  // the four initial oracles: the row of each tree at leaf x0
  for (uint32_t o = 0; o < 4; o++) {
    const size_t leaf_at = L.leaf_at(qi, o), len_at = L.leaf_len_at(qi, o);
    *index = o;
    if (p[len_at] != L.init_len) return VR_Q_INIT_SHAPE;
    if (!canonical_words(p, leaf_at, L.cols[o])) {
      *index = VR_NONE;
      return VR_Q_LEAF;
    }
    const dig_t leaf = leaf_digest_at<HK>(p, leaf_at, L.cols[o], c.prc);
    bool canon = true, cap_canon = true;
    const dig_t top = merkle_walk<HK>(p, leaf, x0, len_at + 1, L.init_len, hb, c.prc, &canon);
    const size_t entry = x0 >> L.init_len;  // < 2^cap_h: x0 < 2^lgN
    const dig_t cap = o == 0 ? c.cs_cap[entry] : ld_digest<HK>(p, ((size_t)(o - 1) * L.ncap + entry) * hb, &cap_canon);  // (o > 0: the proof's own caps)
    if (!canon || !dig_same<HK>(top, cap)) return VR_Q_INIT_PATH;
  }
  *index = VR_NONE;
  size_t e;
  ext_t cur = query_initial(c, L, p, rec, qi, &e);
  unsigned lg = lgN;
  gl_t shift = GL_GEN;
  // commit-phase folds
  size_t x = x0;
  for (uint32_t s = 0; s < c.n_steps; s++) {
    const unsigned ab = c.arity[s];
    const uint32_t a = 1u << ab;
    const size_t vals_at = L.vals_at(qi, s), len_at = L.vals_len_at(qi, s, ab);
    const uint32_t levels = lg - ab - c.cap_h;
    *index = s;
    if (!canonical_words(p, vals_at, 2 * (size_t)a) || p[len_at] != levels) return VR_Q_STEP_SHAPE;
    const size_t leaf_index = x >> ab, within = x & (a - 1);
    if (!ext_eq(ld_ext(p, vals_at + 16 * within), cur)) return VR_Q_FOLD;
    const dig_t leaf = leaf_digest_at<HK>(p, vals_at, 2 * a, c.prc);
    bool canon = true, cap_canon = true;
    const dig_t top = merkle_walk<HK>(p, leaf, leaf_index, len_at + 1, levels, hb, c.prc, &canon);
    const size_t entry = leaf_index >> levels;  // < 2^cap_h: leaf_index < 2^(lg - ab)
    const dig_t cap = ld_digest<HK>(p, L.step_caps_at + ((size_t)s * L.ncap + entry) * hb, &cap_canon);
    if (!canon || !dig_same<HK>(top, cap)) return VR_Q_STEP_PATH;
    cur = fold_step(p, vals_at, ab, lg, shift, &e, rec->beta[s]);
    for (unsigned i = 0; i < ab; i++) shift = gl_sqr(shift);
    lg -= ab;
    x = leaf_index;
  }
  *index = VR_NONE;
  // the final polynomial at the folded point
  const gl_t x_last = gl_mul(shift, gl_pow(gl_root(lg), e));
  ext_t fe = ext_from(0);
  for (size_t i = L.final_len; i-- > 0;) fe = ext_add(ext_scale(fe, x_last), ld_ext(p, L.tail_at + 16 * i));
  if (!ext_eq(fe, cur)) return VR_Q_FINAL;
  return VR_OK;
}

// one proof on the calling thread: the head, then the queries in order -- the verdict every entry point gives
struct Verdict {
  uint32_t reason, query, index;
};
// shape_reason as a verdict: a wrong length is reported with the length given and the length the circuit fixes (a proof is
// far below 4 GiB)
template <int HK>
inline Verdict shape_verdict(const CircuitView &c, const Layout &L, const uint8_t *p, size_t len) {
  const uint32_t r = shape_reason<HK>(c, L, p, len);
  const size_t top = VR_NONE - 1;
  if (r == VR_LENGTH) return Verdict{r, (uint32_t)(len < top ? len : top), (uint32_t)(L.want < top ? L.want : top)};
  return Verdict{r, VR_NONE, VR_NONE};
}
template <int HK>
inline Verdict verify_one(const CircuitView &c, const Layout &L, const uint8_t *p, size_t len, gl_t *sponge /* [12] */, ext_t *terms /* [identity_terms] */,
                          HeadRecord *rec) {
  const Verdict shape = shape_verdict<HK>(c, L, p, len);
  if (shape.reason) return shape;
  if (const uint32_t r = verify_head<HK>(c, L, p, Strided<gl_t>{sponge, 1}, Strided<ext_t>{terms, 1}, rec)) return Verdict{r, VR_NONE, VR_NONE};
  for (uint32_t q = 0; q < c.num_queries; q++) {
    uint32_t index = VR_NONE;
    if (const uint32_t r = verify_query<HK>(c, L, p, rec, q, &index)) return Verdict{r, q, index};
  }
  return Verdict{VR_OK, VR_NONE, VR_NONE};
}

}  // namespace vc
}  // namespace p2
