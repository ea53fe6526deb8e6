// decompresscore.hpp -- the inverse of the on-disk proof compression (proofio.hip decompress), once, for the host and for the
// device, written for lanes: p2gpu_verify_batch_compressed_host runs the functions of this file in plain loops on the calling
// thread, the kernels of decompressdev.hip run them with one wave per proof (or per proof and tree) and one lane per query.
// proofio.hip's decompress stays what it is -- sequential, with a cursor and maps -- and is the oracle of this file: the same
// bytes out, and the same reject site for every input.
//
//   walk          host only, per proof: the cursor walk over the variable-length container.  The stored u32 indices fix the
//                 distinct leaves per tree and every path carries its length byte, so the walk needs no transcript and no
//                 arithmetic: it leaves an offset table (where the tail lies, and per query where its entry of each initial
//                 tree and of each fold step lies).  A proof whose walk fails -- out of bytes, a path longer than its tree, an
//                 index >= 2^lgN, trailing bytes -- never reaches the functions below.
//   scatter_lane  the head, the tail and every query's four leaves to their place in the uncompressed proof, the length bytes
//                 the circuit fixes, and the canonicity checks of the sequential reader (header, initial entries, step entries,
//                 tail) as flags
//   head_lane     one lane per proof: the transcript on the scattered head and tail (vc::head_challenges, once), the stored
//                 indices against the transcript's, and the head's own reason (vc::verify_head's, which ranks after every
//                 failure of the decompression), kept aside
//   infer_*       one lane per query, a wave-level sync per fold step: the running value inserted among the stored ones; the
//                 lowest query that reaches a leaf infers, every later one copies that query's values and stops inferring
//   rebuild_*     one wave per tree (four initial trees, one per fold step), one lane per query, layer by layer: a lane reads
//                 the next sibling of its compressed path iff no lane holds its sibling node and it is the lowest lane with its
//                 node; else it takes the digest of the lane that holds the sibling, or what the lowest lane with its node read
// WHAT NO PROOF BYTE CAN DO after the walk: move a read or a write.  Every offset into the compressed bytes comes from the
// table, every path length byte was compared with the height of its tree by the walk and a lane reads sibling `used` only
// while used < that byte, every stored index is < 2^lgN, and every write goes to an offset of vc::Layout.
// The lanes of a proof share three small arrays (LDS on the device, the stack on the host): no lane indexes a private array
// at run time.
#pragma once
#include "verifycore.hpp"
#include <algorithm>

namespace p2 {
namespace dc {

// ---- reasons: one per reject site of proofio.hip's decompress, in its order, after vc's ------------------------------------
enum : uint32_t {
  VR_C_ARITY = 16,
  VR_C_HEADER = 17,
  VR_C_INDICES = 18,
  VR_C_INIT_ENTRY = 19,
  VR_C_STEP_ENTRY = 20,
  VR_C_LENGTH = 21,
  VR_C_TAIL = 22,
  VR_C_INDEX_CHECK = 23,
  VR_C_INIT_PATH = 24,
  VR_C_STEP_PATH = 25,
  VR_C_FOLD_CHAIN = 26,  // (unreachable: an equal leaf at one step implies equal leaves after)
  VR_C_END
};
// the wording behind "malformed proof: " (nullptr: not a code of this file)
inline const char *reason_words(uint32_t reason) {
  switch (reason) {
  case VR_C_ARITY: return "bad reduction arity in circuit";
  case VR_C_HEADER: return "caps / openings";
  case VR_C_INDICES: return "query indices";
  case VR_C_INIT_ENTRY: return "initial tree entry";
  case VR_C_STEP_ENTRY: return "fold step entry";
  case VR_C_LENGTH: return "final polynomial / length";
  case VR_C_TAIL: return "final polynomial / public inputs";
  case VR_C_INDEX_CHECK: return "query indices differ from the transcript's";
  case VR_C_INIT_PATH: return "compressed Merkle path (initial tree)";
  case VR_C_STEP_PATH: return "compressed Merkle path (fold step)";
  case VR_C_FOLD_CHAIN: return "fold chain";
  }
  return nullptr;
}

// What the lanes find, one bit per reject site that is theirs, in the order the sequential reader meets the sites: the
// verdict is the lowest bit set.
enum : uint32_t { F_HEADER = 1, F_INIT_ENTRY = 2, F_STEP_ENTRY = 4, F_TAIL = 8, F_INDEX_CHECK = 16, F_INIT_PATH = 32, F_STEP_PATH = 64 };
P2_HD uint32_t flags_reason(uint32_t flags) {
  if (flags & F_HEADER) return VR_C_HEADER;
  if (flags & F_INIT_ENTRY) return VR_C_INIT_ENTRY;
  if (flags & F_STEP_ENTRY) return VR_C_STEP_ENTRY;
  if (flags & F_TAIL) return VR_C_TAIL;
  if (flags & F_INDEX_CHECK) return VR_C_INDEX_CHECK;
  if (flags & F_INIT_PATH) return VR_C_INIT_PATH;
  if (flags & F_STEP_PATH) return VR_C_STEP_PATH;
  return vc::VR_OK;
}

// ---- the offset table of one compressed proof ---------------------------------------------------------------------------
// [0]: the tail; then per query 4 + n_steps words: its leaf in the entry of each initial tree, its stored evaluations in the
// entry of each fold step (queries that share a leaf share the entry).  An entry is: words | length byte | kept siblings.
P2_HD uint32_t table_words(const vc::CircuitView &c) { return 1 + c.num_queries * (4 + c.n_steps); }
P2_HD uint32_t table_init(const vc::CircuitView &c, uint32_t q, uint32_t t) { return 1 + q * (4 + c.n_steps) + t; }
P2_HD uint32_t table_step(const vc::CircuitView &c, uint32_t q, uint32_t s) { return 1 + q * (4 + c.n_steps) + 4 + s; }

// stored evaluations of a step entry: 2^ab - 1 extension elements
P2_HD size_t step_entry_words(unsigned ab) { return 2 * (((size_t)1 << ab) - 1); }
// the bits a query index has lost when it names a leaf of step s's tree
P2_HD unsigned step_shift(const vc::CircuitView &c, uint32_t s) {
  unsigned sh = 0;
  for (uint32_t i = 0; i <= s; i++) sh += c.arity[i];
  return sh;
}

P2_HD uint32_t ld32(const uint8_t *p, size_t at) {
  return (uint32_t)p[at] | (uint32_t)p[at + 1] << 8 | (uint32_t)p[at + 2] << 16 | (uint32_t)p[at + 3] << 24;
}
// query q's index as the container stores it
P2_HD uint32_t stored_index(const vc::Layout &L, const uint8_t *cp, uint32_t q) { return ld32(cp, L.queries_at + 4 * (size_t)q); }

// The cursor walk (host).  False: the lone path answers for this proof.
inline bool walk(const vc::CircuitView &c, const vc::Layout &L, const uint8_t *data, size_t len, uint32_t *tab) {
  if (L.bad_arity || len > UINT32_MAX || c.num_queries > vc::VC_MAX_QUERIES) return false;
  const uint32_t nq = c.num_queries, hb = L.hb;
  size_t at = L.queries_at;
  if (len < at + 4 * (size_t)nq) return false;
  uint32_t idx[vc::VC_MAX_QUERIES], order[vc::VC_MAX_QUERIES];
  for (uint32_t q = 0; q < nq; q++) {
    idx[q] = stored_index(L, data, q);
    if ((size_t)idx[q] >> L.lgN) return false;
  }
  at += 4 * (size_t)nq;
  // one tree's entries, sorted by leaf index `idx >> sh`, one per distinct leaf: `words` field elements, a path of at most
  // `max_len` siblings; slot: the table word of query q for this tree
  auto entries = [&](unsigned sh, size_t words, uint32_t max_len, uint32_t ntrees, auto slot) {
    for (uint32_t q = 0; q < nq; q++) order[q] = q;
    std::sort(order, order + nq, [&](uint32_t a, uint32_t b) { return (idx[a] >> sh) < (idx[b] >> sh); });
    for (uint32_t i = 0; i < nq;) {
      uint32_t j = i;
      while (j < nq && (idx[order[j]] >> sh) == (idx[order[i]] >> sh)) j++;
      for (uint32_t t = 0; t < ntrees; t++) {
        const size_t w = ntrees == 4 ? 8 * (size_t)L.cols[t] : 8 * words, entry = at;
        if (len - at < w + 1) return false;
        at += w;
        const uint32_t n = data[at++];
        if (n > max_len || len - at < (size_t)hb * n) return false;
        at += (size_t)hb * n;
        for (uint32_t k = i; k < j; k++) tab[slot(order[k], t)] = (uint32_t)entry;
      }
      i = j;
    }
    return true;
  };
  if (!entries(0, 0, L.init_len, 4, [&](uint32_t q, uint32_t t) { return table_init(c, q, t); })) return false;
  for (uint32_t s = 0; s < c.n_steps; s++) {
    const unsigned ab = c.arity[s];
    if (!entries(step_shift(c, s), step_entry_words(ab), L.step_lg[s] - ab - c.cap_h, 1, [&](uint32_t q, uint32_t) { return table_step(c, q, s); }))
      return false;
  }
  tab[0] = (uint32_t)at;
  return len - at == L.want - L.tail_at;
}

// ---- bytes in and out -----------------------------------------------------------------------------------------------------
// bytes [0, n) of src to dst, this lane's share; neither side is aligned (digests of 25 bytes, length bytes)
P2_HD void copy_bytes(uint8_t *dst, const uint8_t *src, size_t n, uint32_t lane, uint32_t lanes) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll 4
  for (size_t i = lane; i < n; i += lanes) dst[i] = src[i];
#else
  if (lane == 0) memcpy(dst, src, n);
#endif
}
P2_HD void st64(uint8_t *p, size_t at, uint64_t v) {
#if defined(__HIP_DEVICE_COMPILE__)
#pragma unroll
  for (int i = 0; i < 8; i++) p[at + i] = (uint8_t)(v >> (8 * i));
#else
  memcpy(p + at, &v, 8);
#endif
}
P2_HD void st_ext(uint8_t *p, size_t at, ext_t v) {
  st64(p, at, v.c0);
  st64(p, at + 8, v.c1);
}
template <int HK>
P2_HD void st_digest(uint8_t *p, size_t at, const dig_t &d) {
  st64(p, at, d.w[0]);
  st64(p, at + 8, d.w[1]);
  st64(p, at + 16, d.w[2]);
  if constexpr (HK) st64(p, at + 24, d.w[3]);
  else p[at + 24] = (uint8_t)d.w[3];
}
// this lane's share of `count` words at `at`: are they field elements
P2_HD bool canonical_share(const uint8_t *p, size_t at, size_t count, uint32_t lane, uint32_t lanes) {
  bool ok = true;
  for (size_t i = lane; i < count; i += lanes) ok &= vc::ld64(p, at + 8 * i) < GL_P;
  return ok;
}

// ---- scatter ---------------------------------------------------------------------------------------------------------------
// cp: the compressed proof, tab: its table, out: the uncompressed proof (L.want bytes).  `lanes` lanes share the work of one
// proof; the flags of a proof are the OR over its lanes.
template <int HK>
P2_HD uint32_t scatter_lane(const vc::CircuitView &c, const vc::Layout &L, const uint8_t *cp, const uint32_t *tab, uint8_t *out, uint32_t lane,
                            uint32_t lanes) {
  uint32_t flags = 0;
  // header: caps | openings | step caps, as vc::header_canonical asks
  copy_bytes(out, cp, L.queries_at, lane, lanes);
  bool ok = canonical_share(cp, L.open_at, 2 * (size_t)(L.nall + c.K), lane, lanes);
  if constexpr (HK) {
    ok &= canonical_share(cp, 0, 12 * (size_t)L.ncap, lane, lanes);
    ok &= canonical_share(cp, L.step_caps_at, 4 * (size_t)L.ncap * c.n_steps, lane, lanes);
  }
  if (!ok) flags |= F_HEADER;
  // initial entries: the leaf to its place; its words and (PoseidonHash) its kept siblings canonical
  ok = true;
  for (uint32_t q = 0; q < c.num_queries; q++)
    for (uint32_t t = 0; t < 4; t++) {
      const size_t src = tab[table_init(c, q, t)], nbytes = 8 * (size_t)L.cols[t];
      copy_bytes(out + L.leaf_at(q, t), cp + src, nbytes, lane, lanes);
      ok &= canonical_share(cp, src, L.cols[t], lane, lanes);
      if constexpr (HK) ok &= canonical_share(cp, src + nbytes + 1, 4 * (size_t)cp[src + nbytes], lane, lanes);
      if (lane == 0) out[L.leaf_len_at(q, t)] = (uint8_t)L.init_len;
    }
  if (!ok) flags |= F_INIT_ENTRY;
  // step entries: checked here, placed by the inference
  ok = true;
  for (uint32_t q = 0; q < c.num_queries; q++)
    for (uint32_t s = 0; s < c.n_steps; s++) {
      const unsigned ab = c.arity[s];
      const size_t src = tab[table_step(c, q, s)], words = step_entry_words(ab);
      ok &= canonical_share(cp, src, words, lane, lanes);
      if constexpr (HK) ok &= canonical_share(cp, src + 8 * words + 1, 4 * (size_t)cp[src + 8 * words], lane, lanes);
      if (lane == 0) out[L.vals_len_at(q, s, ab)] = (uint8_t)(L.step_lg[s] - ab - c.cap_h);
    }
  if (!ok) flags |= F_STEP_ENTRY;
  // tail: final polynomial | PoW witness (a u64 to this format) | public inputs
  const size_t tail = tab[0];
  copy_bytes(out + L.tail_at, cp + tail, L.want - L.tail_at, lane, lanes);
  ok = canonical_share(cp, tail, 2 * L.final_len, lane, lanes) && canonical_share(cp, tail + (L.pis_at - L.tail_at), c.num_pi, lane, lanes);
  if (!ok) flags |= F_TAIL;
  return flags;
}

// ---- head -------------------------------------------------------------------------------------------------------------------
// The transcript of the scattered head and tail, once: fills *rec as proofio.hip's decompress would have it, compares the stored
// indices (F_INDEX_CHECK), and -- judge -- leaves in *head_reason what vc::verify_head answers for these bytes (the header and
// the tail but for the PoW witness are known to be canonical here).
template <int HK>
P2_HD uint32_t head_lane(const vc::CircuitView &c, const vc::Layout &L, const uint8_t *cp, const uint8_t *out, vc::Strided<gl_t> sponge,
                         vc::Strided<ext_t> terms, vc::HeadRecord *rec, bool judge, uint32_t *head_reason) {
  *head_reason = vc::VR_OK;
  gl_t betas[vc::VC_MAX_CHALLENGES], gammas[vc::VC_MAX_CHALLENGES], alphas[vc::VC_MAX_CHALLENGES], pih[4];
  const gl_t pow_response = vc::head_challenges<HK>(c, L, out, sponge, betas, gammas, alphas, pih, rec);
  bool same = true;
  for (uint32_t q = 0; q < c.num_queries; q++) same &= rec->qidx[q] == stored_index(L, cp, q);
  if (!same) return F_INDEX_CHECK;
  if (!judge) return 0;
  if (vc::ld64(out, L.pow_at) >= GL_P) {
    *head_reason = vc::VR_TAIL;
    return 0;
  }
  ext_t zn = rec->zeta;
  for (uint32_t i = 0; i < c.d; i++) zn = ext_mul(zn, zn);
  if (zn.c0 == 1 && zn.c1 == 0) *head_reason = vc::VR_ZETA;
  else if (!vc::plonk_identity_at(c, vc::proof_openings(c, L, out), terms, betas, gammas, alphas, rec->zeta, pih)) *head_reason = vc::VR_IDENTITY;
  else if (c.pow_bits && (pow_response >> (64 - c.pow_bits)) != 0) *head_reason = vc::VR_POW;
  return 0;
}

// ---- inferred evaluations -------------------------------------------------------------------------------------------------
struct InferLane {
  ext_t cur;
  size_t e;
  gl_t shift;
  unsigned lg;
  uint32_t first;  // at the step in hand: the lowest query that reaches this lane's leaf
  bool live;       // false once a leaf was already rebuilt: the rest of this query's chain is known
};
P2_HD void infer_begin(const vc::CircuitView &c, const vc::Layout &L, const uint8_t *out, const vc::HeadRecord *rec, uint32_t q, InferLane &n) {
  n.cur = vc::query_initial(c, L, out, rec, q, &n.e);
  n.shift = GL_GEN;
  n.lg = L.lgN;
  n.first = q;
  n.live = true;
}
// Step s, before the sync: the lowest query of a leaf writes its 2^ab values, the running one at slot x & (a - 1).
P2_HD void infer_place(const vc::CircuitView &c, const vc::Layout &L, const uint8_t *cp, const uint32_t *tab, uint8_t *out, const vc::HeadRecord *rec,
                       uint32_t s, uint32_t q, InferLane &n) {
  const unsigned ab = c.arity[s], sh = step_shift(c, s);
  const uint32_t a = 1u << ab, leaf_index = rec->qidx[q] >> sh, within = (rec->qidx[q] >> (sh - ab)) & (a - 1);
  uint32_t first = q;
  for (uint32_t k = q; k-- > 0;)
    if ((rec->qidx[k] >> sh) == leaf_index) first = k;
  n.first = first;
  if (first != q) return;
  const size_t stored = tab[table_step(c, q, s)], vals_at = L.vals_at(q, s);
  for (uint32_t i = 0; i < a; i++) {
    const ext_t v = i == within ? n.cur : vc::ld_ext(cp, stored + 16 * (size_t)(i < within ? i : i - 1));
    st_ext(out, vals_at + 16 * (size_t)i, v);
  }
}
// Step s, after the sync: every later query of the leaf copies the lowest one's values and stops inferring; a live query folds.
P2_HD void infer_fold(const vc::CircuitView &c, const vc::Layout &L, uint8_t *out, const vc::HeadRecord *rec, uint32_t s, uint32_t q, InferLane &n) {
  const unsigned ab = c.arity[s];
  const size_t vals_at = L.vals_at(q, s);
  if (n.first != q) {
    n.live = false;
    const size_t from = L.vals_at(n.first, s);
    for (size_t i = 0; i < ((size_t)2 << ab); i++) st64(out, vals_at + 8 * i, vc::ld64(out, from + 8 * i));
  }
  if (n.live) n.cur = vc::fold_step(out, vals_at, ab, n.lg, n.shift, &n.e, rec->beta[s]);
  for (unsigned i = 0; i < ab; i++) n.shift = gl_sqr(n.shift);
  n.lg -= ab;
}

// ---- path rebuild -----------------------------------------------------------------------------------------------------------
// tree < 4: that initial oracle; tree >= 4: fold step tree - 4
struct Tree {
  uint32_t shift, levels, leaf_words, flag;
};
P2_HD Tree tree_of(const vc::CircuitView &c, const vc::Layout &L, uint32_t tree) {
  if (tree < 4) return Tree{0, L.init_len, L.cols[tree], F_INIT_PATH};
  const uint32_t s = tree - 4;
  const unsigned ab = c.arity[s];
  return Tree{step_shift(c, s), L.step_lg[s] - ab - c.cap_h, 2u << ab, F_STEP_PATH};
}
// what the lanes of a tree share: every lane's leaf index, its node's digest, and the sibling it read at the layer in hand
struct TreeShared {
  uint32_t leaf[vc::VC_MAX_QUERIES];
  dig_t cur[vc::VC_MAX_QUERIES], read[vc::VC_MAX_QUERIES];
};
struct PathLane {
  dig_t cur;
  size_t stored, sib_at;  // the kept siblings in the container; the full path in the proof
  uint32_t used, n, partner, lowest;
  bool counted;  // the lowest lane of its leaf: its stored path must be used up exactly
};
template <int HK>
P2_HD void rebuild_begin(const vc::CircuitView &c, const vc::Layout &L, const uint8_t *cp, const uint32_t *tab, const uint8_t *out,
                         const vc::HeadRecord *rec, uint32_t tree, const Tree &T, uint32_t q, TreeShared &sh, PathLane &n) {
  size_t leaf_at, len_at;
  if (tree < 4) {
    leaf_at = L.leaf_at(q, tree);
    len_at = tab[table_init(c, q, tree)] + 8 * (size_t)T.leaf_words;
    n.sib_at = L.leaf_len_at(q, tree) + 1;
  } else {
    const unsigned ab = c.arity[tree - 4];
    leaf_at = L.vals_at(q, tree - 4);
    len_at = tab[table_step(c, q, tree - 4)] + 8 * step_entry_words(ab);
    n.sib_at = L.vals_len_at(q, tree - 4, ab) + 1;
  }
  n.cur = vc::leaf_digest_at<HK>(out, leaf_at, T.leaf_words, c.prc);
  n.n = cp[len_at];
  n.stored = len_at + 1;
  n.used = 0;
  n.partner = n.lowest = vc::VR_NONE;
  n.counted = false;
  sh.leaf[q] = rec->qidx[q] >> T.shift;
}
// Layer `layer`, before the sync: who holds my sibling node, who is the lowest lane with my node; I read if neither helps.
// False: this lane must read and its path is used up.
template <int HK>
P2_HD bool rebuild_read(const vc::Layout &L, const uint8_t *cp, uint32_t nq, uint32_t layer, uint32_t q, TreeShared &sh, PathLane &n) {
  const uint32_t node = sh.leaf[q] >> layer;
  n.partner = n.lowest = vc::VR_NONE;
  for (uint32_t k = nq; k-- > 0;) {
    const uint32_t other = sh.leaf[k] >> layer;
    if (other == (node ^ 1)) n.partner = k;
    if (other == node) n.lowest = k;
  }
  if (layer == 0) n.counted = n.lowest == q;
  sh.cur[q] = n.cur;
  if (n.partner != vc::VR_NONE || n.lowest != q) return true;
  dig_t d;
  d.w[0] = d.w[1] = d.w[2] = d.w[3] = 0;
  const bool have = n.used < n.n;
  if (have) {
    bool canon = true;  // (checked with the entry)
    d = vc::ld_digest<HK>(cp, n.stored + (size_t)L.hb * n.used++, &canon);
  }
  sh.read[q] = d;
  return have;
}
// Layer `layer`, after the sync: the sibling into the full path, the parent's digest
template <int HK>
P2_HD void rebuild_hash(const vc::CircuitView &c, const vc::Layout &L, uint8_t *out, uint32_t layer, uint32_t q, const TreeShared &sh, PathLane &n) {
  const dig_t sib = n.partner != vc::VR_NONE ? sh.cur[n.partner] : sh.read[n.lowest];
  st_digest<HK>(out, n.sib_at + (size_t)L.hb * layer, sib);
  const bool odd = (sh.leaf[q] >> layer) & 1;
  const dig_t left = odd ? sib : n.cur, right = odd ? n.cur : sib;
  n.cur = vc::node_digest_hk<HK>(left, right, c.prc);
}
P2_HD bool rebuild_end(const PathLane &n) { return !n.counted || n.used == n.n; }

// ---- one proof on the calling thread ---------------------------------------------------------------------------------------
// The stages above in plain loops.  Returns the flags; out: L.want bytes, complete when the flags are 0.  A stage runs only
// when none before it has failed, as on the device.
template <int HK>
inline uint32_t decompress_one(const vc::CircuitView &c, const vc::Layout &L, const uint8_t *cp, const uint32_t *tab, uint8_t *out, gl_t *sponge,
                               ext_t *terms, vc::HeadRecord *rec, bool judge, uint32_t *head_reason) {
  const uint32_t nq = c.num_queries;
  *head_reason = vc::VR_OK;
  uint32_t flags = scatter_lane<HK>(c, L, cp, tab, out, 0, 1);
  if (flags) return flags;
  flags = head_lane<HK>(c, L, cp, out, vc::Strided<gl_t>{sponge, 1}, vc::Strided<ext_t>{terms, 1}, rec, judge, head_reason);
  if (flags) return flags;
  InferLane lanes[vc::VC_MAX_QUERIES];
  for (uint32_t q = 0; q < nq; q++) infer_begin(c, L, out, rec, q, lanes[q]);
  for (uint32_t s = 0; s < c.n_steps; s++) {
    for (uint32_t q = 0; q < nq; q++) infer_place(c, L, cp, tab, out, rec, s, q, lanes[q]);
    for (uint32_t q = 0; q < nq; q++) infer_fold(c, L, out, rec, s, q, lanes[q]);
  }
  TreeShared sh;
  PathLane path[vc::VC_MAX_QUERIES];
  for (uint32_t tree = 0; tree < 4 + c.n_steps; tree++) {
    const Tree T = tree_of(c, L, tree);
    bool ok = true;
    for (uint32_t q = 0; q < nq; q++) rebuild_begin<HK>(c, L, cp, tab, out, rec, tree, T, q, sh, path[q]);
    for (uint32_t layer = 0; layer < T.levels; layer++) {
      for (uint32_t q = 0; q < nq; q++) ok &= rebuild_read<HK>(L, cp, nq, layer, q, sh, path[q]);
      for (uint32_t q = 0; q < nq; q++) rebuild_hash<HK>(c, L, out, layer, q, sh, path[q]);
    }
    for (uint32_t q = 0; q < nq; q++) ok &= rebuild_end(path[q]);
    if (!ok) flags |= T.flag;
  }
  return flags;
}

}  // namespace dc
}  // namespace p2
