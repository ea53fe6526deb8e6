// proofio.hip -- the reference's on-disk proof format, host code only (no kernel in this file).
//
// `plonky2-backend prove` does not write the prover's output as is: it compresses it first,
// `proof.compress(&circuit_digest, &common).to_bytes()` (plonky2-backend/src/actions/
// prove_action.rs:75-78, hex-encoded at :38-42), and `verify` reads that back with
// `CompressedProofWithPublicInputs::from_bytes` + `verify_compressed`
// (actions/verify_action.rs:11-17, noir_and_plonky2_serialization.rs:24-33).  This file is that
// pair on top of the uncompressed bytes p2gpu_prove writes:
//
//   compress   (plonky2 0.2.2 fri/proof.rs FriProof::compress, hash/merkle_proofs.rs
//               compress_merkle_proofs): query indices stored as u32; per tree the Merkle paths of
//               all queries lose every sibling that another path or leaf already determines; a leaf
//               reached by several queries is stored once (the first query's copy, entries sorted
//               by index); each fold step drops the one evaluation the verifier can infer.
//   decompress the inverse: replays the transcript for the challenges, re-derives the dropped
//               evaluations query by query (get_challenges.rs get_inferred_elements) and rebuilds
//               the sibling lists by hashing upwards.
//
// What is this file's own is the compressed container (variable length: read with a Cursor) and the (de)duplication of
// Merkle paths.  The uncompressed bytes are never parsed here: their length and every offset in them are the circuit's
// (verifycore.hpp make_layout), compress reads them and decompress writes them where they lie, and whatever either needs of
// the verifier -- is this a proof of the circuit's shape, the transcript, the combined initial value, a fold, a digest -- is
// the core's function for it, with the hasher as the template parameter HK.
//
// Pinned by the reference's own files: compress(decompress(x)) == x for
// tests/golden/reference/*.proof.hex (tests/test_reference_proofs.py).  Those have no fold step;
// with fold steps the layout follows the same recollection of 0.2.2 as SURVEY.md C.11 and is covered
// by round trips and by both verifiers accepting the decompressed bytes; tests/test_proofio_pinned.py holds
// every answer (code and output digest) to a fixed list of sound and damaged inputs.
#include "hostproof.hpp"
#include <map>
#include <set>

using namespace p2;

namespace {

int bad(const char *what) {
  set_err("malformed proof: %s", what);
  return P2GPU_E_VERIFY;
}

// the transcript of the proof bytes p (head and tail are all it reads): query indices, fold betas, reduced openings
template <int HK>
vc::HeadRecord challenges(const vc::CircuitView &v, const vc::Layout &L, const uint8_t *p) {
  gl_t sponge[12], betas[vc::VC_MAX_CHALLENGES], gammas[vc::VC_MAX_CHALLENGES], alphas[vc::VC_MAX_CHALLENGES], pih[4];
  vc::HeadRecord rec;
  memset(&rec, 0, sizeof rec);
  vc::head_challenges<HK>(v, L, p, vc::Strided<gl_t>{sponge, 1}, betas, gammas, alphas, pih, &rec);
  return rec;
}

// ---- hash/merkle_proofs.rs compress_merkle_proofs / decompress_merkle_proofs ----
// heap numbering below the cap: node = (leaf index + 2^height) >> level, `height` levels in total
// Per query, the levels of its (full) path whose sibling no leaf and no earlier path determines.
std::vector<std::vector<unsigned>> compress_paths(unsigned height_total, unsigned cap_h, const std::vector<size_t> &idx) {
  const size_t nl = (size_t)1 << height_total;
  std::set<size_t> known;
  for (size_t x : idx)
    for (unsigned j = 0; j < height_total - cap_h; j++) known.insert((x + nl) >> j);
  std::vector<std::vector<unsigned>> out(idx.size());
  for (size_t q = 0; q < idx.size(); q++) {
    size_t node = idx[q] + nl;
    for (unsigned level = 0; level < height_total - cap_h; level++) {
      if (known.insert(node ^ 1).second) out[q].push_back(level);
      node >>= 1;
    }
  }
  return out;
}
// a compressed path: its length byte, then the kept siblings of the full path at sib_at
void put_path(Out &o, const uint8_t *proof, size_t sib_at, uint32_t hb, const std::vector<unsigned> &kept) {
  o.u8((uint8_t)kept.size());
  for (unsigned level : kept) o.put(proof + sib_at + (size_t)hb * level, hb);
}

struct CPath {  // a compressed path where it lies in the input
  const uint8_t *sib = nullptr;
  size_t n = 0;
};
// Rebuilds the full paths of all queries into one tree, each at sib_at[q] of `out`.  False when a compressed path is too
// short / too long.
template <int HK>
bool decompress_paths(const vc::CircuitView &v, const vc::Layout &L, unsigned height_total, const std::vector<size_t> &idx,
                      const std::vector<dig_t> &leaf_hash, const std::vector<const CPath *> &cpaths, const std::vector<size_t> &sib_at, uint8_t *out) {
  const size_t nl = (size_t)1 << height_total;
  std::map<size_t, dig_t> seen;
  for (size_t q = 0; q < idx.size(); q++) seen[idx[q] + nl] = leaf_hash[q];
  std::vector<size_t> used(idx.size(), 0);
  bool canon = true;  // (checked when the path was read)
  for (unsigned layer = 0; layer < height_total - v.cap_h; layer++)
    for (size_t q = 0; q < idx.size(); q++) {
      const size_t node = (idx[q] + nl) >> layer;
      auto it = seen.find(node ^ 1);
      if (it == seen.end()) {
        if (used[q] >= cpaths[q]->n) return false;
        it = seen.emplace(node ^ 1, vc::ld_digest<HK>(cpaths[q]->sib, (size_t)L.hb * used[q]++, &canon)).first;
      }
      const dig_t &cur = seen[node], &sib = it->second;
      seen[node >> 1] = (node & 1) ? vc::node_digest_hk<HK>(sib, cur, v.prc) : vc::node_digest_hk<HK>(cur, sib, v.prc);
    }
  // duplicate queries share one stored path: only the first copy must be used up
  std::set<size_t> first;
  for (size_t q = 0; q < idx.size(); q++)
    if (first.insert(idx[q]).second && used[q] != cpaths[q]->n) return false;
  for (size_t q = 0; q < idx.size(); q++) {
    size_t node = idx[q] + nl;
    for (unsigned layer = 0; layer < height_total - v.cap_h; layer++) {
      memcpy(out + sib_at[q] + (size_t)L.hb * layer, seen[node ^ 1].w, L.hb);
      node >>= 1;
    }
  }
  return true;
}

template <int HK>
int compress(const vc::CircuitView &v, const uint8_t *proof, size_t len, Out &o) {
  const vc::Layout L = vc::make_layout(v);
  if (!vc::well_formed<HK>(v, L, proof, len)) return bad("not the bytes of a proof of this circuit (length, path lengths, canonical field elements)");
  const vc::HeadRecord rec = challenges<HK>(v, L, proof);
  const std::vector<size_t> idx(rec.qidx, rec.qidx + v.num_queries);
  o.put(proof, L.queries_at);
  for (size_t x : idx) o.u32((uint32_t)x);
  // initial trees (all four of one height): the compressed paths, then one entry per distinct index
  {
    const auto kept = compress_paths(L.lgN, v.cap_h, idx);
    std::map<size_t, size_t> first;  // index -> first query with it
    for (size_t q = 0; q < idx.size(); q++) first.emplace(idx[q], q);
    for (auto &kv : first)
      for (int t = 0; t < 4; t++) {
        o.put(proof + L.leaf_at(kv.second, t), 8 * (size_t)L.cols[t]);
        put_path(o, proof, L.leaf_len_at(kv.second, t) + 1, L.hb, kept[kv.second]);
      }
  }
  // fold steps
  std::vector<size_t> cur = idx;
  for (uint32_t s = 0; s < v.n_steps; s++) {
    const unsigned ab = v.arity[s];
    const size_t a = (size_t)1 << ab;
    std::vector<size_t> within(cur.size());
    for (size_t q = 0; q < cur.size(); q++) {
      within[q] = cur[q] & (a - 1);
      cur[q] >>= ab;
    }
    const auto kept = compress_paths(L.step_lg[s] - ab, v.cap_h, cur);
    std::map<size_t, size_t> firsts;
    for (size_t q = 0; q < cur.size(); q++) firsts.emplace(cur[q], q);
    for (auto &kv : firsts) {
      const size_t vals_at = L.vals_at(kv.second, s);
      for (size_t i = 0; i < a; i++)
        if (i != within[kv.second]) o.put(proof + vals_at + 16 * i, 16);
      put_path(o, proof, L.vals_len_at(kv.second, s, ab) + 1, L.hb, kept[kv.second]);
    }
  }
  o.put(proof + L.tail_at, L.want - L.tail_at);
  return P2GPU_OK;
}

// ---- reading the compressed container ----
const uint8_t *take_felts(Cursor &in, size_t n) {  // n canonical field elements
  const uint8_t *q = in.take(8 * n);
  if (q && !vc::canonical_words(q, 0, n)) in.ok = false;
  return in.ok ? q : nullptr;
}
template <int HK>
bool take_path(Cursor &in, size_t max_len, uint32_t hb, CPath &cp) {
  const uint8_t *l = in.take(1);
  if (!l || *l > max_len) return in.ok = false;
  cp.n = *l;
  cp.sib = in.take(hb * cp.n);
  // PoseidonHash digests are 4 field elements: w and w + p hash alike, so only the canonical encoding is a proof
  if (HK && cp.sib && !vc::canonical_words(cp.sib, 0, 4 * cp.n)) in.ok = false;
  return in.ok;
}

// out: the L.want bytes of the uncompressed proof, written where the layout puts them
template <int HK>
int decompress(const vc::CircuitView &v, const uint8_t *data, size_t len, std::vector<uint8_t> &out) {
  const vc::Layout L = vc::make_layout(v);
  if (L.bad_arity) return bad("bad reduction arity in circuit");
  const uint32_t hb = L.hb, n_steps = v.n_steps;
  Cursor in{data, len};
  const uint8_t *head = in.take(L.queries_at);
  if (!head || !vc::header_canonical<HK>(v, L, head, L.queries_at)) return bad("caps / openings");
  std::vector<size_t> idx(v.num_queries);
  for (auto &x : idx) {
    const uint8_t *p = in.take(4);
    uint32_t w = 0;
    if (p) memcpy(&w, p, 4);
    x = w;
    if (x >> L.lgN) in.ok = false;
  }
  if (!in.ok) return bad("query indices");
  // entries sorted by index
  std::set<size_t> distinct(idx.begin(), idx.end());
  struct InitEntry {
    const uint8_t *leaf[4];
    CPath cpath[4];
  };
  std::map<size_t, InitEntry> init;
  for (size_t x : distinct) {
    InitEntry &e = init[x];
    for (int t = 0; t < 4; t++)
      if (!(e.leaf[t] = take_felts(in, L.cols[t])) || !take_path<HK>(in, L.init_len, hb, e.cpath[t])) return bad("initial tree entry");
  }
  struct StepEntry {
    const uint8_t *evals;  // arity - 1 values
    CPath cpath;
  };
  std::vector<std::map<size_t, StepEntry>> steps(n_steps);
  {
    std::vector<size_t> cur = idx;
    for (uint32_t s = 0; s < n_steps; s++) {
      const unsigned ab = v.arity[s];
      std::set<size_t> ds;
      for (auto &x : cur) {
        x >>= ab;
        ds.insert(x);
      }
      for (size_t x : ds) {
        StepEntry &e = steps[s][x];
        if (!(e.evals = take_felts(in, 2 * (((size_t)1 << ab) - 1))) || !take_path<HK>(in, L.step_lg[s] - ab - v.cap_h, hb, e.cpath)) return bad("fold step entry");
      }
    }
  }
  const uint8_t *tail = in.take(L.want - L.tail_at);
  if (!tail || in.at != len) return bad("final polynomial / length");
  out.assign(L.want, 0);
  uint8_t *o = out.data();
  memcpy(o, head, L.queries_at);
  memcpy(o + L.tail_at, tail, L.want - L.tail_at);
  // (the PoW witness between the two is a u64 to this format)
  if (!vc::canonical_words(o, L.tail_at, 2 * L.final_len) || !vc::canonical_words(o, L.pis_at, v.num_pi)) return bad("final polynomial / public inputs");
  for (size_t q = 0; q < idx.size(); q++)
    for (int t = 0; t < 4; t++) {
      memcpy(o + L.leaf_at(q, t), init[idx[q]].leaf[t], 8 * (size_t)L.cols[t]);
      o[L.leaf_len_at(q, t)] = (uint8_t)L.init_len;
    }

  // the stored indices must be the transcript's (CompressedProofWithPublicInputs::decompress
  // takes them from the challenges)
  const vc::HeadRecord rec = challenges<HK>(v, L, o);
  for (size_t q = 0; q < idx.size(); q++)
    if (rec.qidx[q] != idx[q]) return bad("query indices differ from the transcript's");

  std::vector<dig_t> lh(idx.size());
  std::vector<const CPath *> cps(idx.size());
  std::vector<size_t> sib_at(idx.size());
  for (int t = 0; t < 4; t++) {
    for (size_t q = 0; q < idx.size(); q++) {
      lh[q] = vc::leaf_digest_at<HK>(o, L.leaf_at(q, t), L.cols[t], v.prc);
      cps[q] = &init[idx[q]].cpath[t];
      sib_at[q] = L.leaf_len_at(q, t) + 1;
    }
    if (!decompress_paths<HK>(v, L, L.lgN, idx, lh, cps, sib_at, o)) return bad("compressed Merkle path (initial tree)");
  }
  // fold steps: re-derive the dropped evaluation for the first query that reaches a leaf, reuse it after
  std::vector<std::map<size_t, size_t>> rebuilt(n_steps);  // per step: leaf index -> the query whose copy is complete
  for (size_t q = 0; q < idx.size(); q++) {
    size_t x = idx[q], e;
    ext_t cur = vc::query_initial(v, L, o, &rec, (uint32_t)q, &e);
    unsigned lg = L.lgN;
    gl_t shift = GL_GEN;
    bool live = true;  // false once a leaf was already rebuilt: the rest of this query's chain is known
    for (uint32_t s = 0; s < n_steps; s++) {
      const unsigned ab = v.arity[s];
      const size_t a = (size_t)1 << ab, within = x & (a - 1), leaf_index = x >> ab, vals_at = L.vals_at(q, s);
      auto it = rebuilt[s].find(leaf_index);
      if (it == rebuilt[s].end()) {
        if (!live) return bad("fold chain");  // cannot happen: equal leaf at step s implies equal leaves after
        const uint8_t *stored = steps[s][leaf_index].evals;
        const gl_t inferred[2] = {cur.c0, cur.c1};
        memcpy(o + vals_at, stored, 16 * within);
        memcpy(o + vals_at + 16 * within, inferred, 16);
        memcpy(o + vals_at + 16 * (within + 1), stored + 16 * within, 16 * (a - 1 - within));
        rebuilt[s].emplace(leaf_index, q);
      } else {
        live = false;
        memcpy(o + vals_at, o + L.vals_at(it->second, s), 16 * a);
      }
      o[L.vals_len_at(q, s, ab)] = (uint8_t)(lg - ab - v.cap_h);
      if (live) cur = vc::fold_step(o, vals_at, ab, lg, shift, &e, rec.beta[s]);
      for (unsigned i = 0; i < ab; i++) shift = gl_sqr(shift);
      lg -= ab;
      x = leaf_index;
    }
  }
  std::vector<size_t> cur = idx;
  for (uint32_t s = 0; s < n_steps; s++) {
    const unsigned ab = v.arity[s];
    for (size_t q = 0; q < cur.size(); q++) {
      cur[q] >>= ab;
      lh[q] = vc::leaf_digest_at<HK>(o, L.vals_at(q, s), 2u << ab, v.prc);
      cps[q] = &steps[s][cur[q]].cpath;
      sib_at[q] = L.vals_len_at(q, s, ab) + 1;
    }
    if (!decompress_paths<HK>(v, L, L.step_lg[s] - ab, cur, lh, cps, sib_at, o)) return bad("compressed Merkle path (fold step)");
  }
  return P2GPU_OK;
}

int do_decompress(const p2gpu_circuit *c, const uint8_t *data, size_t len, std::vector<uint8_t> &out) {
  const vc::CircuitView v = view_of(c);
  return v.hasher ? decompress<1>(v, data, len, out) : decompress<0>(v, data, len, out);
}

}  // namespace

extern "C" {

int p2gpu_proof_compress(const p2gpu_circuit *c, const uint8_t *proof, size_t len, uint8_t *out, size_t *out_len) try {
  if (!c || !proof || !out_len) return P2GPU_E_ARG;
  const vc::CircuitView v = view_of(c);
  Out o;
  if (int rc = v.hasher ? compress<1>(v, proof, len, o) : compress<0>(v, proof, len, o)) return rc;
  return emit(o, out, out_len);
} P2GPU_CATCH

int p2gpu_proof_decompress(const p2gpu_circuit *c, const uint8_t *cproof, size_t len, uint8_t *out, size_t *out_len) try {
  if (!c || !cproof || !out_len) return P2GPU_E_ARG;
  std::vector<uint8_t> proof;
  if (int rc = do_decompress(c, cproof, len, proof)) return rc;
  return emit(proof, out, out_len);
} P2GPU_CATCH

int p2gpu_verify_compressed(const p2gpu_circuit *c, const uint8_t *cproof, size_t len) try {
  if (!c || !cproof) return P2GPU_E_ARG;
  std::vector<uint8_t> proof;
  if (int rc = do_decompress(c, cproof, len, proof)) return rc;
  return p2gpu_verify(c, proof.data(), proof.size());
} P2GPU_CATCH

}  // extern "C"
