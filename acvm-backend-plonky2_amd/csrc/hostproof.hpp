// hostproof.hpp -- where the handle (circuit.hpp) meets the core (verifycore.hpp), for every host file that reads or writes
// proof or key bytes: the verifier (verify.hip, verifydev.hip), the proof (de)compression (proofio.hip), the verifier-key file
// format (vkio.hip), the prover's transcript and serialiser (prover.hip) and the handle's digest and size getters (handle.hip,
// hostcore.hip).  A bounds-checked byte cursor for input of variable length, a growing byte sink with the two-call output
// convention of the C ABI, the handle's view and layout for the core, and the core's hasher chosen by the handle's.
#pragma once
#include "circuit.hpp"
#include "verifycore.hpp"
#include "decompresscore.hpp"

namespace p2 {

// bounds-checked cursor over input bytes whose parts have no fixed place (a compressed proof, a verifier-key file)
struct Cursor {
  const uint8_t *p;
  size_t len, at = 0;
  bool ok = true;
  const uint8_t *take(size_t n) {
    if (!ok || n > len - at) {
      ok = false;
      return nullptr;
    }
    const uint8_t *q = p + at;
    at += n;
    return q;
  }
  uint64_t u64() {
    uint64_t v = 0;
    if (const uint8_t *q = take(8)) memcpy(&v, q, 8);
    return v;
  }
  gl_t felt() {  // canonical field element
    uint64_t v = u64();
    if (v >= GL_P) ok = false;
    return v;
  }
};

// growing output bytes, and how an entry point hands them over: `out == NULL` asks for the size
struct Out {
  std::vector<uint8_t> v;
  void put(const void *p, size_t n) {
    const uint8_t *q = (const uint8_t *)p;
    v.insert(v.end(), q, q + n);
  }
  void u8(uint8_t x) { v.push_back(x); }
  void u32(uint32_t x) { put(&x, 4); }
  void u64(uint64_t x) { put(&x, 8); }
  void dig(const dig_t &d, size_t hb) { put(d.w, hb); }  // hb: digest_bytes of the circuit's hasher
};
inline int emit(const std::vector<uint8_t> &v, uint8_t *out, size_t *out_len) {
  if (!out || *out_len < v.size()) {
    const bool probe = out == nullptr;
    *out_len = v.size();
    if (probe) return P2GPU_OK;
    set_err("output buffer too small: %zu bytes needed", v.size());
    return P2GPU_E_BUFFER;
  }
  memcpy(out, v.data(), v.size());
  *out_len = v.size();
  return P2GPU_OK;
}
inline int emit(const Out &o, uint8_t *out, size_t *out_len) { return emit(o.v, out, out_len); }

// the verifier's share of a handle as the core takes it (host pointers, valid while the handle lives)
inline vc::CircuitView view_of(const p2gpu_circuit *c) {
  vc::CircuitView v;
  memset(&v, 0, sizeof v);
  v.d = c->d; v.W = c->W; v.R = c->R; v.NC = c->NC; v.num_selectors = c->num_selectors; v.K = c->K; v.QF = c->QF; v.PP = c->PP;
  v.nchunks = c->nchunks; v.rate_bits = c->rate_bits; v.cap_h = c->cap_h; v.pow_bits = c->pow_bits; v.num_queries = c->num_queries;
  v.n_steps = c->n_steps;
  for (int i = 0; i < 8; i++) v.arity[i] = c->arity[i];
  v.num_gates = c->num_gates; v.num_pi = c->num_pi; v.max_gate_constraints = c->max_gate_constraints; v.hasher = c->hasher;
  v.gates = c->gates.data(); v.k_is = c->k_is.data(); v.cs_cap = c->cs.cap.data(); v.prc = c->poseidon_rc_gate;
  v.circuit_digest = c->circuit_digest;
  return v;
}

// every offset of the circuit's proofs, and their one length (`want`)
inline vc::Layout layout_of(const p2gpu_circuit *c) { return vc::make_layout(view_of(c)); }

// a cap the prover holds (Batch::cap) into a transcript
template <int HK>
inline void observe_cap(vc::Transcript<HK> &ch, const std::vector<dig_t> &cap) {
  for (const dig_t &d : cap) ch.observe_digest(d);
}

// H::hash_no_pad of n > 4 words under the circuit's hasher (at that length the core's hash_or_noop hashes); prc: CircuitView::prc
inline dig_t hash_no_pad(uint32_t hasher, const gl_t *v, uint32_t n, const gl_t *prc) {
  const uint8_t *p = (const uint8_t *)v;
  return hasher ? vc::leaf_digest_at<1>(p, 0, n, prc) : vc::leaf_digest_at<0>(p, 0, n, prc);
}

// ---- verify.hip: what p2gpu_verify_batch_host and p2gpu_verify_batch (verifydev.hip) share ----
// the refusals that need no device (P2GPU_E_ARG; 0: the call may go on); reports: the per-proof output, whatever its type
int verify_batch_args(const p2gpu_circuit *c, const uint8_t *proofs, const size_t *offsets, size_t batch, const void *reports);
void verify_report_fill(p2gpu_verify_report *r, const vc::Verdict &v);
int verify_batch_finish(size_t batch, const size_t *offsets, const vc::Layout &L, const p2gpu_verify_report *reports);
vc::Verdict verify_one_host(const vc::CircuitView &v, const vc::Layout &L, const uint8_t *proof, size_t len, std::vector<ext_t> &terms);

// ---- decompressbatch.hip: what the entry points for a batch of compressed proofs share (decompressdev.hip has the device's) ----
// The container walk of every proof.  slot: the batch index of each proof that goes on to the core, tabs: their offset tables
// back to back (dc::table_words each); reason[b]: for every other proof its verdict from the lone path, a dc::VR_C_* code.
int cbatch_walk(const p2gpu_circuit *c, const vc::CircuitView &v, const vc::Layout &L, const uint8_t *cproofs, const size_t *offsets, size_t batch,
                std::vector<uint32_t> &reason, std::vector<size_t> &slot, std::vector<uint32_t> &tabs);
// p2gpu_last_error for the lowest failing proof, in p2gpu_verify_compressed's words; the batch's return code
int cbatch_finish(size_t batch, const p2gpu_verify_report *reports);

}  // namespace p2
