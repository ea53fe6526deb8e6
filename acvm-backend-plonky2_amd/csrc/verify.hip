// verify.hip -- proof verification on the host (no kernel in this file): the verifier-only handle, the verifier key, and the
// host entry points of the verifier core -- p2gpu_verify (one proof), p2gpu_verify_batch_host (a plain loop over a batch) and
// p2gpu_verify_reason (the wording of a report).  The checks themselves are in verifycore.hpp, written once for the host and
// the device; p2gpu_verify_batch runs the same functions as kernels (verifydev.hip).
//
// The reference's `verify` action (plonky2-backend/src/actions/verify_action.rs:11-17,
// VerifierCircuitData::verify) and the assertion every in-tree test ends with
// (`circuit_data.verify(proof)`, e.g. circuit_translation/tests/factories/utils.rs:26-27) check a
// proof in a few milliseconds of scalar work; so does p2gpu_verify -- it is what SURVEY.md 8(b) calls
// `p2gpu-verify`, and it needs no GPU: a handle made by p2gpu_verifier_create holds only the
// verifier's share of the circuit (parameters, gate table, constants_sigmas cap, circuit digest,
// k_is) -- the counterpart of the VK file written by actions/write_vk_action.rs:65-81.
//
// Checks, in plonky2 0.2.2 order (plonk/verifier.rs verify_with_challenges, fri/verifier.rs
// verify_fri_proof):  shape of the byte string -> transcript replay -> plonk identity at zeta ->
// proof-of-work -> per query: Merkle paths of the four initial oracles, the combined quotient
// value, every arity-16 fold (closed-form barycentric interpolation on the coset s<g_16>), the
// final polynomial.  Proof layout: SURVEY.md C.11; it accepts the reference's own proofs
// (tests/test_reference_proofs.py::test_product_verifier_accepts_reference_proof).
#include "hostproof.hpp"
#include "prover_internal.hpp"
#include <algorithm>
#include <cstdio>

using namespace p2;

namespace p2 {

// The verifier's plonk identity at zeta, on the opened values (verifycore.hpp plonk_identity_core).
// `op` = constants, sigmas, wires, zs, partial products, quotient chunks, then zs_next.
// It fails exactly when the witness does not satisfy the circuit (with overwhelming
// probability); upstream only finds that out in its witness generator, which stays in Rust, so
// the prover runs this as its self-check too.
bool plonk_identity_holds(const p2gpu_circuit *c, const std::vector<ext_t> &op, const gl_t *betas, const gl_t *gammas,
                          const gl_t *alphas, ext_t zeta, const gl_t pih[4]) {
  const vc::CircuitView v = view_of(c);
  std::vector<ext_t> terms(vc::identity_terms(v));
  return vc::plonk_identity_at(v, vc::Openings{op.data(), nullptr, 0, 0, 0, 0}, vc::Strided<ext_t>{terms.data(), 1}, betas, gammas, alphas, zeta, pih);
}

// ---- what the batch entry points share (p2gpu_verify_batch_host below, p2gpu_verify_batch in verifydev.hip) ----
int verify_batch_args(const p2gpu_circuit *c, const uint8_t *proofs, const size_t *offsets, size_t batch, const void *reports) {
  if (!c || !proofs || !offsets || !reports || batch == 0) return P2GPU_E_ARG;
  for (size_t b = 0; b < batch; b++)
    if (offsets[b + 1] < offsets[b]) {
      set_err("p2gpu_verify_batch: offsets decrease at proof %zu", b);
      return P2GPU_E_ARG;
    }
  if (!c->group.empty()) {
    set_err("p2gpu_verify_batch: a device group verifies nothing as a group: use a plain handle (p2gpu_circuit_create_on) or a verifier-only one");
    return P2GPU_E_ARG;
  }
  if (c->cs.cap.size() != (size_t)1 << c->cap_h) return P2GPU_E_ARG;
  return 0;
}

void verify_report_fill(p2gpu_verify_report *r, const vc::Verdict &v) {
  r->status = v.reason ? P2GPU_E_VERIFY : P2GPU_OK;
  r->reason = v.reason;
  r->query = v.query;
  r->index = v.index;
}

// p2gpu_last_error for the lowest failing proof, in p2gpu_verify's words; the batch's return code
int verify_batch_finish(size_t batch, const size_t *offsets, const vc::Layout &L, const p2gpu_verify_report *reports) {
  for (size_t b = 0; b < batch; b++) {
    const p2gpu_verify_report &r = reports[b];
    if (r.status == P2GPU_OK) continue;
    char text[400], who[48] = "";
    if (r.reason == vc::VR_LENGTH) vc::reason_text(r.reason, offsets[b + 1] - offsets[b], L.want, text, sizeof text);
    else vc::reason_text(r.reason, r.query, r.index, text, sizeof text);
    if (batch > 1) snprintf(who, sizeof who, "proof %zu of the batch: ", b);
    set_err("%sproof rejected: %s", who, text);
    return P2GPU_E_VERIFY;
  }
  return P2GPU_OK;
}

vc::Verdict verify_one_host(const vc::CircuitView &v, const vc::Layout &L, const uint8_t *proof, size_t len, std::vector<ext_t> &terms) {
  gl_t sponge[12];
  vc::HeadRecord rec;
  terms.resize(vc::identity_terms(v));
  return v.hasher ? vc::verify_one<1>(v, L, proof, len, sponge, terms.data(), &rec) : vc::verify_one<0>(v, L, proof, len, sponge, terms.data(), &rec);
}

}  // namespace p2

extern "C" {

int p2gpu_verifier_create(const uint8_t *blob, size_t len, p2gpu_circuit **out) try {
  if (!blob || !out) return P2GPU_E_ARG;
  HalfBuilt c(new p2gpu_circuit());
  c->device = -1;  // no device state: only p2gpu_verify and the getters accept this handle
  size_t off = 0;
  const uint8_t *cap_in = nullptr;
  if (int rc = circuit_parse(blob, len, c.get(), &off, &cap_in)) return rc;
  if ((c->flags & 3) != 3 || !cap_in) {
    set_err("a verifier handle needs the circuit digest and the constants_sigmas cap in the blob (flags 0b11)");
    return P2GPU_E_BLOB;
  }
  c->cs.cap.resize((size_t)1 << c->cap_h);
  for (size_t i = 0; i < c->cs.cap.size(); i++) {
    memset(&c->cs.cap[i], 0, sizeof(dig_t));
    memcpy(c->cs.cap[i].w, cap_in + 32 * i, digest_bytes(c->hasher));
  }
  if (c->hasher) {  // Poseidon digests are field elements: canonical encodings only (as verifycore.hpp ld_digest asks of a proof)
    bool canon = true;
    for (auto &dg : c->cs.cap)
      for (int i = 0; i < 4; i++) canon &= dg.w[i] < GL_P;
    for (int i = 0; i < 4; i++) canon &= c->circuit_digest.w[i] < GL_P;
    if (!canon) {
      set_err("verifier key holds a non-canonical Poseidon digest word");
      return P2GPU_E_BLOB;
    }
  }
  *out = c.release();
  return P2GPU_OK;
} P2GPU_CATCH

// header | gate table | cap | k_is: the verifier's share of a circuit blob
int p2gpu_circuit_export_vk(const p2gpu_circuit *c, uint8_t *out, size_t *len) try {
  if (!c || !len) return P2GPU_E_ARG;
  const size_t ncap = (size_t)1 << c->cap_h;
  const size_t need = 256 + 48 * (size_t)c->num_gates + 32 * ncap + 8 * (size_t)c->R;
  if (!out || *len < need) {
    *len = need;
    if (out) set_err("verifier blob needs %zu bytes", need);
    return out ? P2GPU_E_BUFFER : P2GPU_OK;
  }
  if (c->cs.cap.size() != ncap) return P2GPU_E_ARG;
  uint32_t h[64];
  memset(h, 0, sizeof h);
  h[0] = 0x43473250u; h[1] = 1; h[2] = c->d; h[3] = c->W; h[4] = c->R; h[5] = c->NC; h[6] = c->num_selectors;
  h[7] = c->K; h[8] = c->QF; h[9] = c->rate_bits; h[10] = c->cap_h; h[11] = c->pow_bits; h[12] = c->num_queries;
  h[13] = c->n_steps;
  for (int i = 0; i < 8; i++) h[14 + i] = c->arity[i];
  h[22] = c->hasher; h[23] = c->num_gates; h[24] = c->num_pi; h[25] = 3; h[26] = c->PP;
  memcpy(&h[32], c->circuit_digest.w, digest_bytes(c->hasher));
  memcpy(out, h, sizeof h);
  size_t off = 256;
  for (const GateDesc &G : c->gates) {
    uint32_t g[12];
    memset(g, 0, sizeof g);
    g[0] = G.kind;
    memcpy(&g[1], G.p, 16);
    g[5] = G.sel_index; g[6] = G.group_start; g[7] = G.group_end; g[8] = G.num_constraints; g[9] = G.degree;
    g[10] = G.num_constants;
    memcpy(out + off, g, sizeof g);
    off += sizeof g;
  }
  for (size_t i = 0; i < ncap; i++) {
    memset(out + off, 0, 32);
    memcpy(out + off, c->cs.cap[i].w, digest_bytes(c->hasher));
    off += 32;
  }
  memcpy(out + off, c->k_is.data(), 8 * (size_t)c->R);
  off += 8 * (size_t)c->R;
  *len = off;
  return P2GPU_OK;
} P2GPU_CATCH

int p2gpu_verify(const p2gpu_circuit *c, const uint8_t *proof, size_t len) try {
  if (!c || !proof) return P2GPU_E_ARG;
  if (c->cs.cap.size() != (size_t)1 << c->cap_h) return P2GPU_E_ARG;
  const vc::CircuitView v = view_of(c);
  const vc::Layout L = vc::make_layout(v);
  std::vector<ext_t> terms;
  const vc::Verdict vd = verify_one_host(v, L, proof, len, terms);
  if (!vd.reason) return P2GPU_OK;
  char text[400];
  if (vd.reason == vc::VR_LENGTH) vc::reason_text(vd.reason, len, L.want, text, sizeof text);
  else vc::reason_text(vd.reason, vd.query, vd.index, text, sizeof text);
  set_err("proof rejected: %s", text);
  return P2GPU_E_VERIFY;
} P2GPU_CATCH

// the core in a plain loop on the calling thread: no device is touched
int p2gpu_verify_batch_host(const p2gpu_circuit *c, const uint8_t *proofs, const size_t *offsets, size_t batch, p2gpu_verify_report *reports) try {
  if (int rc = verify_batch_args(c, proofs, offsets, batch, reports)) return rc;
  const vc::CircuitView v = view_of(c);
  const vc::Layout L = vc::make_layout(v);
  std::vector<ext_t> terms;
  for (size_t b = 0; b < batch; b++) {
    const size_t len = offsets[b + 1] - offsets[b];
    verify_report_fill(&reports[b], verify_one_host(v, L, proofs + offsets[b], len, terms));
  }
  return verify_batch_finish(batch, offsets, L, reports);
} P2GPU_CATCH

int p2gpu_verify_reason(const p2gpu_verify_report *r, char *out, size_t cap) {
  if (!r || !out || cap == 0) return P2GPU_E_ARG;
  const char *words = dc::reason_words(r->reason);  // a reject site of the decompression: the text behind "malformed proof: "
  const int n = words ? snprintf(out, cap, "%s", words) : vc::reason_text(r->reason, r->query, r->index, out, cap);
  if (n < 0 || (size_t)n >= cap) {
    set_err("p2gpu_verify_reason: the text needs %d bytes", n + 1);
    return P2GPU_E_BUFFER;
  }
  return P2GPU_OK;
}

}  // extern "C"
