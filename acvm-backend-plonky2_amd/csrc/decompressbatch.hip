// decompressbatch.hip -- a batch of on-disk (compressed) proofs, the host's share (no kernel in this file): what
// p2gpu_verify_batch_compressed_host, p2gpu_verify_batch_compressed and p2gpu_proof_decompress_batch (decompressdev.hip) have
// in common -- the container walk with the lone path's answer for a proof the walk gives up on, the wording of
// the lowest failing proof -- and p2gpu_verify_batch_compressed_host itself: the core (decompresscore.hpp, then
// verifycore.hpp) in a plain loop on the calling thread, its test bed and its sanitised build.
// The verdict of proof b is p2gpu_verify_compressed's on that byte string (proofio.hip, untouched: the oracle of all this).
#include "hostproof.hpp"

using namespace p2;

namespace p2 {

// The lone path's verdict on a proof the walk gave up on: p2gpu_verify_compressed rejects it at one of decompress's sites, and
// its words name the site.  0: it did not (an internal error; p2gpu_last_error says what it answered).
static uint32_t lone_reason(const p2gpu_circuit *c, const uint8_t *p, size_t len) {
  const int rc = p2gpu_verify_compressed(c, p, len);
  const std::string said = last_error_copy();
  static const char prefix[] = "malformed proof: ";
  if (rc == P2GPU_E_VERIFY && said.compare(0, sizeof prefix - 1, prefix) == 0)
    for (uint32_t r = dc::VR_C_ARITY; r < dc::VR_C_END; r++)
      if (said.compare(sizeof prefix - 1, std::string::npos, dc::reason_words(r)) == 0) return r;
  set_err("p2gpu_verify_batch_compressed: internal error: the container walk refused what p2gpu_verify_compressed answers with %d (%s)", rc, said.c_str());
  return 0;
}

int cbatch_walk(const p2gpu_circuit *c, const vc::CircuitView &v, const vc::Layout &L, const uint8_t *cproofs, const size_t *offsets, size_t batch,
                std::vector<uint32_t> &reason, std::vector<size_t> &slot, std::vector<uint32_t> &tabs) {
  const size_t tw = dc::table_words(v);
  reason.assign(batch, vc::VR_OK);
  slot.clear();
  tabs.clear();
  std::vector<uint32_t> tab(tw);
  for (size_t b = 0; b < batch; b++) {
    const uint8_t *p = cproofs + offsets[b];
    const size_t len = offsets[b + 1] - offsets[b];
    if (L.bad_arity) reason[b] = dc::VR_C_ARITY;
    else if (dc::walk(v, L, p, len, tab.data())) {
      slot.push_back(b);
      tabs.insert(tabs.end(), tab.begin(), tab.end());
    } else if (!(reason[b] = lone_reason(c, p, len))) return P2GPU_E_DEVICE;
  }
  return 0;
}

int cbatch_finish(size_t batch, const p2gpu_verify_report *reports) {
  for (size_t b = 0; b < batch; b++) {
    const p2gpu_verify_report &r = reports[b];
    if (r.status == P2GPU_OK) continue;
    char text[400], who[48] = "";
    if (batch > 1) snprintf(who, sizeof who, "proof %zu of the batch: ", b);
    if (const char *words = dc::reason_words(r.reason)) set_err("%smalformed proof: %s", who, words);
    else {
      vc::reason_text(r.reason, r.query, r.index, text, sizeof text);
      set_err("%sproof rejected: %s", who, text);
    }
    return P2GPU_E_VERIFY;
  }
  return P2GPU_OK;
}

}  // namespace p2

namespace {

template <int HK>
vc::Verdict one(const vc::CircuitView &v, const vc::Layout &L, const uint8_t *cp, const uint32_t *tab, std::vector<uint8_t> &out, std::vector<ext_t> &terms) {
  gl_t sponge[12];
  vc::HeadRecord rec;
  memset(&rec, 0, sizeof rec);
  uint32_t head_reason = vc::VR_OK;
  out.assign(L.want, 0);
  terms.resize(vc::identity_terms(v));
  if (const uint32_t flags = dc::decompress_one<HK>(v, L, cp, tab, out.data(), sponge, terms.data(), &rec, true, &head_reason))
    return vc::Verdict{dc::flags_reason(flags), vc::VR_NONE, vc::VR_NONE};
  if (head_reason) return vc::Verdict{head_reason, vc::VR_NONE, vc::VR_NONE};
  for (uint32_t q = 0; q < v.num_queries; q++) {
    uint32_t index = vc::VR_NONE;
    if (const uint32_t r = vc::verify_query<HK>(v, L, out.data(), &rec, q, &index)) return vc::Verdict{r, q, index};
  }
  return vc::Verdict{vc::VR_OK, vc::VR_NONE, vc::VR_NONE};
}

}  // namespace

// the core in a plain loop on the calling thread: no device is touched
extern "C" int p2gpu_verify_batch_compressed_host(const p2gpu_circuit *c, const uint8_t *cproofs, const size_t *offsets, size_t batch,
                                                  p2gpu_verify_report *reports) try {
  if (int rc = verify_batch_args(c, cproofs, offsets, batch, reports)) return rc;
  const vc::CircuitView v = view_of(c);
  const vc::Layout L = vc::make_layout(v);
  std::vector<uint32_t> reason, tabs;
  std::vector<size_t> slot;
  if (int rc = cbatch_walk(c, v, L, cproofs, offsets, batch, reason, slot, tabs)) return rc;
  for (size_t b = 0; b < batch; b++) verify_report_fill(&reports[b], vc::Verdict{reason[b], vc::VR_NONE, vc::VR_NONE});
  std::vector<uint8_t> out;
  std::vector<ext_t> terms;
  const size_t tw = dc::table_words(v);
  for (size_t i = 0; i < slot.size(); i++) {
    const uint8_t *cp = cproofs + offsets[slot[i]];
    const uint32_t *tab = tabs.data() + i * tw;
    verify_report_fill(&reports[slot[i]], v.hasher ? one<1>(v, L, cp, tab, out, terms) : one<0>(v, L, cp, tab, out, terms));
  }
  return cbatch_finish(batch, reports);
} P2GPU_CATCH
