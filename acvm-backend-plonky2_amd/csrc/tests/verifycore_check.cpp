// verifycore_check.cpp -- the verifier core (verifycore.hpp) on a verifier key and a proof, without the library and without a
// GPU (tests/test_verifycore_host.py compares what it prints with p2gpu_verify_batch_host on the same byte strings).
//   g++ -O2 -std=c++17 -Wall -Werror -o verifycore_check verifycore_check.cpp && ./verifycore_check VK PROOF SEED COUNT [LEN ...] > OUT
// VK: the verifier's share of a circuit blob (header | gate table | cap | k_is, as p2gpu_circuit_export_vk writes it).
// Cases, in this order: the proof as it is; the proof cut (or zero-extended) to every LEN; COUNT single-bit flips drawn from SEED
// by step() below.  Every case is verified in a heap block of exactly its own length, so that a read past its end is the
// sanitizer's to find.  OUT: per case "reason query index well_formed", then "counts" and the number of cases per reason code.
// Checked here, by abort: a case that is not well_formed() is not accepted, and on the proof as it is head_challenges() alone
// leaves the HeadRecord that verify_head() leaves.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../verifycore.hpp"

using namespace p2;

static std::vector<uint8_t> slurp(const char *path) {
  std::vector<uint8_t> v;
  FILE *f = std::fopen(path, "rb");
  if (!f) return v;
  uint8_t buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + n);
  std::fclose(f);
  return v;
}

// the generator both sides draw the flips from: Knuth's 64-bit LCG, the position and the bit from its high bits
static uint64_t step(uint64_t &s) {
  s = s * 6364136223846793005ULL + 1442695040888963407ULL;
  return s >> 24;
}

int main(int argc, char **argv) {
  if (argc < 5) { std::fprintf(stderr, "usage: verifycore_check VK PROOF SEED COUNT [LEN ...]\n"); return 2; }
  const std::vector<uint8_t> vk = slurp(argv[1]), proof = slurp(argv[2]);
  uint64_t seed = std::strtoull(argv[3], nullptr, 10);
  const size_t count = std::strtoull(argv[4], nullptr, 10);
  if (vk.size() < 256 || proof.empty()) { std::fprintf(stderr, "cannot read the key or the proof\n"); return 2; }
  // ---- the key (the test wrote it with the library: trusted, but its size is checked) ----
  uint32_t h[64];
  std::memcpy(h, vk.data(), sizeof h);
  vc::CircuitView c;
  std::memset(&c, 0, sizeof c);
  c.d = h[2]; c.W = h[3]; c.R = h[4]; c.NC = h[5]; c.num_selectors = h[6]; c.K = h[7]; c.QF = h[8]; c.rate_bits = h[9]; c.cap_h = h[10];
  c.pow_bits = h[11]; c.num_queries = h[12]; c.n_steps = h[13];
  for (int i = 0; i < 8; i++) c.arity[i] = h[14 + i];
  c.hasher = h[22]; c.num_gates = h[23]; c.num_pi = h[24]; c.PP = h[26];
  c.nchunks = (c.R + c.QF - 1) / c.QF;
  const size_t ncap = (size_t)1 << c.cap_h;
  if (c.num_gates > 64 || c.cap_h > 16 || c.n_steps > 8 || c.K > 2 || c.num_queries > 64 ||
      vk.size() != 256 + 48 * (size_t)c.num_gates + 32 * ncap + 8 * (size_t)c.R) {
    std::fprintf(stderr, "not a verifier key\n");
    return 2;
  }
  std::vector<GateDesc> gates(c.num_gates);
  for (uint32_t i = 0; i < c.num_gates; i++) {
    uint32_t g[12];
    std::memcpy(g, vk.data() + 256 + 48 * (size_t)i, sizeof g);
    GateDesc &G = gates[i];
    G.kind = g[0];
    std::memcpy(G.p, &g[1], 16);
    G.sel_index = g[5]; G.group_start = g[6]; G.group_end = g[7]; G.num_constraints = g[8]; G.degree = g[9]; G.num_constants = g[10]; G.pad = 0;
    if (G.num_constraints > c.max_gate_constraints) c.max_gate_constraints = G.num_constraints;
  }
  std::vector<dig_t> cap(ncap);
  std::memcpy((void *)cap.data(), vk.data() + 256 + 48 * (size_t)c.num_gates, 32 * ncap);
  std::vector<gl_t> k_is(c.R);
  std::memcpy(k_is.data(), vk.data() + vk.size() - 8 * (size_t)c.R, 8 * (size_t)c.R);
  std::memset(&c.circuit_digest, 0, sizeof c.circuit_digest);
  std::memcpy(c.circuit_digest.w, &h[32], c.hasher ? 32 : 25);
  std::vector<gl_t> rc(360), prc(360);
  poseidon_round_constants_host(rc.data());
  poseidon_device_constants(rc.data(), prc.data());
  c.gates = gates.data(); c.k_is = k_is.data(); c.cs_cap = cap.data(); c.prc = prc.data();
  const vc::Layout L = vc::make_layout(c);

  std::vector<ext_t> terms(vc::identity_terms(c));
  std::vector<size_t> counts(vc::VR_COUNT, 0);
  auto run = [&](const uint8_t *src, size_t have, size_t len, long flip_at, unsigned bit) {
    uint8_t *p = (uint8_t *)std::malloc(len ? len : 1);  // exactly the case's bytes
    if (!p) std::abort();
    for (size_t i = 0; i < len; i++) p[i] = i < have ? src[i] : 0;
    if (flip_at >= 0) p[flip_at] ^= (uint8_t)(1u << bit);
    gl_t sponge[12];
    vc::HeadRecord rec;
    std::memset(&rec, 0, sizeof rec);
    const vc::Verdict v = c.hasher ? vc::verify_one<1>(c, L, p, len, sponge, terms.data(), &rec) : vc::verify_one<0>(c, L, p, len, sponge, terms.data(), &rec);
    const bool wf = c.hasher ? vc::well_formed<1>(c, L, p, len) : vc::well_formed<0>(c, L, p, len);
    if (!wf && !v.reason) { std::fprintf(stderr, "accepted, but not well-formed\n"); std::abort(); }
    if (src == proof.data() && len == proof.size() && flip_at < 0) {  // the proof as it is: the transcript alone leaves verify_head's record
      gl_t betas[vc::VC_MAX_CHALLENGES], gammas[vc::VC_MAX_CHALLENGES], alphas[vc::VC_MAX_CHALLENGES], pih[4];
      vc::HeadRecord mine;
      std::memset(&mine, 0, sizeof mine);
      const vc::Strided<gl_t> sp{sponge, 1};
      if (c.hasher) vc::head_challenges<1>(c, L, p, sp, betas, gammas, alphas, pih, &mine);
      else vc::head_challenges<0>(c, L, p, sp, betas, gammas, alphas, pih, &mine);
      if (std::memcmp(&mine, &rec, sizeof rec)) { std::fprintf(stderr, "head_challenges and verify_head leave different records\n"); std::abort(); }
    }
    std::free(p);
    std::printf("%u %u %u %d\n", v.reason, v.query, v.index, (int)wf);
    counts[v.reason < vc::VR_COUNT ? v.reason : 0]++;
  };
  run(proof.data(), proof.size(), proof.size(), -1, 0);
  for (int i = 5; i < argc; i++) run(proof.data(), proof.size(), std::strtoull(argv[i], nullptr, 10), -1, 0);
  for (size_t k = 0; k < count; k++) {
    const uint64_t r = step(seed);
    run(proof.data(), proof.size(), proof.size(), (long)((r >> 3) % proof.size()), (unsigned)(r & 7));
  }
  std::printf("counts");
  for (size_t n : counts) std::printf(" %zu", n);
  std::printf("\n");
  return 0;
}
