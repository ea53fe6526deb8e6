// provebatch_check.cpp -- the batched prover's bodies and launch sequence (csrc/provebatchcore.hpp) on the host, without the
// library and without a GPU, against the CPU oracle's proof bytes (test infrastructure: tests/test_provebatch_host.py).
//   provebatch_check <blob> <wires> <public inputs> <B>
// A host runner calls every body in the order pb::prove_slab enqueues the kernels -- one thread per block, so the barriers are
// no-ops --, on B copies of the witness; the handle's tables (twiddles, coset scales, the constants/sigmas coefficients, LDE and
// tree in commit.hip's layout) are rebuilt here from the oracle's circuit.  Every buffer is a heap block of exactly the size
// pb::slab_buffers asks for, so a sanitized build sees every index.  Exit code 0: every proof equals the oracle's.
// g++ -std=c++17 -I<repo>/acvm-backend-plonky2_amd/csrc -I<repo>/oracle provebatch_check.cpp -L<repo>/oracle -loracle
#include "provebatchcore.hpp"
#include <vector>
#include <cstdlib>
namespace orc {
extern "C" {
#include "oracle.h"
#include "circuit.h"
const circuit_t *orc_circuit_inner(const orc_circuit *oc);
}
}
#undef GL_P
#undef GL_EPS
using namespace p2;

static std::vector<uint8_t> slurp(const char *path) {
  FILE *f = fopen(path, "rb");
  if (!f) { perror(path); exit(2); }
  std::vector<uint8_t> v;
  uint8_t buf[65536];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}
static dig_t dig_of(const orc::digest_t &d, int hb) {
  dig_t o;
  memset(&o, 0, sizeof o);
  memcpy(o.w, d.b, hb);
  return o;
}
struct HostRun {
  uint32_t launches = 0;
  uint32_t pow_groups() { return 1; }
  uint32_t pow_threads() { return 1; }
  template <void (*F)(const pb::Args &, uint32_t)>
  void lanes(const pb::Args &a, size_t total, const char *) {
    launches++;
    for (size_t g = 0; g < total; g++) F(a, (uint32_t)g);
  }
  template <void (*F)(const pb::Args &, uint32_t, uint32_t, uint32_t, gl_t *)>
  void blocks(const pb::Args &a, size_t nb, uint32_t, size_t lds_words, const char *) {
    launches++;
    std::vector<gl_t> lds(lds_words ? lds_words : 1);
    for (size_t b = 0; b < nb; b++) F(a, (uint32_t)b, 0, 1, lds.data());
  }
};

int main(int argc, char **argv) {
  std::vector<uint8_t> blob = slurp(argv[1]), wbytes = slurp(argv[2]), pbytes = slurp(argv[3]);
  const uint32_t B = atoi(argv[4]);
  orc::orc_circuit *oc;
  if (orc::orc_circuit_create(blob.data(), blob.size(), &oc)) { fprintf(stderr, "blob\n"); return 2; }
  const orc::circuit_t *c = orc::orc_circuit_inner(oc);
  const uint32_t d = c->d, rb = c->rate_bits, C = 1u << rb, lgN = d + rb;
  const size_t n = c->n, N = c->N;
  const int HK = c->hasher == 1, hb = HK ? 32 : 25;
  pb::Args a;
  memset(&a, 0, sizeof a);
  vc::CircuitView &v = a.c;
  v.d = d; v.W = c->num_wires; v.R = c->num_routed; v.NC = c->num_constants; v.num_selectors = c->num_selectors; v.K = c->num_challenges;
  v.QF = c->qdf; v.nchunks = (v.R + v.QF - 1) / v.QF; v.PP = v.nchunks - 1; v.rate_bits = rb; v.cap_h = c->cap_height; v.pow_bits = c->pow_bits;
  v.num_queries = c->num_queries; v.n_steps = c->n_steps;
  for (int i = 0; i < 8; i++) v.arity[i] = c->arity_bits[i];
  v.num_gates = c->num_gates; v.num_pi = c->num_pi; v.max_gate_constraints = c->num_gate_constraints; v.hasher = HK;
  std::vector<GateDesc> gates(v.num_gates);
  for (uint32_t i = 0; i < v.num_gates; i++) {
    const orc::gate_t &g = c->gates[i];
    gates[i] = GateDesc{g.kind, {g.p[0], g.p[1], g.p[2], g.p[3]}, g.sel_index, g.group_start, g.group_end, g.num_constraints, g.degree, g.num_constants, 0};
  }
  v.gates = gates.data();
  v.k_is = c->k_is;
  static gl_t prc[360];
  orc::poseidon_init();
  poseidon_device_constants(orc::poseidon_round_constants(), prc);
  v.prc = prc;
  v.circuit_digest = dig_of(c->circuit_digest, hb);
  a.L = vc::make_layout(v);
  a.nterms = v.K + v.K * v.nchunks + v.max_gate_constraints;
  a.self_check = 1;
  a.dh = d;
  // tables
  std::vector<gl_t> twf(n / 2 + 1), twi(n / 2 + 1), sc(C * n), isc(C * n);
  const gl_t wn = gl_root(d), wni = gl_inv(wn), wN = gl_root(lgN);
  twf[0] = twi[0] = 1;
  for (size_t i = 1; i < n / 2; i++) { twf[i] = gl_mul(twf[i - 1], wn); twi[i] = gl_mul(twi[i - 1], wni); }
  for (uint32_t r = 0; r < C; r++) {
    const gl_t s = gl_mul(GL_GEN, gl_pow(wN, r)), si = gl_inv(s);
    for (size_t e = 0; e < n; e++) { sc[r * n + bitrev32(e, d)] = gl_pow(s, e); isc[r * n + bitrev32(e, d)] = gl_pow(si, e); }
  }
  a.tw_fwd = twf.data(); a.tw_inv = twi.data(); a.scale = sc.data(); a.inv_scale = isc.data();
  a.sigmas = c->sigmas;
  const uint32_t ncs = a.L.ncs;
  std::vector<gl_t> cs_coef(ncs * n), cs_lde((size_t)ncs * N);
  for (uint32_t col = 0; col < ncs; col++)
    for (size_t jx = 0; jx < n; jx++) cs_coef[col * n + bitrev32(jx, d)] = c->cs.coeffs[col * n + jx];
  for (uint32_t r = 0; r < C; r++)
    for (uint32_t col = 0; col < ncs; col++)
      for (size_t k = 0; k < n; k++) cs_lde[((size_t)r * ncs + col) * n + k] = orc::batch_lde_row(&c->cs, k * C + r)[col];
  a.cs_coef = cs_coef.data(); a.cs_lde = cs_lde.data();
  // the handle's tree layout
  std::vector<dig_t> cs_dig(2 * N + 16);
  {
    size_t off = 0;
    for (uint32_t l = 0; l <= a.L.init_len; l++) {
      const size_t m = n >> l;
      a.cs_level_off[l] = off;
      for (uint32_t r = 0; r < C; r++)
        for (size_t k = 0; k < m; k++) {
          if (l == 0) cs_dig[off + r * m + k] = dig_of(c->cs.tree.levels[0][bitrev32(k * C + r, lgN)], hb);
          else {
            const dig_t *below = &cs_dig[a.cs_level_off[l - 1] + r * 2 * m];
            cs_dig[off + r * m + k] = HK ? vc::node_digest_hk<1>(below[k], below[k + m], prc) : vc::node_digest_hk<0>(below[k], below[k + m], prc);
          }
        }
      off += C * m;
    }
  }
  a.cs_dig = cs_dig.data();
  // the slab
  std::vector<gl_t> wires((size_t)B * v.W * n);
  for (uint32_t b = 0; b < B; b++) memcpy(&wires[(size_t)b * v.W * n], wbytes.data(), 8 * (size_t)v.W * n);
  a.wires = wires.data();
  auto take = [](size_t bytes) { return calloc(1, bytes); };
  if (!pb::slab_buffers(a, B, take)) return 2;
  for (uint32_t b = 0; b < B && v.num_pi; b++) memcpy((gl_t *)a.pis + (size_t)b * v.num_pi, pbytes.data(), 8 * (size_t)v.num_pi);
  HostRun run;
  if (HK) pb::prove_slab<1>(run, a); else pb::prove_slab<0>(run, a);
  // the oracle
  std::vector<uint8_t> expect(a.L.want + 1024);
  size_t len = expect.size();
  orc::orc_trace tr;
  int rc = orc::orc_prove(oc, (const uint64_t *)wbytes.data(), (const uint64_t *)pbytes.data(), v.num_pi, UINT64_MAX, expect.data(), &len, &tr);
  printf("oracle rc %d len %zu want %zu launches %u\n", rc, len, a.L.want, run.launches);
  int bad = 0;
  for (uint32_t b = 0; b < B; b++) {
    const pb::Record &r = a.rec[b];
    printf("proof %u status %d beta %d gamma %d alpha %d zeta %d fri_alpha %d pow %llu/%llu q0 %u/%u\n", b, r.status, r.betas[0] == tr.betas[0],
           r.gammas[0] == tr.gammas[0], r.alphas[0] == tr.alphas[0], r.zeta.c0 == tr.zeta[0], r.fri_alpha.c0 == tr.alpha_fri[0],
           r.pow_witness, (unsigned long long)tr.pow_witness, r.qidx[0], tr.query_indices[0]);
    const uint8_t *p = a.proofs + (size_t)b * a.want8;
    size_t first = len;
    for (size_t i = 0; i < len; i++)
      if (p[i] != expect[i]) { first = i; break; }
    if (first != len) {
      bad = 1;
      printf("  FIRST DIFF at %zu (open_at %zu step_caps %zu queries %zu qbytes %zu tail %zu)\n", first, a.L.open_at, a.L.step_caps_at, a.L.queries_at,
             a.L.query_bytes, a.L.tail_at);
    } else printf("  bytes equal\n");
  }
  return bad;
}
