// cbatch_check.cpp -- the batch decompressor's core in its host loop (p2gpu_verify_batch_compressed_host: decompresscore.hpp,
// then verifycore.hpp) against the lone p2gpu_verify_compressed (proofio.hip, sequential, with maps) on seeded mutations of a
// compressed proof: every member's report must carry the lone call's code and words.  Plain C ABI, its own main; `make asan`
// links it against the sanitised kernel-free library.
//
//   cbatch_check <vk.blob> <compressed.bin> <mutations> <seed>
// exit 0 = every report agrees (counts on stdout), 1 = usage / io / the untouched proof is not accepted, 2 = a difference.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../../include/p2gpu.h"

static uint64_t rng_state;
static uint64_t rnd() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

static bool slurp(const char *path, std::vector<uint8_t> &out) {
  FILE *f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[4096];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

static std::vector<uint8_t> mutate(const std::vector<uint8_t> &src) {
  std::vector<uint8_t> m = src;
  switch (rnd() % 8) {
  case 0: m.resize(rnd() % (src.size() + 1)); break;                                    // truncate
  case 1: for (uint64_t k = 1 + rnd() % 40; k--;) m.push_back((uint8_t)rnd()); break;   // trailing bytes
  case 2: case 3: case 4: m[rnd() % m.size()] ^= (uint8_t)(1u << (rnd() % 8)); break;   // one bit
  case 5: {                                                                             // a word that is no field element
    static const uint64_t V[] = {0xFFFFFFFF00000001ull, 0xFFFFFFFFFFFFFFFFull, 0xFFFFFFFF00000002ull};
    const uint64_t v = V[rnd() % 3];
    if (m.size() >= 8) memcpy(&m[rnd() % (m.size() - 7)], &v, 8);
    break;
  }
  case 6: m[rnd() % m.size()] = (uint8_t)rnd(); break;                                  // one byte
  case 7: {                                                                             // a random run
    const size_t a = rnd() % m.size(), l = 1 + rnd() % 48;
    for (size_t i = a; i < m.size() && i < a + l; i++) m[i] = (uint8_t)rnd();
    break;
  }
  }
  return m;
}

int main(int argc, char **argv) {
  if (argc < 5) {
    fprintf(stderr, "usage: %s <vk.blob> <compressed.bin> <mutations> <seed>\n", argv[0]);
    return 1;
  }
  std::vector<uint8_t> blob, comp;
  if (!slurp(argv[1], blob) || !slurp(argv[2], comp) || comp.empty()) {
    fprintf(stderr, "cannot read inputs\n");
    return 1;
  }
  const long count = atol(argv[3]);
  rng_state = strtoull(argv[4], nullptr, 0);
  p2gpu_circuit *vd = nullptr;
  if (p2gpu_verifier_create(blob.data(), blob.size(), &vd) || p2gpu_verify_compressed(vd, comp.data(), comp.size())) {
    fprintf(stderr, "the unmutated inputs are not accepted: %s\n", p2gpu_last_error());
    return 1;
  }
  // one batch: the mutations, an untouched proof in front, after every eighth and at the end
  std::vector<std::vector<uint8_t>> members{comp};
  for (long i = 0; i < count; i++) {
    members.push_back(mutate(comp));
    if (i % 8 == 7 || i == count - 1) members.push_back(comp);
  }
  std::vector<uint8_t> bytes{0};  // (a valid pointer for an empty first member)
  std::vector<size_t> offsets{1};
  for (auto &m : members) {
    bytes.insert(bytes.end(), m.begin(), m.end());
    offsets.push_back(bytes.size());
  }
  std::vector<p2gpu_verify_report> reports(members.size());
  const int rc = p2gpu_verify_batch_compressed_host(vd, bytes.data(), offsets.data(), members.size(), reports.data());
  const std::string batch_error = rc ? p2gpu_last_error() : "";
  long differences = 0, accepted = 0, malformed = 0, rejected = 0;
  bool first_failure = true;
  for (size_t b = 0; b < members.size(); b++) {
    const int lone = members[b] == comp ? P2GPU_OK : p2gpu_verify_compressed(vd, bytes.data() + offsets[b], offsets[b + 1] - offsets[b]);
    const std::string said = lone ? p2gpu_last_error() : "";
    const p2gpu_verify_report &r = reports[b];
    char words[400] = "";
    std::string expect;
    bool same = r.status == lone && p2gpu_verify_reason(&r, words, sizeof words) == P2GPU_OK;
    if (lone == P2GPU_OK) {
      accepted++;
      same = same && r.reason == P2GPU_VR_OK && !strcmp(words, "accepted");
    } else {
      const bool container = r.reason >= P2GPU_VR_C_ARITY;
      (container ? malformed : rejected)++;
      expect = std::string(container ? "malformed proof: " : "proof rejected: ") + words;
      same = same && lone == P2GPU_E_VERIFY && r.reason != P2GPU_VR_OK && said == expect;
      if (container) same = same && r.query == UINT32_MAX && r.index == UINT32_MAX;
      if (first_failure) {  // p2gpu_last_error of the batch words the lowest failing proof
        char who[64];
        snprintf(who, sizeof who, "proof %zu of the batch: ", b);
        same = same && rc == P2GPU_E_VERIFY && batch_error == (members.size() > 1 ? who + said : said);
        first_failure = false;
      }
    }
    if (!same) {
      differences++;
      fprintf(stderr, "member %zu (%zu bytes): lone %d \"%s\", batch status %d reason %u \"%s\"\n", b, offsets[b + 1] - offsets[b], lone, said.c_str(),
              r.status, r.reason, words);
    }
  }
  if (first_failure && rc != P2GPU_OK) differences++;
  printf("members %zu accepted %ld malformed %ld rejected %ld DIFFERENCES %ld\n", members.size(), accepted, malformed, rejected, differences);
  p2gpu_circuit_destroy(vd);
  return differences ? 2 : 0;
}
