// prover_internal.hpp -- what the translation units of the prover share: commit.hip (commitment operators), upload.hip (the
// host-witness pipeline), prover.hip (the proof and its entry points) and handle.hip (the circuit handle, the stage-level operators).
#pragma once
#include "circuit.hpp"
#include "transport.hpp"
#include <algorithm>
#include <cstdio>
#include <memory>
#include <string>
#include <thread>
#include <utility>
#include <vector>

namespace p2 {
#define TRACE(c, label)                                                                     \
  do {                                                                                      \
    if (p2::trace_on()) {                                                                   \
      hipError_t e_ = hipStreamSynchronize((c)->stream);                                    \
      fprintf(stderr, "[p2gpu] %s: %s\n", label, e_ == hipSuccess ? "ok" : hipGetErrorString(e_)); \
      fflush(stderr);                                                                       \
    }                                                                                       \
  } while (0)

// the refusal of a verifier-only handle by every entry point that needs prover state (0: c is a prover handle)
inline int prover_handle(const p2gpu_circuit *c) {
  if (c->device >= 0) return 0;
  set_err("this is a verifier-only handle (p2gpu_verifier_create): no prover state");
  return P2GPU_E_ARG;
}

// the public inputs of one witness against the circuit's count, each a canonical field element (0: acceptable)
inline int check_public_inputs(const p2gpu_circuit *c, const uint64_t *pis, uint32_t n_pi) {
  if (n_pi != c->num_pi || (n_pi && !pis)) {
    set_err("expected %u public inputs, got %u", c->num_pi, n_pi);
    return P2GPU_E_ARG;
  }
  for (uint32_t i = 0; i < n_pi; i++)
    if (pis[i] >= GL_P) {
      set_err("public input %u is not a canonical field element", i);
      return P2GPU_E_ARG;
    }
  return 0;
}

// ---- check.hip ----
// p2gpu_check_witness_dev behind its argument checks: `batch` witnesses [batch][W][n] resident on c's device, c a plain prover handle
int check_witness_impl(p2gpu_circuit *c, const gl_t *wires_dev, size_t batch, const uint64_t *pis, uint32_t n_pi,
                       p2gpu_witness_report *reports, uint16_t *row_status, uint8_t *cell_flags);

// ---- prover.hip ----
// P2GPU_TRACE=1: synchronise after every phase and report progress on stderr (debugging aid)
bool trace_on();
double now_ms();
// P2GPU_HOSTPROF=1: host-side timestamps at the transcript sync points of one proof (no extra synchronisation), printed
// at the end of prove: where the host sits between GPU phases.  One per host thread.
struct HostProf {
  std::vector<std::pair<const char *, double>> ev;
  void mark(const char *label);
  void dump();
};
extern thread_local HostProf g_hp;
// per-launch timing with HIP events on the launch stream (knob "profile")
struct EventProf : Prof {
  p2gpu_circuit *c;
  hipEvent_t a = nullptr, b = nullptr;
  const char *name = nullptr;
  double bytes = 0;
  bool active = false;
  explicit EventProf(p2gpu_circuit *c_) : c(c_) {}
  hipEvent_t get();  // from the handle's pool
  void begin(const char *k, double by) override;
  void end() override;
};
// ... installed as the calling thread's g_prof for the guard's lifetime when the handle's knob asks for it
struct ProfGuard {
  EventProf prof;
  explicit ProfGuard(p2gpu_circuit *c) : prof(c) { g_prof = c->profile ? &prof : nullptr; }
  ~ProfGuard() { g_prof = nullptr; }
};
void flush_kstats(p2gpu_circuit *c);                 // read the pending per-launch event pairs into c->kstats
int prove_impl(p2gpu_circuit *c, const gl_t *wires_dev, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out, size_t *proof_len,
               p2gpu_timings *tm, double h2d_ms);
// ---- provebatch.hip ----
// frees the slab buffers p2gpu_prove_batch_dev left on the handle (none: nothing to do)
void prove_batch_release(p2gpu_circuit *c);
// ---- commit.hip ----
int pin_exhausted();
const gl_t *hprc(const p2gpu_circuit *c);
int wait_stream(p2gpu_circuit *c);
void tree_layout(Batch &b, uint32_t cosets, size_t m0, size_t cap_per);
int tree_alloc(Batch &b, uint32_t C, size_t m0, size_t cap_per);
int tree_build(p2gpu_circuit *c, Batch &b, size_t m0, uint32_t levels_done = 0);
const uint32_t *batch_colnz(const p2gpu_circuit *c, const Batch &b);
uint32_t virt_first(const p2gpu_circuit *c);
ColHints wire_hints(const p2gpu_circuit *c, uint32_t col0, bool lde);
VirtCols batch_virt(const p2gpu_circuit *c, const Batch &b);
int batch_alloc(p2gpu_circuit *c, Batch &b, uint32_t cols);
int batch_commit_from_values(p2gpu_circuit *c, Batch &b, const gl_t *vals_dev);
int batch_commit_from_coeffs(p2gpu_circuit *c, Batch &b);
// ---- upload.hip ----
int prove_host(p2gpu_circuit *c, const uint64_t *wires, uint32_t ncols, const uint64_t *tail, uint32_t row, const uint64_t *pis,
               uint32_t n_pi, uint8_t *proof_out, size_t *proof_len, p2gpu_timings *tm);
// ---- build.hip: build() on the device (p2gpu_circuit_build) ----
// the caller's arrays, still in host memory (validated on the device before anything indexes with them)
struct BuildInputs {
  const uint32_t *row_gate;        // [n]
  const uint64_t *row_constants;   // [NC - num_selectors][n], nullptr when no gate has constants
  const uint32_t *copies;          // [num_copies][4]
  size_t num_copies;
};
// P2GPU_TRACE=1: where circuit creation spends its time.  t0 is taken once the device is selected; every mark waits for the
// handle's stream first, so its figure covers the device work enqueued so far.
struct CreateTrace {
  p2gpu_circuit *c;
  double t0;
  void mark(const char *label) const {
    if (!trace_on()) return;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    fprintf(stderr, "[p2gpu] create %-28s +%.2f ms\n", label, now_ms() - t0);
  }
};
// The device form of the table phase of circuit creation (handle.hip circuit_finish; the blob form is tables_from_blob there).
// On entry the root tables exist and k_is and the gate table are enqueued on c->stream; both forms leave d_row_gate, d_gconsts,
// d_sigmas, sparse_row and sparse_rows behind.  Every scratch buffer is gone when it returns.
int build_device_tables(p2gpu_circuit *c, const BuildInputs &in, const CreateTrace &tr);
// consts [num_selectors][n] <- the selector columns of d_row_gate (row of a gate outside the column's group: 2^32 - 1)
void build_selector_columns(hipStream_t st, const p2gpu_circuit *c, gl_t *consts);
// ---- handle.hip ----
int ensure_device();
extern int g_device;
extern std::vector<int> g_devices, g_peer_access;
void circuit_release(p2gpu_circuit *c);
// Owner of a handle from `new` until it is handed to the caller.  Whatever leaves creation early -- a refusal, a device error,
// an exception on its way to P2GPU_CATCH -- destroys the handle the way the caller would have (p2gpu_circuit_destroy: the device
// state through circuit_release; none, and no device call, for a verifier-only handle); the thread's error message survives.
struct HalfBuiltDelete {
  void operator()(p2gpu_circuit *c) const {
    const std::string keep = last_error_copy();
    p2gpu_circuit_destroy(c);
    last_error_restore(keep);
  }
};
using HalfBuilt = std::unique_ptr<p2gpu_circuit, HalfBuiltDelete>;

// run f(rank handle, rank) on one host thread per rank of a device group (rank 0 on the caller's thread); a rank
// that fails releases the others from their rendezvous.  Returns the first failing rank's code with its message.
template <class F>
inline int group_run(p2gpu_circuit *c, F f) {
  const int n = 1 + (int)c->group.size();
  std::vector<int> rcs(n, 0);
  std::vector<std::string> errs(n);
  c->peer->reset();
  auto work = [&](int q) {
    p2gpu_circuit *m = q ? c->group[q - 1] : c;
    int rc;
    try {
      rc = f(m, q);
    } catch (const std::exception &e) {
      set_err("internal error: %s", e.what());
      rc = P2GPU_E_DEVICE;
    }
    if (rc) {
      errs[q] = p2gpu_last_error();
      c->peer->abort();
    }
    rcs[q] = rc;
  };
  std::vector<std::thread> th;
  for (int q = 1; q < n; q++) th.emplace_back(work, q);
  work(0);
  for (auto &t : th) t.join();
  (void)hipSetDevice(c->device);
  // prefer the code of a rank that failed on its own over "another rank failed"
  int first = -1;
  for (int q = 0; q < n; q++)
    if (rcs[q] && (first < 0 || (errs[first].find("another rank") != std::string::npos && errs[q].find("another rank") == std::string::npos))) first = q;
  if (first < 0) return P2GPU_OK;
  set_err("%s%s", errs[first].c_str(), n > 1 ? (" (device group rank " + std::to_string(first) + ")").c_str() : "");
  return rcs[first];
}

}  // namespace p2
