// genwit.hip -- the witness from the solver's values, on the device (SURVEY 8(f) "P2": `generate_partial_witness`,
// iop/generator.rs -- every generator in dependency order, every copy constraint propagated).
//
// Plan (once per circuit and seed set; p2gpu_witness_plan_create: host code, below -- p2gpu_witness_plan_build compiles the same
// plan on the device, genplan.hip, and this one is its differential oracle):
//   classes   sigma is read back and decoded (sigma[x] = k_is[col'] * w^row': the coset of the value names col', the
//             subgroup element row'); the cycles become compact class ids.  A handle from a blob and one from
//             p2gpu_circuit_build hold the same sigma, hence give the same plan.
//   slots     one value slot per class, and one per routed cell outside every class that a seed names or an op writes.
//   ops       the closed registry of generators.hpp, per slot / copy / row as DESIGN 6b lists them; an op none of whose
//             cells has a slot produces nothing (fill_witness derives such rows from zeros afterwards).
//   levels    level 0 = seeds, ConstantGate rows and ops without inputs; an op runs one level above its latest input.
//             The first op (by level, then creation order) that reaches a slot WRITES it -- its cell carries the
//             writer bit -- every other op that derives the same slot COMPARES, one level above the writer at least.
//             A BaseSum row runs in the direction the schedule reaches first.
// Proof (p2gpu_generate_witness): one persistent workgroup walks the levels with a barrier in between (the SHA-256
// compression circuit: 6 170 levels of median width 38 -- a chain, not a wave front), a wide kernel scatters the slot
// values over the routed cells, fill_witness derives the rest.  The first contradiction, by op order, comes back in
// one word after everything is queued.
// Batch (p2gpu_generate_witness_batch): B witnesses of one plan through the SAME kernels.  Only the values are per
// witness -- val[slot][B], seed_vals[seed][B], err[B], the witness index innermost -- and a lane of the walk takes the pair
// (op, witness) with the witness as the fast index: neighbouring lanes run one generator on neighbouring words.  Groups of
// WALK_GROUP witnesses get a workgroup each; a group shares nothing it writes with another, so nothing synchronises across
// workgroups.  The lone call is the batch of one on the plan's own buffers.
#include <chrono>
#include <unordered_map>
#include "generators.hpp"
#include "genplan.hpp"

using namespace p2;

namespace {

constexpr uint32_t UNSET = PLAN_UNSET, WRITER = PLAN_WRITER;
constexpr uint32_t WALK_TPB = 512;
// witnesses per workgroup of the walk; a power of two.  8 is the starting value (41 ops of the median SHA level x 8 = 328 of 512
// lanes), NOT yet a measured choice: profiles/device_witness.md says how 4 / 8 / 16 are to be compared
constexpr uint32_t WALK_GROUP = 8;

struct WalkArgs {
  const OpRec *ops;
  const uint32_t *level_off;  // [levels + 1]
  uint32_t levels;
  const uint32_t *cell_slot;  // [R][n]
  gl_t *val;                  // [slots][B]
  const uint2 *seed_cells;    // (row, col)
  const gl_t *seed_vals;      // [seeds][B]
  const uint8_t *row_gate;
  const GateDesc *gates;
  const gl_t *gconsts, *prc;
  unsigned long long *err;    // [B]: per witness, the smallest (op position << 8 | column) that contradicts
  uint32_t d, R, ngc, B;
};

// the row as the level walk sees it: witness b's slot values behind the routed cells
struct RowSlots {
  const WalkArgs &a;
  size_t row;
  uint32_t pos;  // of the op in the schedule
  uint32_t b;    // witness of the batch
  __device__ __forceinline__ gl_t &slot(uint32_t s) const { return a.val[(size_t)s * a.B + b]; }
  __device__ __forceinline__ gl_t get(uint32_t col) const {
    if (col >= a.R) return 0;
    const uint32_t s = a.cell_slot[((size_t)col << a.d) + row];
    return s == UNSET ? (gl_t)0 : slot(s & ~WRITER);
  }
  __device__ __forceinline__ void set(uint32_t col, gl_t v) {
    if (col >= a.R) return;  // gate-internal column: fill_witness derives it
    const uint32_t s = a.cell_slot[((size_t)col << a.d) + row];
    if (s == UNSET) return;
    if (s & WRITER) slot(s & ~WRITER) = v;
    else if (slot(s) != v) reject(col);
  }
  __device__ __forceinline__ gl_t lc(uint32_t i) const { return i < a.ngc ? a.gconsts[((size_t)i << a.d) + row] : (gl_t)0; }
  __device__ __forceinline__ void reject(uint32_t col) { atomicMin(a.err + b, ((unsigned long long)pos << 8) | col); }
};

__device__ __forceinline__ void run_op(const WalkArgs &a, uint32_t pos, uint32_t b) {
  const OpRec op = a.ops[pos];
  const uint32_t code = op.y & 0xFF, sub = op.y >> 8;
  if (code == OP_SEED) {
    const uint2 cell = a.seed_cells[op.x];
    const gl_t v = a.seed_vals[(size_t)op.x * a.B + b];
    RowSlots w{a, cell.x, pos, b};
    if (v >= GL_P) w.reject(cell.y);
    else w.set(cell.y, v);
    return;
  }
  RowSlots w{a, op.x, pos, b};
  const GateDesc g = a.gates[a.row_gate[op.x]];
  switch (code) {
  case OP_CONSTANT: gen_constant(w, g); break;
  case OP_ARITHMETIC: gen_arithmetic_op(w, sub, w.lc(0), w.lc(1)); break;
  case OP_BASE_SPLIT: gen_base_sum_split(w, g); break;
  case OP_BASE_JOIN: gen_base_sum_join(w, g); break;
  case OP_RA_COPY: gen_random_access_copy(w, g, sub); break;
  case OP_RA_CONSTS: gen_random_access_consts(w, g); break;
  case OP_POSEIDON: gen_poseidon(w, a.prc); break;
  case OP_U32_ARITHMETIC: gen_u32_arithmetic_op(w, g, sub); break;
  case OP_U32_ADD_MANY: gen_u32_add_many_op(w, g, sub); break;
  case OP_U32_SUBTRACTION: gen_u32_subtraction_op(w, g, sub); break;
  case OP_U32_RANGE_CHECK: gen_u32_range_check(w, g); break;
  case OP_COMPARISON: gen_comparison(w, g); break;
  default: break;
  }
}

// ONE workgroup per group of WALK_GROUP witnesses (the last group may hold fewer): the waves of a workgroup share their CU's
// vector cache, so what a level stored is what the next level loads after the barrier, and a group reads and writes its own
// witnesses' words only; the rest of the device stays free for the proofs in flight.  With 1 << sh the group's width rounded
// up to a power of two, lane t takes witness t & mask of the group and the level's ops t >> sh, + 512 >> sh, ... (the lone
// call: sh = 0, a lane per op).
__global__ __launch_bounds__(WALK_TPB) void genwit_walk_kernel(WalkArgs a) {
  const uint32_t b0 = blockIdx.x * WALK_GROUP, gw = min(WALK_GROUP, a.B - b0);
  const uint32_t sh = gw > 1 ? 32 - __clz(gw - 1) : 0, lb = threadIdx.x & ((1u << sh) - 1);
  const uint32_t first = threadIdx.x >> sh, step = WALK_TPB >> sh;
  for (uint32_t l = 0; l < a.levels; l++) {
    const uint32_t end = a.level_off[l + 1];
    if (lb < gw)
      for (uint32_t pos = a.level_off[l] + first; pos < end; pos += step) run_op(a, pos, b0 + lb);
    __syncthreads();
  }
}

// wires[b][col][row] = witness b's value of the slot, zero for a cell without one and for the gate-internal columns
// (cells <= i < matrix); cell_slot is read once for the whole batch.  A lane keeps its cell and loops over b: the stores of a
// wave are 64 consecutive words of one matrix, and a lane's loads are the B consecutive words of its slot (whole cache lines
// from B = 16 on) -- a lane per (cell, b) would coalesce the loads and scatter every store over B matrices instead.
__global__ __launch_bounds__(256) void genwit_scatter_kernel(const uint32_t *cell_slot, const gl_t *val, size_t cells, size_t matrix,
                                                             uint32_t B, gl_t *wires) {
  const size_t step = (size_t)gridDim.x * 256;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < matrix; i += step) {
    const uint32_t s = i < cells ? cell_slot[i] : UNSET;
    const gl_t *v = s == UNSET ? nullptr : val + (size_t)(s & ~WRITER) * B;
    for (uint32_t b = 0; b < B; b++) wires[b * matrix + i] = v ? v[b] : (gl_t)0;
  }
}

// the seeds no slot carries: pi_rows = 0: those on gate-internal columns; 1: those in PublicInputGate rows, whose wires are
// the caller's whatever ran in between.  A lane per (seed, witness), the witness the fast index as in vals.
__global__ void genwit_seed_write_kernel(const uint2 *cells, const gl_t *vals, uint32_t count, uint32_t B, uint32_t R, uint32_t d,
                                         int pi_rows, const uint8_t *row_gate, const GateDesc *gates, size_t matrix, gl_t *wires) {
  const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= (size_t)count * B) return;
  const uint2 c = cells[k / B];
  if (pi_rows ? gates[row_gate[c.x]].kind == G_PUBLIC_INPUT : c.y >= R) wires[(k % B) * matrix + ((size_t)c.y << d) + c.x] = vals[k];
}

// ---- plan compilation (host) ----
struct HostOp {
  uint32_t code, row, sub;
  uint32_t in0, in1, out0, out1;  // ranges in Compiler::cols
  uint32_t pending = 0, twin = UNSET;
  int level = -1;
  bool dead = false;
};

double wall_ms() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count(); }

}  // namespace

struct p2gpu_witness_plan {
  p2gpu_circuit *c = nullptr;
  uint32_t n_seeds = 0, levels = 0, slots = 0, widest = 0;
  size_t n_ops = 0;
  double compile_ms = 0, walk_ms = 0;
  std::vector<OpRec> h_ops;  // the schedule, to name the cell of a contradiction
  DBuf<OpRec> ops;
  DBuf<uint32_t> level_off, cell_slot;
  DBuf<gl_t> val, seed_vals;
  DBuf<uint2> seed_cells;
  std::vector<uint2> h_seed_cells;
  DBuf<unsigned long long> err;
  uint64_t *pin = nullptr;  // page-locked: [n_seeds] staging of the seed values, then the contradiction word
  // the same four for p2gpu_generate_witness_batch, sized for batch_cap witnesses by the first call that needs them
  struct Values {
    gl_t *val, *seed_vals;
    unsigned long long *err;
    uint64_t *pin;
  };
  size_t batch_cap = 0;
  DBuf<gl_t> bval, bseed_vals;
  DBuf<unsigned long long> berr;
  uint64_t *bpin = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  void release_batch() {
    bval.release(); bseed_vals.release(); berr.release();
    if (bpin) (void)hipHostFree(bpin);
    bpin = nullptr;
    batch_cap = 0;
  }
  void release() {
    ops.release(); level_off.release(); cell_slot.release(); val.release(); seed_vals.release(); seed_cells.release(); err.release();
    release_batch();
    if (pin) (void)hipHostFree(pin);
    if (ev0) (void)hipEventDestroy(ev0);
    if (ev1) (void)hipEventDestroy(ev1);
    pin = nullptr; ev0 = ev1 = nullptr;
  }
};

namespace {

struct Compiler {
  const p2gpu_circuit *c;
  size_t n;
  uint32_t R, d, ngc;
  std::vector<gl_t> sigma, gconsts;
  std::vector<uint8_t> row_gate;
  std::vector<uint32_t> cell_slot;  // [R][n]; classes first, then the lone cells
  std::vector<uint32_t> cols;       // input / output columns of the ops
  std::vector<HostOp> ops;
  uint32_t slots = 0;

  size_t key(uint32_t row, uint32_t col) const { return ((size_t)col << d) + row; }

  // sigma -> class ids of the cells on a cycle of length > 1
  int classes() {
    gl_t w = GL_ROOT_2_32;
    for (uint32_t i = d; i < 32; i++) w = gl_sqr(w);
    std::vector<gl_t> wp(n);
    std::unordered_map<gl_t, uint32_t> row_of, col_of;
    row_of.reserve(2 * n);
    gl_t x = 1;
    for (size_t r = 0; r < n; r++, x = gl_mul(x, w)) wp[r] = x, row_of[x] = (uint32_t)r;
    std::vector<gl_t> kinv(R);
    for (uint32_t col = 0; col < R; col++) {
      gl_t t = c->k_is[col];
      for (uint32_t i = 0; i < d; i++) t = gl_sqr(t);
      col_of[t] = col;
      kinv[col] = gl_inv(c->k_is[col]);
    }
    const size_t tot = (size_t)R * n;
    std::vector<uint32_t> parent(tot, UNSET);
    auto find = [&](uint32_t v) {
      uint32_t r = v;
      while (parent[r] != r) r = parent[r];
      while (parent[v] != r) { const uint32_t nx = parent[v]; parent[v] = r; v = nx; }
      return r;
    };
    for (uint32_t col = 0; col < R; col++)
      for (size_t row = 0; row < n; row++) {
        const gl_t s = sigma[key(row, col)];
        if (s == gl_mul(c->k_is[col], wp[row])) continue;
        gl_t t = s;
        for (uint32_t i = 0; i < d; i++) t = gl_sqr(t);
        const auto ci = col_of.find(t);
        const auto ri = ci == col_of.end() ? row_of.end() : row_of.find(gl_mul(s, kinv[ci->second]));
        if (s >= GL_P || ri == row_of.end()) {
          set_err("p2gpu_witness_plan_create: sigma of cell (row %zu, column %u) names no routed cell", row, col);
          return P2GPU_E_ARG;
        }
        const uint32_t a = (uint32_t)key(row, col), b = (uint32_t)key(ri->second, ci->second);
        if (parent[a] == UNSET) parent[a] = a;
        if (parent[b] == UNSET) parent[b] = b;
        const uint32_t ra = find(a), rb = find(b);
        if (ra != rb) parent[std::max(ra, rb)] = std::min(ra, rb);
      }
    cell_slot.assign(tot, UNSET);
    for (size_t v = 0; v < tot; v++)
      if (parent[v] != UNSET) {
        const uint32_t r = find((uint32_t)v);
        if (cell_slot[r] == UNSET) cell_slot[r] = slots++;  // (r <= v: the root is numbered first)
        cell_slot[v] = cell_slot[r];
      }
    return P2GPU_OK;
  }

  // an op of the row (genops.hpp lists its input columns and the columns its generator sets; routed ones only count); kept when
  // one of its cells has a slot, and then every output cell gets one
  uint32_t add_op(uint32_t row, const OpCols &oc) {
    bool active = false;
    auto has_slot = [&](uint32_t col) { active |= col < R && cell_slot[key(row, col)] != UNSET; };
    for_cols(oc.in, has_slot);
    for_cols(oc.out, has_slot);
    if (!active) return UNSET;
    HostOp op;
    op.code = oc.code; op.row = row; op.sub = oc.sub;
    op.in0 = (uint32_t)cols.size();
    for_cols(oc.in, [&](uint32_t col) { if (col < R && cell_slot[key(row, col)] != UNSET) cols.push_back(col); });  // a cell without a slot reads as zero
    op.in1 = op.out0 = (uint32_t)cols.size();
    for_cols(oc.out, [&](uint32_t col) {
      if (col >= R) return;
      uint32_t &s = cell_slot[key(row, col)];
      if (s == UNSET) s = slots++;
      cols.push_back(col);
    });
    op.out1 = (uint32_t)cols.size();
    ops.push_back(op);
    return (uint32_t)ops.size() - 1;
  }

  void row_ops(uint32_t row) {
    const GateDesc &g = c->gates[row_gate[row]];
    auto LC = [&](uint32_t i) { return i < ngc ? gconsts[(size_t)i * n + row] : (gl_t)0; };
    const gl_t c0 = LC(0), c1 = LC(1);
    if (g.kind == G_BASE_SUM) {
      // every cell is an input of one direction and an output of the other: all of them get their slot before either op
      // lists its inputs
      bool active = false;
      for (uint32_t col = 0; col <= g.p[1] && col < R; col++) active |= cell_slot[key(row, col)] != UNSET;
      if (!active) return;
      for (uint32_t col = 0; col <= g.p[1] && col < R; col++)
        if (cell_slot[key(row, col)] == UNSET) cell_slot[key(row, col)] = slots++;
      const uint32_t a = add_op(row, row_op(g, 0, c0, c1)), b = add_op(row, row_op(g, 1, c0, c1));
      if (a != UNSET) ops[a].twin = b, ops[b].twin = a;  // (both see the same cells: kept or dropped together)
      return;
    }
    for (uint32_t k = 0, m = row_num_ops(g); k < m; k++) add_op(row, row_op(g, k, c0, c1));
  }
  // seeds first, then the rows in order; levels; what the schedule did not reach.  order: the ops by (level, creation order)
  int schedule(const std::vector<uint2> &seeds, std::vector<uint32_t> &order, std::vector<uint32_t> &level_off) {
    const size_t tot = (size_t)R * n;
    // ---- ops: seeds first, then the rows in order ----
    for (size_t i = 0; i < seeds.size(); i++) {
      const uint2 cell = seeds[i];
      HostOp op;
      op.code = OP_SEED; op.row = (uint32_t)i; op.sub = 0;
      op.in0 = op.in1 = op.out0 = (uint32_t)cols.size();
      if (cell.y < R) {
        uint32_t &s = cell_slot[key(cell.x, cell.y)];
        if (s == UNSET) s = slots++;
        cols.push_back(cell.y);
      }
      op.out1 = (uint32_t)cols.size();
      ops.push_back(op);
    }
    for (size_t row = 0; row < n; row++) row_ops((uint32_t)row);
    if (slots >= WRITER || ops.size() >= ((size_t)1 << 32)) { set_err("p2gpu_witness_plan_create: circuit too large"); return P2GPU_E_ARG; }
    // ---- levels ----
    auto op_row = [&](const HostOp &o) { return o.code == OP_SEED ? seeds[o.row].x : o.row; };
    auto slot_of = [&](const HostOp &o, uint32_t k) -> uint32_t & { return cell_slot[key(op_row(o), cols[k])]; };
    std::vector<uint32_t> use_off(slots + 1, 0);
    for (auto &o : ops) {
      o.pending = o.in1 - o.in0;
      for (uint32_t k = o.in0; k < o.in1; k++) use_off[slot_of(o, k) + 1]++;
    }
    for (uint32_t s = 0; s < slots; s++) use_off[s + 1] += use_off[s];
    std::vector<uint32_t> users(use_off[slots]), fillp(use_off.begin(), use_off.end() - 1);
    for (uint32_t i = 0; i < ops.size(); i++)
      for (uint32_t k = ops[i].in0; k < ops[i].in1; k++) users[fillp[slot_of(ops[i], k)]++] = i;
    std::vector<int> slot_level(slots, -1);
    std::vector<uint32_t> cur, next, fresh;
    order.clear();
    level_off.assign(1, 0);
    for (uint32_t i = 0; i < ops.size(); i++) if (!ops[i].pending) cur.push_back(i);
    for (int lvl = 0; !cur.empty(); lvl++) {
      next.clear(); fresh.clear();
      for (uint32_t i : cur) {
        HostOp &o = ops[i];
        if (o.dead) continue;
        bool wait = false;  // an earlier op of this level writes one of the outputs: compare one level later
        for (uint32_t k = o.out0; k < o.out1; k++) wait |= slot_level[slot_of(o, k) & ~WRITER] == lvl;
        if (wait) { next.push_back(i); continue; }
        o.level = lvl;
        if (o.twin != UNSET) ops[o.twin].dead = true;
        for (uint32_t k = o.out0; k < o.out1; k++) {
          uint32_t &s = slot_of(o, k);
          if (slot_level[s & ~WRITER] < 0) { slot_level[s & ~WRITER] = lvl; fresh.push_back(s & ~WRITER); s |= WRITER; }
        }
        order.push_back(i);
      }
      level_off.push_back((uint32_t)order.size());
      for (uint32_t s : fresh)
        for (uint32_t u = use_off[s]; u < use_off[s + 1]; u++) if (--ops[users[u]].pending == 0) next.push_back(users[u]);
      std::sort(next.begin(), next.end());
      cur.swap(next);
    }
    // ---- what the schedule did not reach ----
    {
      // producers of every slot: 1 = some op, 2 = only the limbs -> sum direction of BaseSum rows (whose limbs wait for the sum)
      std::vector<uint8_t> producer(slots, 0);
      for (auto &o : ops)
        for (uint32_t k = o.out0; k < o.out1; k++) {
          uint8_t &f = producer[slot_of(o, k) & ~WRITER];
          f = o.code == OP_BASE_JOIN ? (f ? f : 2) : 1;
        }
      size_t stuck = SIZE_MAX, join_only = SIZE_MAX, cyc = SIZE_MAX;
      for (size_t v = 0; v < tot && stuck == SIZE_MAX; v++) {
        const uint32_t s = cell_slot[v];
        if (s == UNSET || slot_level[s & ~WRITER] >= 0) continue;
        const uint8_t f = producer[s & ~WRITER];
        if (!f) stuck = v;
        else if (f == 2 && join_only == SIZE_MAX) join_only = v;
        else if (cyc == SIZE_MAX) cyc = v;
      }
      if (stuck == SIZE_MAX) stuck = join_only;
      if (stuck != SIZE_MAX) {
        set_err("no seed, constant or generator reaches the copy class of cell (row %zu, column %zu): a seed is missing", stuck & (n - 1), stuck >> d);
        return P2GPU_E_ARG;
      }
      if (cyc != SIZE_MAX) {
        set_err("dependency cycle: the generator that derives cell (row %zu, column %zu) waits for its own output", cyc & (n - 1), cyc >> d);
        return P2GPU_E_ARG;
      }
    }
    return P2GPU_OK;
  }
};


// the seed checks of both compilers: every seed inside the matrix, no cell twice
int plan_seeds(p2gpu_witness_plan *p, const uint32_t *seed_cells, size_t n_seeds) {
  const p2gpu_circuit *c = p->c;
  const size_t n = c->n;
  std::unordered_map<uint64_t, size_t> seen;
  for (size_t i = 0; i < n_seeds; i++) {
    const uint32_t row = seed_cells[2 * i], col = seed_cells[2 * i + 1];
    if (row >= n || col >= c->W) {
      set_err("seed %zu names cell (row %u, column %u) outside the %zu x %u wire matrix", i, row, col, n, c->W);
      return P2GPU_E_ARG;
    }
    if (!seen.emplace(((uint64_t)row << 32) | col, i).second) {
      set_err("cell (row %u, column %u) is seeded twice (seeds %zu and %zu)", row, col, seen[((uint64_t)row << 32) | col], i);
      return P2GPU_E_ARG;
    }
    p->h_seed_cells.push_back(make_uint2(row, col));
  }
  return P2GPU_OK;
}

// The tail of both compilers: the plan's own buffers, filled from the three arrays (an upload for the host compiler, a copy
// inside HBM and ONE read-back -- the op records name_contradiction needs -- for the device one).
int plan_finish(p2gpu_witness_plan *p, const PlanArrays &a) {
  p2gpu_circuit *c = p->c;
  const size_t n_seeds = p->n_seeds, tot = (size_t)c->R * c->n;
  p->levels = a.levels; p->slots = a.slots; p->n_ops = a.n_ops; p->widest = a.widest;
  HIP_TRY(p->ops.alloc(std::max<size_t>(1, a.n_ops)));
  HIP_TRY(p->level_off.alloc((size_t)a.levels + 1));
  HIP_TRY(p->cell_slot.alloc(tot));
  HIP_TRY(p->val.alloc(std::max<uint32_t>(1, a.slots)));
  HIP_TRY(p->seed_vals.alloc(std::max<size_t>(1, n_seeds)));
  HIP_TRY(p->seed_cells.alloc(std::max<size_t>(1, n_seeds)));
  HIP_TRY(p->err.alloc(1));
  HIP_TRY(hipHostMalloc((void **)&p->pin, 8 * (n_seeds + 1), hipHostMallocDefault));
  HIP_TRY(hipEventCreate(&p->ev0));
  HIP_TRY(hipEventCreate(&p->ev1));
  p->h_ops.resize(a.n_ops);
  if (a.n_ops) {
    HIP_TRY(hipMemcpyAsync(p->ops.p, a.ops, sizeof(OpRec) * a.n_ops, a.kind, c->stream));
    if (a.kind == hipMemcpyHostToDevice) memcpy(p->h_ops.data(), a.ops, sizeof(OpRec) * a.n_ops);
    else HIP_TRY(hipMemcpyAsync(p->h_ops.data(), a.ops, sizeof(OpRec) * a.n_ops, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(hipMemcpyAsync(p->level_off.p, a.level_off, 4 * ((size_t)a.levels + 1), a.kind, c->stream));
  HIP_TRY(hipMemcpyAsync(p->cell_slot.p, a.cell_slot, 4 * tot, a.kind, c->stream));
  if (n_seeds) HIP_TRY(hipMemcpyAsync(p->seed_cells.p, p->h_seed_cells.data(), sizeof(uint2) * n_seeds, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemsetAsync(p->val.p, 0, 8 * (size_t)std::max<uint32_t>(1, a.slots), c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));  // (the arrays go out of scope)
  return P2GPU_OK;
}

int plan_compile(p2gpu_witness_plan *p, const uint32_t *seed_cells, size_t n_seeds) {
  p2gpu_circuit *c = p->c;
  Compiler K;
  K.c = c; K.n = c->n; K.R = c->R; K.d = c->d; K.ngc = c->NC - c->num_selectors;
  const size_t n = c->n, tot = (size_t)c->R * n;
  if (int rc = plan_seeds(p, seed_cells, n_seeds)) return rc;
  // ---- the circuit's tables, as the device holds them ----
  K.sigma.resize(tot); K.gconsts.resize((size_t)K.ngc * n); K.row_gate.resize(n);
  HIP_TRY(hipMemcpyAsync(K.sigma.data(), c->d_sigmas.p, 8 * tot, hipMemcpyDeviceToHost, c->stream));
  if (K.ngc) HIP_TRY(hipMemcpyAsync(K.gconsts.data(), c->d_gconsts.p, 8 * K.gconsts.size(), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(K.row_gate.data(), c->d_row_gate.p, n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  if (int rc = K.classes()) return rc;
  std::vector<uint32_t> order, level_off;
  if (int rc = K.schedule(p->h_seed_cells, order, level_off)) return rc;
  std::vector<OpRec> recs;
  recs.reserve(order.size());
  for (uint32_t i : order) recs.push_back(make_uint2(K.ops[i].row, K.ops[i].code | (K.ops[i].sub << 8)));
  PlanArrays a;
  a.cell_slot = K.cell_slot.data(); a.ops = recs.data(); a.level_off = level_off.data();
  a.levels = (uint32_t)level_off.size() - 1; a.slots = K.slots; a.n_ops = order.size();
  for (uint32_t l = 0; l < a.levels; l++) a.widest = std::max(a.widest, level_off[l + 1] - level_off[l]);
  return plan_finish(p, a);
}

// the device compiler (genplan.hip) behind the same seed checks and the same tail
int plan_build(p2gpu_witness_plan *p, const uint32_t *seed_cells, size_t n_seeds) {
  if (int rc = plan_seeds(p, seed_cells, n_seeds)) return rc;
  classes::Scratch S;
  PlanArrays a;
  if (int rc = plan_compile_device(p->c, p->h_seed_cells, S, a)) return rc;
  return plan_finish(p, a);  // (S goes out of scope behind it: the plan holds what a host-compiled one holds)
}

// the batched buffers, grown to hold `batch` witnesses (the stream is idle between calls: one call at a time per handle).
// batch_cap is a capacity in witnesses: a call lays its values out with its own B as the stride, in the front of the buffers.
// Nothing is cleared: every slot has a writer (plan_compile refuses a plan with an unreached one) and is written before it is read.
int reserve_batch(p2gpu_witness_plan *p, size_t batch) {
  if (batch <= p->batch_cap) return P2GPU_OK;
  p->release_batch();
  HIP_TRY(p->bval.alloc(batch * std::max<uint32_t>(1, p->slots)));
  HIP_TRY(p->bseed_vals.alloc(batch * std::max<uint32_t>(1, p->n_seeds)));
  HIP_TRY(p->berr.alloc(batch));
  HIP_TRY(hipHostMalloc((void **)&p->bpin, 8 * batch * ((size_t)p->n_seeds + 1), hipHostMallocDefault));
  p->batch_cap = batch;
  return P2GPU_OK;
}

// everything of B witnesses on the handle's stream: v.pin holds the seed values [n_seeds][B] on entry and, from
// v.pin + n_seeds * B on, the B contradiction words when this returns.  wires: [B][num_wires][n]
int walk_and_scatter(p2gpu_witness_plan *p, const p2gpu_witness_plan::Values &v, uint32_t B, gl_t *wires) {
  p2gpu_circuit *c = p->c;
  hipStream_t st = c->stream;
  const uint32_t ngc = c->NC - c->num_selectors;
  const size_t n_vals = (size_t)p->n_seeds * B;
  if (n_vals) HIP_TRY(hipMemcpyAsync(v.seed_vals, v.pin, 8 * n_vals, hipMemcpyHostToDevice, st));
  HIP_TRY(hipMemsetAsync(v.err, 0xFF, 8 * (size_t)B, st));
  WalkArgs a;
  a.ops = p->ops.p; a.level_off = p->level_off.p; a.levels = p->levels; a.cell_slot = p->cell_slot.p; a.val = v.val;
  a.seed_cells = p->seed_cells.p; a.seed_vals = v.seed_vals; a.row_gate = c->d_row_gate.p; a.gates = c->d_gates.p;
  a.gconsts = c->d_gconsts.p; a.prc = c->d_prc.p; a.err = v.err; a.d = c->d; a.R = c->R; a.ngc = ngc; a.B = B;
  HIP_TRY(hipEventRecord(p->ev0, st));
  {
    ProfScope ps("genwit_walk_kernel", 16.0 * (double)p->n_ops * B);
    hipLaunchKernelGGL(genwit_walk_kernel, dim3((B + WALK_GROUP - 1) / WALK_GROUP), dim3(WALK_TPB), 0, st, a);
  }
  HIP_TRY(hipEventRecord(p->ev1, st));
  const size_t cells = (size_t)c->R * c->n, matrix = (size_t)c->W * c->n;
  {
    ProfScope ps("genwit_scatter_kernel", 4.0 * (double)cells + 8.0 * (double)(cells + matrix) * B);
    hipLaunchKernelGGL(genwit_scatter_kernel, dim3((unsigned)std::min<size_t>((matrix + 255) / 256, 1 << 16)), dim3(256), 0, st,
                       p->cell_slot.p, v.val, cells, matrix, B, wires);
  }
  const dim3 sg((unsigned)((n_vals + 255) / 256));
  if (n_vals)
    hipLaunchKernelGGL(genwit_seed_write_kernel, sg, dim3(256), 0, st, p->seed_cells.p, v.seed_vals, p->n_seeds, B, c->R, c->d, 0,
                       c->d_row_gate.p, c->d_gates.p, matrix, wires);
  for (uint32_t b = 0; b < B; b++)
    fill_witness(st, wires + b * matrix, c->d_row_gate.p, c->d_gates.p, c->d_gconsts.p, c->d_prc.p, c->d, ngc, c->W);
  if (n_vals)
    hipLaunchKernelGGL(genwit_seed_write_kernel, sg, dim3(256), 0, st, p->seed_cells.p, v.seed_vals, p->n_seeds, B, c->R, c->d, 1,
                       c->d_row_gate.p, c->d_gates.p, matrix, wires);
  HIP_TRY(hipMemcpyAsync(v.pin + n_vals, v.err, 8 * (size_t)B, hipMemcpyDeviceToHost, st));
  HIP_TRY(hipStreamSynchronize(st));
  HIP_TRY(hipGetLastError());
  float ms = 0;
  if (hipEventElapsedTime(&ms, p->ev0, p->ev1) == hipSuccess) p->walk_ms = ms;
  return P2GPU_OK;
}

// a contradiction word as (row, col) and as p2gpu_last_error's text behind `who`; seed_values: that witness's, [n_seeds]
int name_contradiction(const p2gpu_witness_plan *p, uint64_t e, const uint64_t *seed_values, const char *who, uint32_t cell[2]) {
  const size_t pos = (size_t)(e >> 8);
  const uint32_t col = (uint32_t)(e & 0xFF);
  if (pos >= p->h_ops.size()) { set_err("p2gpu_generate_witness: internal error (contradiction word)"); return P2GPU_E_DEVICE; }
  const OpRec op = p->h_ops[pos];
  const bool seed = (op.y & 0xFF) == OP_SEED;
  cell[0] = seed ? p->h_seed_cells[op.x].x : op.x;
  cell[1] = col;
  if (seed)
    set_err("%sseed %u for cell (row %u, column %u) %s", who, op.x, cell[0], col,
            seed_values[op.x] >= GL_P ? "is not a canonical field element" : "contradicts the value its copy class already has");
  else
    set_err("%sunsatisfiable: the generator of row %u contradicts the value cell (row %u, column %u) already has", who, op.x, op.x, col);
  return P2GPU_E_UNSATISFIED;
}

// one witness: the batch of one on the plan's own buffers; returns after the contradiction word has arrived
int generate(p2gpu_witness_plan *p, const uint64_t *seed_values, gl_t *wires) {
  HIP_TRY(hipSetDevice(p->c->device));
  if (p->n_seeds) memcpy(p->pin, seed_values, 8 * (size_t)p->n_seeds);
  if (int rc = walk_and_scatter(p, {p->val.p, p->seed_vals.p, p->err.p, p->pin}, 1, wires)) return rc;
  const uint64_t e = p->pin[p->n_seeds];
  uint32_t cell[2];
  return e == UINT64_MAX ? P2GPU_OK : name_contradiction(p, e, seed_values, "", cell);
}

// seed_values: [batch][n_seeds]; status: [batch]; bad_cells: [batch][2] or null
int generate_batch(p2gpu_witness_plan *p, const uint64_t *seed_values, size_t batch, gl_t *wires, int *status, uint32_t *bad_cells) {
  HIP_TRY(hipSetDevice(p->c->device));
  if (int rc = reserve_batch(p, batch)) return rc;
  const uint32_t B = (uint32_t)batch, S = p->n_seeds;
  for (uint32_t b = 0; b < B; b++)
    for (uint32_t i = 0; i < S; i++) p->bpin[(size_t)i * B + b] = seed_values[(size_t)b * S + i];
  if (int rc = walk_and_scatter(p, {p->bval.p, p->bseed_vals.p, p->berr.p, p->bpin}, B, wires)) return rc;
  int rc = P2GPU_OK;
  for (uint32_t b = B; b-- > 0;) {  // downwards: p2gpu_last_error keeps the lowest failing witness
    const uint64_t e = p->bpin[(size_t)S * B + b];
    uint32_t cell[2] = {UINT32_MAX, UINT32_MAX};
    status[b] = P2GPU_OK;
    if (e != UINT64_MAX) {
      char who[48];
      snprintf(who, sizeof who, "witness %u of the batch: ", b);
      status[b] = name_contradiction(p, e, seed_values + (size_t)b * S, who, cell);
      if (status[b] != P2GPU_E_UNSATISFIED || rc == P2GPU_OK) rc = status[b];  // (an internal error, once seen, is what returns)
    }
    if (bad_cells) bad_cells[2 * b] = cell[0], bad_cells[2 * b + 1] = cell[1];
  }
  return rc;
}

// the front checks and the ownership of a half-made plan, for either compiler
int plan_new(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, p2gpu_witness_plan **out,
             int (*compile)(p2gpu_witness_plan *, const uint32_t *, size_t)) {
  if (out) *out = nullptr;
  if (!c || !out || (n_seeds && !seed_cells)) return P2GPU_E_ARG;
  if (int rc = prover_handle(c)) return rc;
  if (!c->group.empty()) {
    set_err("p2gpu_witness_plan_create: a device group takes a wire matrix (every rank of a sharded proof reads all of it)");
    return P2GPU_E_ARG;
  }
  if (c->R > 256 || n_seeds >= ((size_t)1 << 32)) return P2GPU_E_ARG;  // (the contradiction word keeps the column in 8 bits)
  HIP_TRY(hipSetDevice(c->device));
  const double t0 = wall_ms();
  p2gpu_witness_plan *p = new p2gpu_witness_plan();
  p->c = c;
  p->n_seeds = (uint32_t)n_seeds;
  int rc;
  try {
    rc = compile(p, seed_cells, n_seeds);
  } catch (...) {
    p->release();
    delete p;
    throw;
  }
  if (rc) {
    p->release();
    delete p;
    return rc;
  }
  p->compile_ms = wall_ms() - t0;
  *out = p;
  return P2GPU_OK;
}

}  // namespace

extern "C" {

int p2gpu_witness_plan_create(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, p2gpu_witness_plan **out) try {
  return plan_new(c, seed_cells, n_seeds, out, plan_compile);
} P2GPU_CATCH

int p2gpu_witness_plan_build(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, p2gpu_witness_plan **out) try {
  return plan_new(c, seed_cells, n_seeds, out, plan_build);
} P2GPU_CATCH

int p2gpu_witness_plan_export(const p2gpu_witness_plan *p, uint32_t *cell_slot, uint64_t *ops, uint32_t *level_off, size_t sizes[3]) try {
  if (!p || !sizes) return P2GPU_E_ARG;
  const p2gpu_circuit *c = p->c;
  const size_t tot = (size_t)c->R * c->n;
  sizes[0] = tot; sizes[1] = p->n_ops; sizes[2] = (size_t)p->levels + 1;
  if (!cell_slot && !ops && !level_off) return P2GPU_OK;
  if (!cell_slot || !ops || !level_off) return P2GPU_E_ARG;
  static_assert(sizeof(OpRec) == sizeof(uint64_t), "an op record is one 64-bit word: row | (code | sub << 8) << 32");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipMemcpyAsync(cell_slot, p->cell_slot.p, 4 * tot, hipMemcpyDeviceToHost, c->stream));
  if (p->n_ops) HIP_TRY(hipMemcpyAsync(ops, p->ops.p, sizeof(OpRec) * p->n_ops, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipMemcpyAsync(level_off, p->level_off.p, 4 * sizes[2], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return P2GPU_OK;
} P2GPU_CATCH

void p2gpu_witness_plan_destroy(p2gpu_witness_plan *p) {
  if (!p) return;
  (void)hipSetDevice(p->c->device);
  (void)hipStreamSynchronize(p->c->stream);
  p->release();
  delete p;
}

int p2gpu_witness_plan_info(const p2gpu_witness_plan *p, uint64_t counts[5], double ms[2]) {
  if (!p || !counts || !ms) return P2GPU_E_ARG;
  counts[0] = p->n_ops; counts[1] = p->levels; counts[2] = p->widest; counts[3] = p->slots; counts[4] = p->n_seeds;
  ms[0] = p->compile_ms; ms[1] = p->walk_ms;
  return P2GPU_OK;
}

int p2gpu_generate_witness(p2gpu_witness_plan *p, const uint64_t *seed_values, uint64_t *wires_dev_out) try {
  if (!p || !wires_dev_out || (p->n_seeds && !seed_values)) return P2GPU_E_ARG;
  ProfGuard pg(p->c);
  return generate(p, seed_values, wires_dev_out);
} P2GPU_CATCH

int p2gpu_generate_witness_batch(p2gpu_witness_plan *p, const uint64_t *seed_values, size_t batch, uint64_t *wires_dev_out, int *status,
                                 uint32_t *bad_cells) try {
  if (!p || !wires_dev_out || !status || batch == 0 || (p->n_seeds && !seed_values)) return P2GPU_E_ARG;
  if (batch >= ((size_t)1 << 32) / std::max<uint32_t>(1, p->n_seeds)) return P2GPU_E_ARG;  // (the seed-write kernel's grid)
  ProfGuard pg(p->c);
  return generate_batch(p, seed_values, batch, wires_dev_out, status, bad_cells);
} P2GPU_CATCH

int p2gpu_prove_seeds(p2gpu_witness_plan *p, const uint64_t *seed_values, const uint64_t *pis, uint32_t n_pi, uint8_t *proof_out,
                      size_t *proof_len, p2gpu_timings *tm) try {
  if (!p || !proof_out || !proof_len || (p->n_seeds && !seed_values)) return P2GPU_E_ARG;
  p2gpu_circuit *c = p->c;
  const double t0 = now_ms();
  {
    ProfGuard pg(c);
    if (int rc = generate(p, seed_values, c->wires_vals.p)) return rc;
  }
  // (h2d_ms: what stands in front of the resident proof -- here the witness generation)
  return prove_impl(c, c->wires_vals.p, pis, n_pi, proof_out, proof_len, tm, now_ms() - t0);
} P2GPU_CATCH

}  // extern "C"
