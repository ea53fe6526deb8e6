// genplan.hip -- the witness plan compiled on the device (p2gpu_witness_plan_build): the same cell_slot words, op records and
// level offsets as the host compiler of planhost.hpp (Compiler::classes / add_op / row_ops / schedule), which stays as the
// differential oracle (tests/test_gpu_witness_plan.py compares the exported arrays byte for byte).
//
// Cells are numbered as sigma is laid out, key = col << d | row.  Every phase restates the host rule it replaces:
//   1. decode    sigma[x] = k_is[col'] * w^row' for every routed cell that is no fixed point: sigma^n against the R values
//                k_is[c]^n names col', a binary search of sigma / k_is[col'] in the sorted powers of w names row'.  The smallest
//                key whose value is >= p or names no routed cell is refused (atomicMin), as the host's first one in its loop.
//   2. classes   devclasses.hpp's touch / hook / jump over the pairs (x, partner[x]): parent[x] = the smallest key of the class.
//                The host numbers a class when it meets its root, the smallest key: slot = rank of the root among roots.
//   3. slots/ops seeds first (a routed seed cell without a slot takes the next one, in seed order), then the generators that are
//                no gate's own (a cell one of them names, without a slot, takes the next one at its FIRST naming, by generator
//                and cell position: an atomicMin of the naming's index per cell, flags, a scan), then the rows top to
//                bottom, ops left to right.  The ops of a row touch only that row's cells and no two ops of a row share a cell
//                (the BaseSum twins aside, whose cells all get their slots first), so one lane per row runs genops.hpp's
//                enumerator twice: count (ops kept, new slots), exclusive scans over the rows, fill.  For the same reason the
//                cells an op lists as inputs -- those with a slot when the op is created -- are those with a slot in the end.
//   4. levels    one persistent workgroup; see plan_schedule_kernel.
//   5. unreached one pass over the routed cells, three atomicMin words, the host's priority.
// The phases are PlanCtx's decode .. unreached below.  Scratch (DESIGN 6b states the bound) lives in the
// caller's classes::Scratch and is gone when the plan is attached.
#include "devclasses.hpp"
#include "genplan.hpp"

using namespace p2;

namespace {

using classes::TPB;
using classes::grid_for;
using classes::subgroup_power;
constexpr uint32_t UNSET = PLAN_UNSET, WRITER = PLAN_WRITER;
constexpr uint32_t SCHED_TPB = 512;
constexpr int32_t LEVEL_DEAD = -2;  // level[] of an op whose twin ran (-1: not scheduled, or not yet)
// counters on the device, read back in one copy
enum { C_BAD_SIGMA = 0, C_TOUCHED, C_CLASSES, C_SEED_SLOTS, C_GEN_SLOTS, C_SLOTS, C_ROW_OPS, C_READY, C_NO_PRODUCER, C_JOIN_ONLY, C_OTHER, C_COUNT };
// plan_schedule_kernel's result words
enum { S_LEVELS = 0, S_WIDEST, S_ERROR, S_DONE, S_COUNT };

// words other lanes of the persistent workgroup change between two barriers: read and written past the vector cache
template <class T> __device__ __forceinline__ T ld_shared(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <class T> __device__ __forceinline__ void st_shared(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// ---- 1. decode ----
__global__ void plan_powers_kernel(const gl_t *tw, uint32_t d, gl_t *keys, uint32_t *rows) {
  const size_t n = (size_t)1 << d, step = (size_t)gridDim.x * TPB;
  for (size_t r = (size_t)blockIdx.x * TPB + threadIdx.x; r < n; r += step) {
    keys[r] = subgroup_power(tw, d, (uint32_t)r);
    rows[r] = (uint32_t)r;
  }
}

// partner[x] = the key sigma[x] names, UNSET for a fixed point (and for a refused value: nothing is indexed with it)
__global__ void plan_decode_kernel(const gl_t *sigma, const gl_t *kis, const gl_t *kpow /* [R] k^n, then [R] 1/k */, const gl_t *tw,
                                   const gl_t *wsorted, const uint32_t *wrow, uint32_t d, uint32_t R, uint32_t *partner,
                                   unsigned long long *bad) {
  const size_t n = (size_t)1 << d, tot = (size_t)R << d, step = (size_t)gridDim.x * TPB;
  for (size_t x = (size_t)blockIdx.x * TPB + threadIdx.x; x < tot; x += step) {
    const uint32_t col = (uint32_t)(x >> d), row = (uint32_t)(x & (n - 1));
    const gl_t s = sigma[x];
    uint32_t y = UNSET;
    if (s != gl_mul(kis[col], subgroup_power(tw, d, row))) {
      bool ok = s < GL_P;
      uint32_t c2 = UNSET;
      if (ok) {
        gl_t t = s;
        for (uint32_t i = 0; i < d; i++) t = gl_sqr(t);
        for (uint32_t k = 0; k < R; k++)
          if (kpow[k] == t) c2 = k;  // (the cosets are distinct: one match at most)
        ok = c2 != UNSET;
      }
      if (ok) {
        const gl_t u = gl_mul(s, kpow[R + c2]);
        size_t lo = 0, hi = n;  // the first entry >= u
        while (lo < hi) {
          const size_t mid = (lo + hi) >> 1;
          if (wsorted[mid] < u) lo = mid + 1;
          else hi = mid;
        }
        ok = lo < n && wsorted[lo] == u;
        if (ok) y = (c2 << d) | wrow[lo];
      }
      if (!ok) atomicMin(bad, (unsigned long long)x);
    }
    partner[x] = y;
  }
}

// the decoded pairs as devclasses.hpp's pair source: entry x is (x, partner[x])
struct SigmaPairs {
  const uint32_t *partner;
  __device__ __forceinline__ bool get(size_t i, uint32_t &a, uint32_t &b) const {
    b = partner[i];
    a = (uint32_t)i;
    return b != UNSET;
  }
};

// ---- 2. classes -> slots ----
__global__ void plan_root_flags_kernel(const uint32_t *parent, size_t tot, uint32_t *flag) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t v = (size_t)blockIdx.x * TPB + threadIdx.x; v < tot; v += step) flag[v] = parent[v] == (uint32_t)v ? 1u : 0u;
}
__global__ void plan_class_slots_kernel(const uint32_t *parent, const uint32_t *rank, size_t tot, uint32_t *cell_slot) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t v = (size_t)blockIdx.x * TPB + threadIdx.x; v < tot; v += step) {
    const uint32_t r = parent[v];
    cell_slot[v] = r == UNSET ? UNSET : rank[r];
  }
}
// *out = (base ? *base : 0) + the sum of count[0 .. m) given its exclusive scan
__global__ void plan_total_kernel(const unsigned long long *base, const uint32_t *count, const uint32_t *scan, size_t m, unsigned long long *out) {
  *out = (base ? *base : 0ull) + (m ? (unsigned long long)scan[m - 1] + count[m - 1] : 0ull);
}

// ---- 3. slots and ops ----
__global__ void plan_seed_flags_kernel(const uint2 *seeds, uint32_t S, uint32_t d, uint32_t R, const uint32_t *cell_slot, uint32_t *flag) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S) return;
  const uint2 c = seeds[i];
  flag[i] = c.y < R && cell_slot[((size_t)c.y << d) + c.x] == UNSET ? 1u : 0u;
}
__global__ void plan_seed_slots_kernel(const uint2 *seeds, uint32_t S, uint32_t d, const uint32_t *flag, const uint32_t *scan,
                                       const unsigned long long *base, uint32_t *cell_slot) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i >= S || !flag[i]) return;
  const uint2 c = seeds[i];
  cell_slot[((size_t)c.y << d) + c.x] = (uint32_t)*base + scan[i];
}

// the generators that are no gate's own: entry e = the generator's offset + cell position names cell gkeys[e] (the flat list of
// the checked generators, PlanGenList).  first[key] = the smallest
// entry that names a cell without a slot (cleared for exactly the named cells: nothing else of `first` is read)
__global__ void plan_gen_clear_kernel(const uint32_t *gkeys, uint32_t NE, uint32_t *first) {
  const uint32_t e = blockIdx.x * TPB + threadIdx.x;
  if (e < NE) first[gkeys[e]] = UNSET;
}
__global__ void plan_gen_first_kernel(const uint32_t *gkeys, uint32_t NE, const uint32_t *cell_slot, uint32_t *first) {
  const uint32_t e = blockIdx.x * TPB + threadIdx.x;
  if (e < NE && cell_slot[gkeys[e]] == UNSET) atomicMin(&first[gkeys[e]], e);
}
__global__ void plan_gen_flags_kernel(const uint32_t *gkeys, uint32_t NE, const uint32_t *cell_slot, const uint32_t *first, uint32_t *flag) {
  const uint32_t e = blockIdx.x * TPB + threadIdx.x;
  if (e < NE) flag[e] = cell_slot[gkeys[e]] == UNSET && first[gkeys[e]] == e ? 1u : 0u;
}
__global__ void plan_gen_slots_kernel(const uint32_t *gkeys, uint32_t NE, const uint32_t *flag, const uint32_t *scan,
                                      const unsigned long long *base, uint32_t *cell_slot) {
  const uint32_t e = blockIdx.x * TPB + threadIdx.x;
  if (e < NE && flag[e]) cell_slot[gkeys[e]] = (uint32_t)*base + scan[e];
}
// gmeta[g] = input cells | (op code | field << 8) << 16
__global__ void plan_gen_ops_kernel(uint32_t S, uint32_t G, const uint32_t *gmeta, OpRec *recs) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i < G) recs[S + i] = make_uint2(i, gmeta[i] >> 16);
}

// what the compilers read of the circuit
struct Rows {
  const uint8_t *row_gate;
  const GateDesc *gates;
  const gl_t *gconsts;
  uint32_t d, R, ngc;
  __device__ __forceinline__ gl_t lc(uint32_t i, uint32_t row) const { return i < ngc ? gconsts[((size_t)i << d) + row] : (gl_t)0; }
  __device__ __forceinline__ size_t key(uint32_t row, uint32_t col) const { return ((size_t)col << d) + row; }
};

// One row, ops left to right, by the host's rules (Compiler::row_ops / add_op): an op is kept when one of its routed cells has
// a slot, and then every routed output cell without one takes the next; a BaseSum row that has a slot at all gives every cell
// 0 .. limbs one first and keeps both directions.  FILL = false counts (ops kept, new slots), FILL = true writes the slots
// from `slot` on and the op records from `op` on.
template <bool FILL>
__device__ __forceinline__ void plan_row(const Rows &x, uint32_t row, uint32_t *cell_slot, uint32_t &op, uint32_t &slot, OpRec *recs,
                                         uint32_t recs_cap) {
  const GateDesc g = x.gates[x.row_gate[row]];
  const uint32_t R = x.R;
  const gl_t c0 = x.lc(0, row), c1 = x.lc(1, row);
  auto take = [&](uint32_t col) {
    if (col >= R || cell_slot[x.key(row, col)] != UNSET) return;
    if (FILL) cell_slot[x.key(row, col)] = slot;
    slot++;
  };
  auto keep = [&](const OpCols &o) {
    if (FILL && op < recs_cap) recs[op] = make_uint2(row, o.code | (o.sub << 8));
    op++;
  };
  if (g.kind == G_BASE_SUM) {
    bool active = false;
    for (uint32_t col = 0; col <= g.p[1] && col < R; col++) active |= cell_slot[x.key(row, col)] != UNSET;
    if (!active) return;
    for (uint32_t col = 0; col <= g.p[1] && col < R; col++) take(col);
    keep(row_op(g, 0, c0, c1));
    keep(row_op(g, 1, c0, c1));
    return;
  }
  for (uint32_t k = 0, m = row_num_ops(g); k < m; k++) {
    const OpCols o = row_op(g, k, c0, c1);
    bool active = false;
    auto has_slot = [&](uint32_t col) { active |= col < R && cell_slot[x.key(row, col)] != UNSET; };
    for_cols(o.in, has_slot);
    for_cols(o.out, has_slot);
    if (!active) continue;
    for_cols(o.out, take);
    keep(o);
  }
}

__global__ void plan_rows_count_kernel(Rows x, uint32_t *cell_slot, uint32_t *n_ops, uint32_t *n_new) {
  const size_t n = (size_t)1 << x.d, step = (size_t)gridDim.x * TPB;
  for (size_t row = (size_t)blockIdx.x * TPB + threadIdx.x; row < n; row += step) {
    uint32_t op = 0, slot = 0;
    plan_row<false>(x, (uint32_t)row, cell_slot, op, slot, nullptr, 0);
    n_ops[row] = op;
    n_new[row] = slot;
  }
}
__global__ void plan_rows_fill_kernel(Rows x, uint32_t *cell_slot, const uint32_t *op_off, const uint32_t *new_off, uint32_t S,
                                      const unsigned long long *slot_base, OpRec *recs, uint32_t n_ops) {
  const size_t n = (size_t)1 << x.d, step = (size_t)gridDim.x * TPB;
  for (size_t row = (size_t)blockIdx.x * TPB + threadIdx.x; row < n; row += step) {
    uint32_t op = S + op_off[row], slot = (uint32_t)*slot_base + new_off[row];
    plan_row<true>(x, (uint32_t)row, cell_slot, op, slot, recs, n_ops);
  }
}
__global__ void plan_seed_ops_kernel(uint32_t S, OpRec *recs) {
  const uint32_t i = blockIdx.x * TPB + threadIdx.x;
  if (i < S) recs[i] = make_uint2(i, OP_SEED);
}

// the cells of op i as the schedule sees them: f(key) over the routed input cells that have a slot / f(key, word) over the
// routed output cells, `word` the generator-table word that takes the writer bit of a generator's cell (null: cell_slot[key] does)
struct OpView {
  Rows x;
  const OpRec *recs;
  const uint2 *seeds;
  const uint32_t *cell_slot;
  const uint32_t *gkeys;  // the generators' cell keys, generator g's from goff[g] on: its gmeta[g] & 0xFFFF inputs, then its outputs
  uint32_t *gen_table;    // the same with the writer bits the schedule sets
  const uint32_t *goff;   // [generators + 1]
  const uint32_t *gmeta;  // [generators] input cells | (op code | field << 8) << 16
  template <class F> __device__ __forceinline__ void ins(uint32_t i, F &&f) const {
    const OpRec r = recs[i];
    const uint32_t code = r.y & 0xFF;
    if (code == OP_SEED) return;
    if (op_is_listed_generator(code)) {  // (every cell a generator names has a slot)
      for (uint32_t e = goff[r.x], end = e + (gmeta[r.x] & 0xFFFF); e < end; e++) f((size_t)gkeys[e]);
      return;
    }
    const GateDesc g = x.gates[x.row_gate[r.x]];
    const OpCols o = row_op(g, op_index_in_row(g, code, r.y >> 8), x.lc(0, r.x), x.lc(1, r.x));
    for_cols(o.in, [&](uint32_t col) {
      if (col < x.R && cell_slot[x.key(r.x, col)] != UNSET) f(x.key(r.x, col));
    });
  }
  template <class F> __device__ __forceinline__ void outs(uint32_t i, F &&f) const {
    const OpRec r = recs[i];
    const uint32_t code = r.y & 0xFF;
    if (code == OP_SEED) {
      const uint2 c = seeds[r.x];
      if (c.y < x.R) f(x.key(c.x, c.y), (uint32_t *)nullptr);
      return;
    }
    if (op_is_listed_generator(code)) {
      for (uint32_t e = goff[r.x] + (gmeta[r.x] & 0xFFFF), end = goff[r.x + 1]; e < end; e++) f((size_t)gkeys[e], gen_table + e);
      return;
    }
    const GateDesc g = x.gates[x.row_gate[r.x]];
    const OpCols o = row_op(g, op_index_in_row(g, code, r.y >> 8), 0, 0);  // (the constants decide inputs only)
    for_cols(o.out, [&](uint32_t col) {
      if (col < x.R) f(x.key(r.x, col), (uint32_t *)nullptr);
    });
  }
};

// users: slot -> the ops that read it.  pending[i] = input cells of op i; use_cnt[s] = input cells over all ops that hold slot s
__global__ void plan_users_count_kernel(OpView v, uint32_t n_ops, uint32_t *pending, uint32_t *use_cnt) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_ops; i += step) {
    uint32_t k = 0;
    v.ins((uint32_t)i, [&](size_t key) {
      atomicAdd(&use_cnt[v.cell_slot[key] & ~WRITER], 1u);
      k++;
    });
    pending[i] = k;
  }
}
// (the order inside a slot's list does not matter: the level walk sorts what becomes ready)
__global__ void plan_users_fill_kernel(OpView v, uint32_t n_ops, uint32_t *fill, uint32_t *users, size_t users_cap, const uint32_t *pending,
                                       uint32_t *queue, unsigned long long *ready) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_ops; i += step) {
    v.ins((uint32_t)i, [&](size_t key) {
      const uint32_t at = atomicAdd(&fill[v.cell_slot[key] & ~WRITER], 1u);
      if (at < users_cap) users[at] = (uint32_t)i;
    });
    if (!pending[i]) queue[atomicAdd(ready, 1ull)] = (uint32_t)i;
  }
}

// ---- 4. levels ----
struct SchedArgs {
  OpView v;
  uint32_t *cell_slot;            // (v.cell_slot, writable: the writer bits)
  int32_t *level;                 // [n_ops] -1 / LEVEL_DEAD / the level the op runs in
  uint32_t *pending;              // [n_ops] input cells whose slot nobody has claimed yet
  int32_t *slot_level;            // [slots] -1 / the level of the op that writes the slot
  unsigned long long *slot_min;   // [slots] round tag << 32 | the smallest contender of the round
  unsigned long long *twin_min;   // [n_ops] the same for a BaseSum pair, at the split's index
  const uint32_t *use_off, *users;
  uint32_t *queue[2];             // [n_ops] each: this level's ready ops, the next level's
  uint8_t *state;                 // [n_ops] per entry of this level's queue: decided
  uint32_t *level_off;            // [n_ops + 2]
  uint32_t *res;                  // [S_COUNT]
  uint32_t n_ops, ready;
};

// The host walks a level's ready ops in ascending index; an op TAKES the level unless it is dead (its twin took earlier) or one
// of its output slots was first claimed in this same level by an earlier op that took -- then it waits one level and will
// compare.  An op that waits claims nothing.  The same recurrence in rounds, one workgroup, a barrier between the steps:
//   A  every undecided op: dead -> dropped; an output slot claimed in this level -> waits (joins the next level's queue);
//      otherwise atomicMin of its index on each still unclaimed output slot and on the word it shares with its twin;
//   B  an op that holds the minimum on every word it contended for takes: level, claims (slot_level, writer bit of the first
//      cell in its own order), twin dead, pending of the claimed slots' users down -- a user reaching 0 joins the next queue.
// Exact, not approximate: the smallest undecided index i0 has every earlier op decided, so the sequential walk takes it too.
// Another op j that holds all its minima shares no unclaimed output slot with an undecided k < j and is no such k's twin, so
// whatever those k decide -- take or wait -- claims nothing j writes: the sequential walk reaches j with the same claims
// and takes it.  And j's own claims are on slots no undecided k < j has as an output, so no earlier op's decision sees them.
// i0 always decides, hence rounds <= queue length; levels <= ops + 1 (a level without a taker holds dead ops only and is the
// last).  Past either cap the kernel writes S_ERROR and returns; nothing here waits on another workgroup or spins on a flag.
// The words of slot_min / twin_min carry the round in their high half, counted DOWN, so a later round's contender always
// beats what an earlier round left behind and nothing has to be reset.
__global__ __launch_bounds__(SCHED_TPB) void plan_schedule_kernel(SchedArgs a) {
  __shared__ uint32_t s_next, s_took, s_undec[2];
  const uint32_t t = threadIdx.x;
  if (t == 0) {
    s_next = s_took = s_undec[0] = s_undec[1] = 0;
    a.level_off[0] = 0;
  }
  __syncthreads();
  // an op joins the next level's queue once at most (it waits, or its last input was claimed): the bound holds by construction
  // and is checked at the level's end; no entry is ever written past the queue
  auto push = [&](uint32_t *next, uint32_t i) {
    const uint32_t at = atomicAdd(&s_next, 1u);
    if (at < a.n_ops) st_shared(next + at, i);
  };
  uint32_t ncur = a.ready, done = 0, widest = 0, lvl = 0, err = 0, cq = 0;
  uint32_t round = 1;  // (round 0's tag is what the cleared words hold)
  for (; ncur; lvl++) {
    if (lvl > a.n_ops) { err = 1; break; }
    const uint32_t *cur = a.queue[cq];
    uint32_t *next = a.queue[cq ^ 1];
    for (uint32_t k = t; k < ncur; k += SCHED_TPB) a.state[k] = 0;  // (entry k stays with lane k % SCHED_TPB)
    uint32_t undec = ncur, rounds = 0;
    while (undec) {
      if (rounds++ >= ncur || round == 0xFFFFFFFEu) { err = 2; break; }
      const uint32_t par = round & 1;
      const unsigned long long tag = (unsigned long long)(~round) << 32;
      round++;
      // ---- A ----
      for (uint32_t k = t; k < ncur; k += SCHED_TPB) {
        if (a.state[k]) continue;
        const uint32_t i = ld_shared(cur + k);
        if (ld_shared(a.level + i) == LEVEL_DEAD) { a.state[k] = 1; continue; }
        bool wait = false;
        a.v.outs(i, [&](size_t key, uint32_t *) { wait |= ld_shared(a.slot_level + (a.cell_slot[key] & ~WRITER)) == (int32_t)lvl; });
        if (wait) {
          a.state[k] = 1;
          push(next, i);
          continue;
        }
        a.v.outs(i, [&](size_t key, uint32_t *) {
          const uint32_t s = a.cell_slot[key] & ~WRITER;
          if (ld_shared(a.slot_level + s) < 0) atomicMin(a.slot_min + s, tag | i);
        });
        const uint32_t code = a.v.recs[i].y & 0xFF;
        if (code == OP_BASE_SPLIT) atomicMin(a.twin_min + i, tag | i);
        else if (code == OP_BASE_JOIN) atomicMin(a.twin_min + i - 1, tag | i);
      }
      __syncthreads();
      if (t == 0) s_undec[par ^ 1] = 0;  // (the next round's counter: everyone has read it past the barrier above)
      // ---- B ----
      for (uint32_t k = t; k < ncur; k += SCHED_TPB) {
        if (a.state[k]) continue;
        const uint32_t i = ld_shared(cur + k);
        const unsigned long long mine = tag | i;
        bool ok = true;
        a.v.outs(i, [&](size_t key, uint32_t *) {
          const unsigned long long m = ld_shared(a.slot_min + (a.cell_slot[key] & ~WRITER));
          ok &= (m >> 32) != (tag >> 32) || m == mine;  // (a word nobody contended for in this round: claimed in an earlier level)
        });
        const uint32_t code = a.v.recs[i].y & 0xFF;
        uint32_t twin = UNSET;
        if (code == OP_BASE_SPLIT) twin = i + 1, ok &= ld_shared(a.twin_min + i) == mine;
        else if (code == OP_BASE_JOIN) twin = i - 1, ok &= ld_shared(a.twin_min + i - 1) == mine;
        if (!ok) {
          atomicAdd(&s_undec[par], 1u);
          continue;
        }
        a.state[k] = 1;
        st_shared(a.level + i, (int32_t)lvl);
        atomicAdd(&s_took, 1u);
        if (twin != UNSET) st_shared(a.level + twin, LEVEL_DEAD);
        a.v.outs(i, [&](size_t key, uint32_t *gen_word) {
          const uint32_t s = a.cell_slot[key] & ~WRITER;
          if (atomicCAS(a.slot_level + s, -1, (int32_t)lvl) != -1) return;
          if (gen_word) *gen_word = (uint32_t)key | WRITER;  // (a generator's writer bit lives in its own table word)
          else a.cell_slot[key] = s | WRITER;
          for (uint32_t u = a.use_off[s], e = a.use_off[s + 1]; u < e; u++) {
            const uint32_t user = a.users[u];
            if (atomicSub(a.pending + user, 1u) == 1u) push(next, user);
          }
        });
      }
      __syncthreads();
      undec = s_undec[par];
    }
    if (err) break;
    const uint32_t took = s_took, nn = s_next;
    __syncthreads();
    done += took;
    widest = max(widest, took);
    if (t == 0) {
      s_took = s_next = 0;
      a.level_off[lvl + 1] = done;
    }
    if (nn > a.n_ops) { err = 3; break; }  // (every op joins a level's queue once at most)
    ncur = nn;
    cq ^= 1;
    __syncthreads();
  }
  if (t == 0) {
    a.res[S_LEVELS] = lvl;
    a.res[S_WIDEST] = widest;
    a.res[S_ERROR] = err;
    a.res[S_DONE] = done;
  }
}

// order: the levelled ops by (level, creation order); the others sort behind them
__global__ void plan_order_keys_kernel(const int32_t *level, uint32_t n_ops, unsigned long long *keys) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_ops; i += step)
    keys[i] = level[i] >= 0 ? ((unsigned long long)level[i] << 32) | i : ~0ull;
}
__global__ void plan_order_gather_kernel(const unsigned long long *sorted, uint32_t count, const OpRec *recs, OpRec *out) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t k = (size_t)blockIdx.x * TPB + threadIdx.x; k < count; k += step) out[k] = recs[(uint32_t)sorted[k]];
}

// ---- 5. what the schedule did not reach ----
// producer[s]: bit 0 = some op other than a BaseSum join sets it, bit 1 = a join does (every op counts, scheduled or not)
__global__ void plan_producers_kernel(OpView v, uint32_t n_ops, uint32_t *producer) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t i = (size_t)blockIdx.x * TPB + threadIdx.x; i < n_ops; i += step) {
    const uint32_t bit = (v.recs[i].y & 0xFF) == OP_BASE_JOIN ? 2u : 1u;
    v.outs((uint32_t)i, [&](size_t key, uint32_t *) { atomicOr(&producer[v.cell_slot[key] & ~WRITER], bit); });
  }
}
// the smallest unreached cell without a producer / with joins only / with any other producer
__global__ void plan_unreached_kernel(const uint32_t *cell_slot, size_t tot, const int32_t *slot_level, const uint32_t *producer,
                                      unsigned long long *words /* [3] */) {
  const size_t step = (size_t)gridDim.x * TPB;
  for (size_t v = (size_t)blockIdx.x * TPB + threadIdx.x; v < tot; v += step) {
    const uint32_t s = cell_slot[v];
    if (s == UNSET || slot_level[s & ~WRITER] >= 0) continue;
    const uint32_t f = producer[s & ~WRITER];
    atomicMin(&words[f == 0 ? 0 : f == 2 ? 1 : 2], (unsigned long long)v);
  }
}

// what the phases of one compilation share: the sizes, the stream, the counters and the scratch pointers (all inside S)
struct PlanCtx {
  p2gpu_circuit *c;
  classes::Scratch &S;
  const std::vector<PlanSeed> &seeds;
  const PlanGenList &gens;
  hipStream_t st;
  size_t n, tot;
  uint32_t R, d, ngc, NS, NG;
  double t0;
  unsigned long long h[C_COUNT];  // the counters as last read back
  unsigned long long *ctr = nullptr;
  uint2 *d_seeds = nullptr;
  uint32_t *gkeys = nullptr, *gen_table = nullptr, *goff = nullptr, *gmeta = nullptr;
  uint32_t *partner = nullptr, *parent = nullptr, *cell_slot = nullptr;
  unsigned long long *list = nullptr;
  uint32_t slots = 0, NO = 0, n_done = 0;
  OpRec *recs = nullptr, *ordered = nullptr;
  int32_t *level = nullptr, *slot_level = nullptr;
  unsigned long long *slot_min = nullptr, *keys = nullptr;
  uint32_t *level_off = nullptr;
  uint32_t hres[S_COUNT];
  SchedArgs sched;

  PlanCtx(p2gpu_circuit *c_, const std::vector<PlanSeed> &seeds_, const PlanGenList &gens_, classes::Scratch &S_)
      : c(c_), S(S_), seeds(seeds_), gens(gens_), st(c_->stream), n(c_->n), tot((size_t)c_->R * c_->n), R(c_->R), d(c_->d),
        ngc(c_->NC - c_->num_selectors), NS((uint32_t)seeds_.size()), NG((uint32_t)gens_.size()), t0(now_ms()) {}
  Rows rows() const { return Rows{c->d_row_gate.p, c->d_gates.p, c->d_gconsts.p, d, R, ngc}; }
  OpView view() const { return OpView{rows(), recs, d_seeds, cell_slot, gkeys, gen_table, goff, gmeta}; }
  void mark(const char *label) const {
    if (!trace_on()) return;
    (void)hipStreamSynchronize(st);
    fprintf(stderr, "[p2gpu] plan %-28s +%.2f ms\n", label, now_ms() - t0);
  }
  int fail(const char *what, hipError_t e) const {
    (void)hipGetLastError();
    set_err("p2gpu_witness_plan_build: %s: %s", what, hipGetErrorString(e));
    return P2GPU_E_DEVICE;
  }
  // false, with the error set, when a runtime call failed
  bool ok(hipError_t e, const char *what) const { return e == hipSuccess || (fail(what, e), false); }
  int refuse(PlanRefusalKind kind, unsigned long long key) const { return plan_refuse(c, PlanRefusal::at(kind, key, d)); }
  int decode(), copy_classes(), slots_ops(), levels(), unreached();  // the phases, in order
};

// ---- 1. decode sigma ----
int PlanCtx::decode() {
  partner = S.alloc<uint32_t>(tot);
  parent = S.alloc<uint32_t>(tot);
  list = S.alloc<unsigned long long>(tot);
  cell_slot = S.alloc<uint32_t>(tot);
  d_seeds = S.alloc<uint2>(NS);
  if (!partner || !parent || !list || !cell_slot || !d_seeds) return fail("scratch (classes)", hipErrorOutOfMemory);
  if (NS && !ok(hipMemcpyAsync(d_seeds, seeds.data(), sizeof(uint2) * NS, hipMemcpyHostToDevice, st), "copy the seed cells")) return P2GPU_E_DEVICE;
  const char *step = "decode sigma";
  if (!ok(sigma_partners(c, S, partner, ctr + C_BAD_SIGMA, &step), step)) return P2GPU_E_DEVICE;
  return P2GPU_OK;
}

// ---- 2. classes -> class slots ----
int PlanCtx::copy_classes() {
  if (!ok(hipMemsetAsync(parent, 0xFF, 4 * tot, st), "scratch")) return P2GPU_E_DEVICE;
  const SigmaPairs pairs{partner};
  hipLaunchKernelGGL(classes::touch_kernel<SigmaPairs>, dim3(grid_for(tot)), dim3(TPB), 0, st, pairs, tot, parent, list, ctr + C_TOUCHED);
  if (!ok(hipMemcpyAsync(h, ctr, 16, hipMemcpyDeviceToHost, st), "read the decode")) return P2GPU_E_DEVICE;
  if (!ok(hipStreamSynchronize(st), "decode")) return P2GPU_E_DEVICE;
  mark("decode sigma, touch");
  if (h[C_BAD_SIGMA] != UINT64_MAX) return refuse(PLAN_BAD_SIGMA, h[C_BAD_SIGMA]);
  const size_t T = (size_t)h[C_TOUCHED];
  if (T > tot) { set_err("p2gpu_witness_plan_build: internal error (touched cells)"); return P2GPU_E_DEVICE; }
  uint32_t *changed = S.alloc<uint32_t>(1);
  if (!changed) return fail("scratch", hipErrorOutOfMemory);
  if (T)
    if (int rc = classes::settle(pairs, tot, list, T, parent, changed, st, "p2gpu_witness_plan_build")) return rc;
  mark("copy classes");
  // class slots: the rank of the root among roots (the touched list's memory holds the flags and their scan from here on)
  uint32_t *flag = (uint32_t *)list, *rank = flag + tot;
  hipLaunchKernelGGL(plan_root_flags_kernel, dim3(grid_for(tot)), dim3(TPB), 0, st, parent, tot, flag);
  if (!ok(S.exclusive_scan(flag, rank, tot, st), "scan (roots)")) return P2GPU_E_DEVICE;
  hipLaunchKernelGGL(plan_total_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long *)nullptr, flag, rank, tot, ctr + C_CLASSES);
  hipLaunchKernelGGL(plan_class_slots_kernel, dim3(grid_for(tot)), dim3(TPB), 0, st, parent, rank, tot, cell_slot);
  return P2GPU_OK;
}

// ---- 3. slots and ops: the seeds, then the generators that are no gate's own, then the rows; the users of every slot ----
// Leaves the schedule's arguments in `sched` (everything but the ready count is scratch of this phase and the next).
int PlanCtx::slots_ops() {
  SchedArgs &a = sched;
  uint32_t *sflag = S.alloc<uint32_t>(2 * (size_t)NS), *rcnt = S.alloc<uint32_t>(4 * n);
  if (!sflag || !rcnt) return fail("scratch (rows)", hipErrorOutOfMemory);
  if (NS) {
    hipLaunchKernelGGL(plan_seed_flags_kernel, dim3((NS + TPB - 1) / TPB), dim3(TPB), 0, st, d_seeds, NS, d, R, cell_slot, sflag);
    if (!ok(S.exclusive_scan(sflag, sflag + NS, NS, st), "scan (seeds)")) return P2GPU_E_DEVICE;
    hipLaunchKernelGGL(plan_seed_slots_kernel, dim3((NS + TPB - 1) / TPB), dim3(TPB), 0, st, d_seeds, NS, d, sflag, sflag + NS, ctr + C_CLASSES,
                       cell_slot);
  }
  hipLaunchKernelGGL(plan_total_kernel, dim3(1), dim3(1), 0, st, ctr + C_CLASSES, sflag, sflag + NS, (size_t)NS, ctr + C_SEED_SLOTS);
  // the generators' cells: keys from the checked list (every cell inside [n] x [R]), slots behind the seeds'
  const uint32_t NE = gens.n_cells();
  uint32_t *gflag = S.alloc<uint32_t>(2 * (size_t)NE);
  gkeys = S.alloc<uint32_t>(NE);
  gen_table = S.alloc<uint32_t>(NE);
  goff = S.alloc<uint32_t>((size_t)NG + 1);
  gmeta = S.alloc<uint32_t>(NG);
  if (!gflag || !gkeys || !gen_table || !goff || !gmeta) return fail("scratch (generators)", hipErrorOutOfMemory);
  size_t gen_ins = 0;  // the input cells of all generators
  if (NE) {
    std::vector<uint32_t> hkeys(NE), hmeta(NG);
    for (uint32_t e = 0; e < NE; e++) hkeys[e] = (gens.cells[2 * (size_t)e + 1] << d) + gens.cells[2 * (size_t)e];
    for (uint32_t g = 0; g < NG; g++) hmeta[g] = gens.ins(g) | gens.code_word(g) << 16, gen_ins += gens.ins(g);
    // (pageable memory: the copies have left the vectors when the call returns)
    if (!ok(hipMemcpyAsync(gkeys, hkeys.data(), 4 * (size_t)NE, hipMemcpyHostToDevice, st), "copy the generator cells")) return P2GPU_E_DEVICE;
    if (!ok(hipMemcpyAsync(goff, gens.off.data(), 4 * ((size_t)NG + 1), hipMemcpyHostToDevice, st), "copy the generator cells")) return P2GPU_E_DEVICE;
    if (!ok(hipMemcpyAsync(gmeta, hmeta.data(), 4 * (size_t)NG, hipMemcpyHostToDevice, st), "copy the generator cells")) return P2GPU_E_DEVICE;
    if (!ok(hipStreamSynchronize(st), "copy the generator cells")) return P2GPU_E_DEVICE;
    if (!ok(hipMemcpyAsync(gen_table, gkeys, 4 * (size_t)NE, hipMemcpyDeviceToDevice, st), "scratch")) return P2GPU_E_DEVICE;
    const dim3 gg((NE + TPB - 1) / TPB);
    uint32_t *first = partner;  // (the decoded partners are done with once the classes stand)
    hipLaunchKernelGGL(plan_gen_clear_kernel, gg, dim3(TPB), 0, st, gkeys, NE, first);
    hipLaunchKernelGGL(plan_gen_first_kernel, gg, dim3(TPB), 0, st, gkeys, NE, cell_slot, first);
    hipLaunchKernelGGL(plan_gen_flags_kernel, gg, dim3(TPB), 0, st, gkeys, NE, cell_slot, first, gflag);
    if (!ok(S.exclusive_scan(gflag, gflag + NE, NE, st), "scan (generators)")) return P2GPU_E_DEVICE;
    hipLaunchKernelGGL(plan_gen_slots_kernel, gg, dim3(TPB), 0, st, gkeys, NE, gflag, gflag + NE, ctr + C_SEED_SLOTS, cell_slot);
  }
  hipLaunchKernelGGL(plan_total_kernel, dim3(1), dim3(1), 0, st, ctr + C_SEED_SLOTS, gflag, gflag + NE, (size_t)NE, ctr + C_GEN_SLOTS);
  uint32_t *row_ops = rcnt, *row_new = rcnt + n, *op_off = rcnt + 2 * n, *new_off = rcnt + 3 * n;
  hipLaunchKernelGGL(plan_rows_count_kernel, dim3(grid_for(n)), dim3(TPB), 0, st, rows(), cell_slot, row_ops, row_new);
  if (!ok(S.exclusive_scan(row_ops, op_off, n, st), "scan (ops)")) return P2GPU_E_DEVICE;
  if (!ok(S.exclusive_scan(row_new, new_off, n, st), "scan (slots)")) return P2GPU_E_DEVICE;
  hipLaunchKernelGGL(plan_total_kernel, dim3(1), dim3(1), 0, st, (const unsigned long long *)nullptr, row_ops, op_off, n, ctr + C_ROW_OPS);
  hipLaunchKernelGGL(plan_total_kernel, dim3(1), dim3(1), 0, st, ctr + C_GEN_SLOTS, row_new, new_off, n, ctr + C_SLOTS);
  if (!ok(hipMemcpyAsync(h, ctr, sizeof h, hipMemcpyDeviceToHost, st), "read the counts")) return P2GPU_E_DEVICE;
  if (!ok(hipStreamSynchronize(st), "count")) return P2GPU_E_DEVICE;
  mark("class slots, seeds, generators, row count");
  const unsigned long long slots64 = h[C_SLOTS], ops64 = (unsigned long long)NS + NG + h[C_ROW_OPS];
  if (slots64 >= WRITER || ops64 >= (1ull << 32)) return refuse(PLAN_TOO_LARGE, 0);
  slots = (uint32_t)slots64, NO = (uint32_t)ops64;
  if (slots > tot) { set_err("p2gpu_witness_plan_build: internal error (slot count)"); return P2GPU_E_DEVICE; }
  // per op and per slot
  recs = S.alloc<OpRec>(NO);
  ordered = S.alloc<OpRec>(NO);
  uint32_t *pending = S.alloc<uint32_t>(NO), *queue = S.alloc<uint32_t>(2 * (size_t)NO);
  level_off = S.alloc<uint32_t>((size_t)NO + 2);
  level = S.alloc<int32_t>(NO), slot_level = S.alloc<int32_t>(slots);
  unsigned long long *twin_min = S.alloc<unsigned long long>(NO);
  slot_min = S.alloc<unsigned long long>(slots);
  keys = S.alloc<unsigned long long>(2 * (size_t)NO);
  uint8_t *state = S.alloc<uint8_t>(NO);
  uint32_t *use_cnt = S.alloc<uint32_t>((size_t)slots + 1), *use_off = S.alloc<uint32_t>((size_t)slots + 1);
  uint32_t *res = S.alloc<uint32_t>(S_COUNT);
  // the classes are numbered: parent is free.  Every routed cell is an input of one row op at most and of any number of
  // generators: <= tot + (the generators' input cells) entries
  const size_t users_cap = tot + gen_ins;
  uint32_t *users = NG ? S.alloc<uint32_t>(users_cap) : parent;
  if (!recs || !ordered || !pending || !queue || !level_off || !level || !slot_level || !twin_min || !slot_min || !keys || !state || !use_cnt ||
      !use_off || !res || !users)
    return fail("scratch (schedule)", hipErrorOutOfMemory);
  if (NS) hipLaunchKernelGGL(plan_seed_ops_kernel, dim3((NS + TPB - 1) / TPB), dim3(TPB), 0, st, NS, recs);
  if (NG) hipLaunchKernelGGL(plan_gen_ops_kernel, dim3((NG + TPB - 1) / TPB), dim3(TPB), 0, st, NS, NG, gmeta, recs);
  hipLaunchKernelGGL(plan_rows_fill_kernel, dim3(grid_for(n)), dim3(TPB), 0, st, rows(), cell_slot, op_off, new_off, NS + NG, ctr + C_GEN_SLOTS, recs, NO);
  if (!ok(hipMemsetAsync(use_cnt, 0, 4 * ((size_t)slots + 1), st), "scratch")) return P2GPU_E_DEVICE;
  if (!ok(hipMemsetAsync(level, 0xFF, 4 * (size_t)std::max(1u, NO), st), "scratch")) return P2GPU_E_DEVICE;
  if (!ok(hipMemsetAsync(slot_level, 0xFF, 4 * (size_t)std::max(1u, slots), st), "scratch")) return P2GPU_E_DEVICE;
  if (!ok(hipMemsetAsync(twin_min, 0xFF, 8 * (size_t)std::max(1u, NO), st), "scratch")) return P2GPU_E_DEVICE;
  if (!ok(hipMemsetAsync(slot_min, 0xFF, 8 * (size_t)std::max(1u, slots), st), "scratch")) return P2GPU_E_DEVICE;
  if (!ok(hipMemsetAsync(res, 0, 4 * S_COUNT, st), "scratch")) return P2GPU_E_DEVICE;
  hipLaunchKernelGGL(plan_users_count_kernel, dim3(grid_for(NO)), dim3(TPB), 0, st, view(), NO, pending, use_cnt);
  if (!ok(S.exclusive_scan(use_cnt, use_off, (size_t)slots + 1, st), "scan (users)")) return P2GPU_E_DEVICE;
  if (!ok(hipMemcpyAsync(use_cnt, use_off, 4 * ((size_t)slots + 1), hipMemcpyDeviceToDevice, st), "scratch")) return P2GPU_E_DEVICE;  // (the fill pointers)
  hipLaunchKernelGGL(plan_users_fill_kernel, dim3(grid_for(NO)), dim3(TPB), 0, st, view(), NO, use_cnt, users, users_cap, pending, queue, ctr + C_READY);
  if (!ok(hipMemcpyAsync(h + C_READY, ctr + C_READY, 8, hipMemcpyDeviceToHost, st), "read the ready ops")) return P2GPU_E_DEVICE;
  if (!ok(hipStreamSynchronize(st), "ops")) return P2GPU_E_DEVICE;
  mark("ops, users");
  if (h[C_READY] > NO) { set_err("p2gpu_witness_plan_build: internal error (ready ops)"); return P2GPU_E_DEVICE; }
  a.v = view(); a.cell_slot = cell_slot; a.level = level; a.pending = pending; a.slot_level = slot_level; a.slot_min = slot_min;
  a.twin_min = twin_min; a.use_off = use_off; a.users = users; a.queue[0] = queue; a.queue[1] = queue + NO; a.state = state;
  a.level_off = level_off; a.res = res; a.n_ops = NO; a.ready = (uint32_t)h[C_READY];
  return P2GPU_OK;
}

// ---- 4. levels, and the ops in their order ----
int PlanCtx::levels() {
  const SchedArgs &a = sched;
  hipLaunchKernelGGL(plan_schedule_kernel, dim3(1), dim3(SCHED_TPB), 0, st, a);
  if (!ok(hipMemcpyAsync(hres, a.res, sizeof hres, hipMemcpyDeviceToHost, st), "read the schedule")) return P2GPU_E_DEVICE;
  if (!ok(hipStreamSynchronize(st), "levels")) return P2GPU_E_DEVICE;
  mark("levels");
  if (hres[S_ERROR] || hres[S_DONE] > NO || hres[S_LEVELS] > (unsigned long long)NO + 1) {
    set_err("p2gpu_witness_plan_build: internal error (the level walk stopped at its cap, code %u)", hres[S_ERROR]);
    return P2GPU_E_DEVICE;
  }
  n_done = hres[S_DONE];
  hipLaunchKernelGGL(plan_order_keys_kernel, dim3(grid_for(NO)), dim3(TPB), 0, st, level, NO, keys);
  if (NO) {
    const auto sort = S.radix_sort_keys(keys, keys + NO, NO, 0u, 64u, st);
    if (!ok(sort.e, sort.step)) return P2GPU_E_DEVICE;
  }
  hipLaunchKernelGGL(plan_order_gather_kernel, dim3(grid_for(n_done)), dim3(TPB), 0, st, keys + NO, n_done, recs, ordered);
  return P2GPU_OK;
}

// ---- 5. what the schedule did not reach ----
int PlanCtx::unreached() {
  uint32_t *producer = (uint32_t *)slot_min;
  if (!ok(hipMemsetAsync(producer, 0, 4 * (size_t)std::max(1u, slots), st), "scratch")) return P2GPU_E_DEVICE;
  hipLaunchKernelGGL(plan_producers_kernel, dim3(grid_for(NO)), dim3(TPB), 0, st, view(), NO, producer);
  hipLaunchKernelGGL(plan_unreached_kernel, dim3(grid_for(tot)), dim3(TPB), 0, st, cell_slot, tot, slot_level, producer, ctr + C_NO_PRODUCER);
  static_assert(C_JOIN_ONLY == C_NO_PRODUCER + 1 && C_OTHER == C_NO_PRODUCER + 2, "three consecutive words");
  if (!ok(hipMemcpyAsync(h + C_NO_PRODUCER, ctr + C_NO_PRODUCER, 24, hipMemcpyDeviceToHost, st), "read the unreached cells")) return P2GPU_E_DEVICE;
  if (!ok(hipStreamSynchronize(st), "order")) return P2GPU_E_DEVICE;
  if (!ok(hipGetLastError(), "kernel launch")) return P2GPU_E_DEVICE;
  mark("order, unreached cells");
  const unsigned long long stuck = h[C_NO_PRODUCER] != UINT64_MAX ? h[C_NO_PRODUCER] : h[C_JOIN_ONLY];
  if (stuck != UINT64_MAX) return refuse(PLAN_SEED_MISSING, stuck);
  if (h[C_OTHER] != UINT64_MAX) return refuse(PLAN_CYCLE, h[C_OTHER]);
  return P2GPU_OK;
}

}  // namespace

namespace p2 {

hipError_t sigma_partners(p2gpu_circuit *c, classes::Scratch &S, uint32_t *partner, unsigned long long *bad, const char **step) {
  const uint32_t R = c->R, d = c->d;
  const size_t n = c->n, tot = (size_t)R * n;
  hipStream_t st = c->stream;
  std::vector<gl_t> kpow(2 * (size_t)R);
  for (uint32_t col = 0; col < R; col++) {
    gl_t t = c->k_is[col];
    for (uint32_t i = 0; i < d; i++) t = gl_sqr(t);
    kpow[col] = t;
    kpow[R + col] = gl_inv(c->k_is[col]);
  }
  gl_t *d_kpow = S.alloc<gl_t>(2 * (size_t)R);
  gl_t *wkeys = S.alloc<gl_t>(2 * n);
  uint32_t *wrows = S.alloc<uint32_t>(2 * n);
  *step = "scratch (decode sigma)";
  if (!d_kpow || !wkeys || !wrows) return hipErrorOutOfMemory;
  *step = "copy the coset powers";
  // (pageable host memory: the copy has left kpow when the call returns)
  if (hipError_t e = hipMemcpyAsync(d_kpow, kpow.data(), 16 * (size_t)R, hipMemcpyHostToDevice, st)) return e;
  hipLaunchKernelGGL(plan_powers_kernel, dim3(grid_for(n)), dim3(TPB), 0, st, c->tw_fwd.p, d, wkeys, wrows);
  const auto sort = S.radix_sort_pairs(wkeys, wkeys + n, wrows, wrows + n, n, 0u, 64u, st);
  *step = sort.step;
  if (sort.e != hipSuccess) return sort.e;
  hipLaunchKernelGGL(plan_decode_kernel, dim3(grid_for(tot)), dim3(TPB), 0, st, c->d_sigmas.p, c->d_kis.p, d_kpow, c->tw_fwd.p, wkeys + n,
                     wrows + n, d, R, partner, bad);
  *step = "decode sigma";
  return hipSuccess;
}

int plan_compile_device(p2gpu_circuit *c, const std::vector<PlanSeed> &seeds, const PlanGenList &gens, classes::Scratch &S, PlanArrays &out) {
  PlanCtx x(c, seeds, gens, S);
  if (x.d < 1 || x.tot >= UNSET || (x.NG && x.tot >= WRITER)) return x.refuse(PLAN_TOO_LARGE, 0);  // (a table word: the key below the writer bit)
  x.ctr = S.alloc<unsigned long long>(C_COUNT);
  if (!x.ctr) return x.fail("scratch", hipErrorOutOfMemory);
  for (int i = 0; i < C_COUNT; i++) x.h[i] = 0;
  x.h[C_BAD_SIGMA] = x.h[C_NO_PRODUCER] = x.h[C_JOIN_ONLY] = x.h[C_OTHER] = UINT64_MAX;
  if (!x.ok(hipMemcpyAsync(x.ctr, x.h, sizeof x.h, hipMemcpyHostToDevice, x.st), "scratch")) return P2GPU_E_DEVICE;
  if (int rc = x.decode()) return rc;
  if (int rc = x.copy_classes()) return rc;
  if (int rc = x.slots_ops()) return rc;
  if (int rc = x.levels()) return rc;
  if (int rc = x.unreached()) return rc;
  out.cell_slot = x.cell_slot; out.ops = x.ordered; out.level_off = x.level_off; out.gen_table = x.gen_table; out.n_gen_cells = gens.n_cells();
  out.levels = x.hres[S_LEVELS]; out.slots = x.slots; out.widest = x.hres[S_WIDEST]; out.n_ops = x.n_done;
  out.kind = hipMemcpyDeviceToDevice;
  return P2GPU_OK;
}

}  // namespace p2
