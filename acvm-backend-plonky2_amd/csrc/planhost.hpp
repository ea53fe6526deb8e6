// planhost.hpp -- the witness plan compiled on the host: plain C++ over five arrays, no HIP in it (g++ compiles it:
// csrc/tests/planhost_print.cpp, tests/test_witness_plan_host.py).  It is the statement of the plan's rules that the device
// compiler (genplan.hip) is compared with, and the one place where the refusals of both compilers are worded.
//   classes   sigma is decoded (sigma[x] = k_is[col'] * w^row': the coset of the value names col', the subgroup element
//             row'); the cycles become compact class ids.
//   slots     one value slot per class, and one per routed cell outside every class that a seed names or an op writes.
//   ops       the closed registry of genops.hpp, per slot / copy / row as DESIGN 6b lists them; an op none of whose
//             cells has a slot produces nothing (fill_witness derives such rows from zeros afterwards).
//   levels    level 0 = seeds, ConstantGate rows and ops without inputs; an op runs one level above its latest input.
//             The first op (by level, then creation order) that reaches a slot WRITES it -- its cell carries the
//             writer bit -- every other op that derives the same slot COMPARES, one level above the writer at least.
//             A BaseSum row runs in the direction the schedule reaches first.
//   generators that are no gate's own (PlanGenerator; the equality generator of plonky2's `is_equal` is the first): their
//             cells lie in other gates' rows, anywhere among the routed cells.
//             creation order  seeds, then the generators in list order, then the rows; a generator's op record is
//                             list index | (OP_EQUALITY | 0 << 8) << 32.
//             slots           classes, then seeds, then every cell a generator names that has no slot yet -- by (generator,
//                             cell position); a cell named again already has its slot -- then the rows.  So a row op created
//                             afterwards sees these cells as cells with a slot, and the inputs an op lists when it is created
//                             stay those that have a slot in the end.  A generator is always kept.  An input of a generator
//                             that nothing writes is an unreached slot: "a seed is missing", with that cell.
//             writer bits     a generator's live in ITS OWN table word (gen_table [generators][4]: cell key | bit 31), not in
//                             cell_slot, whose bit keeps meaning "the row op (or seed) that has this cell as an output writes
//                             it": a cell that is a generator's output and a row op's output has one writer.  A seed and a
//                             row op can name ONE cell as their output, and then share its bit: it is the seed's (a seed's slot
//                             is written in level 0, by this seed or by an earlier one of its class), the row op compares there
//                             (the walk knows such cells from the plan's seed list: witplan.hpp seed_out).  The level rule
//                             is unchanged: the first by (level, creation order) writes, every other op that derives the slot
//                             -- another generator, a seed, a row op -- compares, one level above at least.
//             refusals        before anything indexes with the cells: an unknown kind, a cell outside [n] x [R].
//             sizes           the generators count among the ops; a cell can be an input of a row op and of generators, so
//                             the `users` lists hold up to R n + (the generators' input cells) entries; a table word keeps the
//                             key in 31 bits.
//             any number of cells  a generator is a kind and a shape, the cell counts of its four groups (PlanGeneratorV); its
//                             cells follow each other in one flat list, and so do its table words: gen_off [generators + 1]
//                             names where a generator's begin.  Equality is the shape {1, 1, 1, 1}; the div-rem generator of
//                             `div_rem_biguint` has {la, lb, ld, lr}: the limbs of a and b (read), of div and rem (set); its
//                             op record is list index | OP_BIGUINT_DIVREM << 32.  The four nonnative generators (add, sub, mul, inv
//                             of `CircuitBuilderNonNative`) carry their field in bits 8-15 of the kind word and their shapes
//                             are stated at PLAN_GEN_NONNATIVE_ADD below; their op record is list index | (code | field << 8)
//                             << 32, the field where a row op keeps its operation index.  Every rule above holds per cell position: a
//                             slot named by several input positions is that many entries of its `users` list and as many
//                             counts of `pending`, hence one dependency; among the outputs the first position that names a
//                             slot may take the writer bit, every later position of the same slot compares.  Further
//                             refusals: a shape that is not the kind's, a cell count that is not the shapes' sum.
#pragma once
#include <algorithm>
#include <cstdio>
#include <string>
#include <unordered_map>
#include <vector>
#include "genops.hpp"
#include "gl.hpp"

namespace p2 {

constexpr uint32_t PLAN_UNSET = 0xFFFFFFFFu;   // cell without a slot
constexpr uint32_t PLAN_WRITER = 0x80000000u;  // cell_slot bit: this cell's op writes the slot (every other one compares)

struct PlanSeed {
  uint32_t row, col;
};

// a generator that is no gate's own: p2gpu.h's p2gpu_generator, word for word
constexpr uint32_t PLAN_GEN_EQUALITY = 0;  // cells: x, y (read), equal, inv (set)
constexpr uint32_t PLAN_GEN_CELLS = 4;
struct PlanGenerator {
  uint32_t kind;
  uint32_t cells[PLAN_GEN_CELLS][2];  // (row, col), routed columns only
};
// a generator with any number of cells: p2gpu.h's p2gpu_generator_v, word for word.  shape: the cell counts of its four groups
constexpr uint32_t PLAN_GEN_BIGUINT_DIVREM = 1;  // cells: a's limbs, b's (read), div's, rem's (set): shape {la, lb, ld, lr}
constexpr uint32_t PLAN_DIVREM_MAX_A = 32, PLAN_DIVREM_MAX_B = 16;  // bigdiv.hpp's arrays; 32 + 16 + 17 + 16 = 81 cells at most
// the four nonnative generators (plonky2_ecdsa/biguint/gadgets/nonnative.rs): the record's kind word is kind | field << 8, the
// field one of the two the reference instantiates (nonnative.hpp); a field element has PLAN_NONNATIVE_LIMBS limbs
//   add / sub  {la, lb, 8, 1}: a, b (read), sum or diff, overflow (set); an operand may have no limbs (`neg_nonnative`
//              subtracts from constant_biguint(0)), not both
//   mul        {la, lb, 8, la + lb - 8}: a, b (read), prod, overflow (set); la + lb < 8 underflows upstream
//   inv        {lx, 0, lx, lx}: x (read), inv, div (set)
constexpr uint32_t PLAN_GEN_NONNATIVE_ADD = 2, PLAN_GEN_NONNATIVE_SUB = 3, PLAN_GEN_NONNATIVE_MUL = 4, PLAN_GEN_NONNATIVE_INV = 5;
constexpr uint32_t PLAN_NONNATIVE_LIMBS = 8, PLAN_NONNATIVE_MAX = 16, PLAN_NONNATIVE_FIELDS = 2;
// the GLV decomposition generator (plonky2_ecdsa/curve/gadgets/glv.rs:117-149, :258-285): {lk, 0, 8, 2}, 1 <= lk <= 16: k's limbs
// (read), k1's four limbs then k2's four, k1_neg then k2_neg (set).  Its kind word takes no field.  Kind numbers 6 and 7 stay
// unknown kinds (reserved): the kind is 8, its op code the next one, OP_GLV_DECOMPOSE
constexpr uint32_t PLAN_GEN_GLV_DECOMPOSE = 8, PLAN_GLV_LIMBS = 4;
static_assert(OP_BIGUINT_DIVREM == OP_EQUALITY + PLAN_GEN_BIGUINT_DIVREM && OP_NONNATIVE_ADD == OP_EQUALITY + PLAN_GEN_NONNATIVE_ADD &&
                  OP_NONNATIVE_INV == OP_EQUALITY + PLAN_GEN_NONNATIVE_INV && OP_GLV_DECOMPOSE == OP_NONNATIVE_INV + 1,
              "PlanGenList::code: the listed kinds up to the nonnative ones and their op codes run in one order, the GLV kind's follows");
struct PlanGeneratorV {
  uint32_t kind;
  uint32_t shape[4];
};
// whether a record's kind word is a known one: the kind in bits 0-7, the field in bits 8-15 (the nonnative kinds only), nothing above
inline bool plan_generator_kind_ok(uint32_t word) {
  const uint32_t kind = word & 0xFF, field = (word >> 8) & 0xFF;
  if (word == PLAN_GEN_GLV_DECOMPOSE) return true;
  if (word >> 16 || kind > PLAN_GEN_NONNATIVE_INV) return false;
  return kind >= PLAN_GEN_NONNATIVE_ADD ? field < PLAN_NONNATIVE_FIELDS : field == 0;
}
// the checked list of either ABI: generator g owns the cells [off[g], off[g + 1]) of the flat list
struct PlanGenList {
  std::vector<PlanGeneratorV> gens;
  std::vector<uint32_t> off = {0};  // [gens + 1]
  std::vector<uint32_t> cells;      // (row, col) per cell
  size_t size() const { return gens.size(); }
  bool empty() const { return gens.empty(); }
  uint32_t n_cells() const { return off.back(); }
  uint32_t ins(size_t g) const { return gens[g].shape[0] + gens[g].shape[1]; }
  // the op record's code and the field beside it: code | field << 8 is the word behind the list index
  uint32_t code(size_t g) const { return gens[g].kind == PLAN_GEN_GLV_DECOMPOSE ? OP_GLV_DECOMPOSE : OP_EQUALITY + (gens[g].kind & 0xFF); }
  uint32_t field(size_t g) const { return gens[g].kind >> 8; }
  uint32_t code_word(size_t g) const { return code(g) | field(g) << 8; }
  // la | lb << 8 | ld << 16 | lr << 24: what the walk reads of a generator beside its table words
  uint32_t shape_word(size_t g) const { const uint32_t *s = gens[g].shape; return s[0] | s[1] << 8 | s[2] << 16 | s[3] << 24; }
  bool four_cells_each() const { return (size_t)n_cells() == PLAN_GEN_CELLS * gens.size(); }
};

// the circuit as both compilers read it
struct PlanInput {
  uint32_t d, R, W, ngc;
  const gl_t *sigma;        // [R][n]
  const gl_t *gconsts;      // [ngc][n]
  const uint8_t *row_gate;  // [n]
  const GateDesc *gates;
  const gl_t *k_is;         // [R]
};

// cell_slot [R][n]; ops by (level, creation order), one 64-bit word each: row | (code | sub << 8) << 32 (OP_SEED: the seed's
// index for the row, OP_EQUALITY .. OP_GLV_DECOMPOSE: the generator's, sub the field); level_off [levels + 1]; gen_off [generators + 1] and
// gen_table [gen_off[generators]], one word per cell a generator names: cell key (col << d | row) | PLAN_WRITER = this naming
// writes the cell's slot (four words per generator when all are equality generators: [generators][4])
struct HostPlan {
  std::vector<uint32_t> cell_slot, level_off, gen_table, gen_off;
  std::vector<uint64_t> ops;
  uint32_t levels = 0, slots = 0, widest = 0;
};

enum PlanRefusalKind { PLAN_OK = 0, PLAN_SEED_OUTSIDE, PLAN_SEED_TWICE, PLAN_BAD_SIGMA, PLAN_TOO_LARGE, PLAN_SEED_MISSING, PLAN_CYCLE, PLAN_GEN_KIND, PLAN_GEN_OUTSIDE,
                       PLAN_GEN_NULL, PLAN_GEN_SHAPE, PLAN_GEN_COUNT, PLAN_GEN_FEW, PLAN_GEN_CELLS_NULL };

// why a plan is refused: the cell, and for the seed checks the seeds that name it (the generator checks: seed = the generator's
// index, seed2 = its kind, shape = its shape; the cell count: row = what the shapes name, col = what is given)
struct PlanRefusal {
  PlanRefusalKind kind = PLAN_OK;
  uint64_t row = 0, col = 0;
  size_t seed = 0, seed2 = 0;
  uint32_t shape[4] = {0, 0, 0, 0};
  explicit operator bool() const { return kind != PLAN_OK; }
  // a cell by its key, col << d | row
  static PlanRefusal at(PlanRefusalKind kind, uint64_t key, uint32_t d) {
    PlanRefusal r;
    r.kind = kind; r.row = key & (((uint64_t)1 << d) - 1); r.col = key >> d;
    return r;
  }
};

// p2gpu_last_error's text of a refusal of a circuit with 2^d rows and W wires, R of them routed
inline std::string plan_refusal_text(const PlanRefusal &r, uint32_t d, uint32_t W, uint32_t R = 0) {
  char buf[256];
  const unsigned long long row = r.row, col = r.col;
  switch (r.kind) {
  case PLAN_SEED_OUTSIDE:
    snprintf(buf, sizeof buf, "seed %zu names cell (row %llu, column %llu) outside the %zu x %u wire matrix", r.seed, row, col, (size_t)1 << d, W);
    break;
  case PLAN_SEED_TWICE: snprintf(buf, sizeof buf, "cell (row %llu, column %llu) is seeded twice (seeds %zu and %zu)", row, col, r.seed, r.seed2); break;
  case PLAN_BAD_SIGMA:
    snprintf(buf, sizeof buf, "p2gpu_witness_plan_create: sigma of cell (row %llu, column %llu) names no routed cell", row, col);
    break;
  case PLAN_TOO_LARGE: snprintf(buf, sizeof buf, "p2gpu_witness_plan_create: circuit too large"); break;
  case PLAN_SEED_MISSING:
    snprintf(buf, sizeof buf, "no seed, constant or generator reaches the copy class of cell (row %llu, column %llu): a seed is missing", row, col);
    break;
  case PLAN_CYCLE:
    snprintf(buf, sizeof buf, "dependency cycle: the generator that derives cell (row %llu, column %llu) waits for its own output", row, col);
    break;
  case PLAN_GEN_KIND: snprintf(buf, sizeof buf, "generator %zu has the unknown kind %zu", r.seed, r.seed2); break;
  case PLAN_GEN_OUTSIDE:
    snprintf(buf, sizeof buf, "generator %zu names cell (row %llu, column %llu) outside the %zu x %u routed cells", r.seed, row, col, (size_t)1 << d, R);
    break;
  case PLAN_GEN_NULL: snprintf(buf, sizeof buf, "generators are counted but the list is a null pointer"); break;
  case PLAN_GEN_SHAPE:
    snprintf(buf, sizeof buf, "generator %zu of kind %zu has the shape {%u, %u, %u, %u}, which is not a shape of its kind", r.seed, r.seed2, r.shape[0],
             r.shape[1], r.shape[2], r.shape[3]);
    break;
  case PLAN_GEN_COUNT: snprintf(buf, sizeof buf, "the generators' shapes name %llu cells, %llu are given", row, col); break;
  case PLAN_GEN_FEW:
    snprintf(buf, sizeof buf, "the shapes of the generators up to generator %zu name %llu cells, %llu are given", r.seed, row, col);
    break;
  case PLAN_GEN_CELLS_NULL: snprintf(buf, sizeof buf, "generator cells are counted but the list is a null pointer"); break;
  default: buf[0] = 0; break;
  }
  return buf;
}

// the seed checks of both compilers: every seed inside the matrix, no cell twice.  seed_cells: (row, col) pairs
inline PlanRefusal plan_seeds(uint32_t d, uint32_t W, const uint32_t *seed_cells, size_t n_seeds, std::vector<PlanSeed> &out) {
  const size_t n = (size_t)1 << d;
  std::unordered_map<uint64_t, size_t> seen;
  for (size_t i = 0; i < n_seeds; i++) {
    const uint32_t row = seed_cells[2 * i], col = seed_cells[2 * i + 1];
    PlanRefusal r;
    r.row = row; r.col = col; r.seed = r.seed2 = i;
    if (row >= n || col >= W) {
      r.kind = PLAN_SEED_OUTSIDE;
      return r;
    }
    if (!seen.emplace(((uint64_t)row << 32) | col, i).second) {
      r.kind = PLAN_SEED_TWICE;
      r.seed = seen[((uint64_t)row << 32) | col];
      return r;
    }
    out.push_back(PlanSeed{row, col});
  }
  return PlanRefusal();
}

// whether `shape` is one of the kind of the kind word `word` (a known one)
inline bool plan_generator_shape_ok(uint32_t word, const uint32_t shape[4]) {
  const uint32_t kind = word & 0xFF, la = shape[0], lb = shape[1], ld = shape[2], lr = shape[3];
  const uint32_t L = PLAN_NONNATIVE_LIMBS, MAX = PLAN_NONNATIVE_MAX;
  if (kind == PLAN_GEN_EQUALITY) return la == 1 && lb == 1 && ld == 1 && lr == 1;
  if (kind == PLAN_GEN_NONNATIVE_ADD || kind == PLAN_GEN_NONNATIVE_SUB) return la <= MAX && lb <= MAX && la + lb >= 1 && ld == L && lr == 1;
  if (kind == PLAN_GEN_NONNATIVE_MUL) return la <= MAX && lb <= MAX && la + lb >= L && ld == L && lr == la + lb - L;
  if (kind == PLAN_GEN_NONNATIVE_INV) return la >= 1 && la <= MAX && lb == 0 && ld == la && lr == la;
  if (kind == PLAN_GEN_GLV_DECOMPOSE) return la >= 1 && la <= MAX && lb == 0 && ld == 2 * PLAN_GLV_LIMBS && lr == 2;
  // div_rem_biguint (biguint.rs:236-244): rem has b's limbs, div a_len - b_len + 1, or none when b_len > a_len + 1
  return la >= 1 && la <= PLAN_DIVREM_MAX_A && lb >= 1 && lb <= PLAN_DIVREM_MAX_B && lr == lb && ld == (lb > la + 1 ? 0 : la - lb + 1);
}

// the generator checks of both compilers, generator by generator: a known kind, a shape of that kind, its cells inside the
// list and every one a routed cell; then no cell left over.  Nothing indexes with a cell before this.  cells: (row, col) pairs
inline PlanRefusal plan_generators_v(uint32_t d, uint32_t R, const PlanGeneratorV *gens, size_t n_gens, const uint32_t *cells, size_t n_cells,
                                     PlanGenList &out) {
  const size_t n = (size_t)1 << d;
  PlanRefusal r;
  if (n_gens && !gens) {
    r.kind = PLAN_GEN_NULL;
    return r;
  }
  if (n_cells && !cells) {
    r.kind = PLAN_GEN_CELLS_NULL;
    return r;
  }
  size_t at = 0;
  for (size_t i = 0; i < n_gens; i++) {
    r.seed = i; r.seed2 = gens[i].kind;
    if (!plan_generator_kind_ok(gens[i].kind)) {
      r.kind = PLAN_GEN_KIND;
      return r;
    }
    for (int k = 0; k < 4; k++) r.shape[k] = gens[i].shape[k];
    if (!plan_generator_shape_ok(gens[i].kind, gens[i].shape)) {
      r.kind = PLAN_GEN_SHAPE;
      return r;
    }
    const size_t count = (size_t)gens[i].shape[0] + gens[i].shape[1] + gens[i].shape[2] + gens[i].shape[3];
    if (count > n_cells - at) {  // too few cells: the refusal counts the generators checked so far, this one included
      r.kind = PLAN_GEN_FEW; r.row = at + count; r.col = n_cells;
      return r;
    }
    for (size_t k = 0; k < count; k++) {
      r.row = cells[2 * (at + k)]; r.col = cells[2 * (at + k) + 1];
      if (r.row >= n || r.col >= R) {
        r.kind = PLAN_GEN_OUTSIDE;
        return r;
      }
    }
    at += count;
    out.gens.push_back(gens[i]);
    out.off.push_back((uint32_t)at);
  }
  if (at != n_cells) {
    r.kind = PLAN_GEN_COUNT; r.row = at; r.col = n_cells;
    return r;
  }
  out.cells.assign(cells, cells + 2 * n_cells);
  return PlanRefusal();
}

// the list of four-cell records (p2gpu_generator): the case of shapes {1, 1, 1, 1}.  The record form knows the equality
// generator only, as it always did: any other kind is an unknown one here
inline PlanRefusal plan_generators(uint32_t d, uint32_t R, const PlanGenerator *gens, size_t n_gens, PlanGenList &out) {
  if (n_gens && !gens) {
    PlanRefusal r;
    r.kind = PLAN_GEN_NULL;
    return r;
  }
  // (in list order, as the checks below: a generator's kind is looked at before the cells of the ones behind it)
  size_t known = 0;
  while (known < n_gens && gens[known].kind == PLAN_GEN_EQUALITY) known++;
  if (known < n_gens) {
    PlanGenList head;
    if (PlanRefusal r = plan_generators(d, R, gens, known, head)) return r;
    PlanRefusal r;
    r.kind = PLAN_GEN_KIND; r.seed = known; r.seed2 = gens[known].kind;
    return r;
  }
  std::vector<PlanGeneratorV> v(n_gens);
  std::vector<uint32_t> cells(2 * PLAN_GEN_CELLS * n_gens);
  for (size_t i = 0; i < n_gens; i++) {
    v[i] = PlanGeneratorV{gens[i].kind, {1, 1, 1, 1}};
    for (uint32_t k = 0; k < PLAN_GEN_CELLS; k++) {
      cells[2 * (PLAN_GEN_CELLS * i + k)] = gens[i].cells[k][0];
      cells[2 * (PLAN_GEN_CELLS * i + k) + 1] = gens[i].cells[k][1];
    }
  }
  return plan_generators_v(d, R, v.data(), n_gens, cells.data(), PLAN_GEN_CELLS * n_gens, out);
}

namespace planhost {

constexpr uint32_t UNSET = PLAN_UNSET, WRITER = PLAN_WRITER;

struct HostOp {
  uint32_t code, row, sub;        // row: the seed's / the generator's index for those
  uint32_t in0, in1, out0, out1;  // ranges in Compiler::cells
  uint32_t pending = 0, twin = UNSET;
  int level = -1;
  bool dead = false;
};

struct Compiler {
  const PlanInput &c;
  size_t n;
  uint32_t R, d, ngc;
  std::vector<uint32_t> cell_slot;  // [R][n]; classes first, then the lone cells
  std::vector<uint32_t> cells;      // input / output cells of the ops, by key: an op's cells need not lie in one row
  std::vector<uint32_t> gen_table;  // one word per cell a generator names, in list order
  const uint32_t *gen_off = nullptr;  // the list's offsets into it
  std::vector<HostOp> ops;
  uint32_t slots = 0;

  explicit Compiler(const PlanInput &in) : c(in), n((size_t)1 << in.d), R(in.R), d(in.d), ngc(in.ngc) {}

  size_t key(uint32_t row, uint32_t col) const { return ((size_t)col << d) + row; }

  // sigma -> class ids of the cells on a cycle of length > 1
  PlanRefusal classes() {
    gl_t w = GL_ROOT_2_32;
    for (uint32_t i = d; i < 32; i++) w = gl_sqr(w);
    std::vector<gl_t> wp(n);
    std::unordered_map<gl_t, uint32_t> row_of, col_of;
    row_of.reserve(2 * n);
    gl_t x = 1;
    for (size_t r = 0; r < n; r++, x = gl_mul(x, w)) wp[r] = x, row_of[x] = (uint32_t)r;
    std::vector<gl_t> kinv(R);
    for (uint32_t col = 0; col < R; col++) {
      gl_t t = c.k_is[col];
      for (uint32_t i = 0; i < d; i++) t = gl_sqr(t);
      col_of[t] = col;
      kinv[col] = gl_inv(c.k_is[col]);
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
        const gl_t s = c.sigma[key(row, col)];
        if (s == gl_mul(c.k_is[col], wp[row])) continue;
        gl_t t = s;
        for (uint32_t i = 0; i < d; i++) t = gl_sqr(t);
        const auto ci = col_of.find(t);
        const auto ri = ci == col_of.end() ? row_of.end() : row_of.find(gl_mul(s, kinv[ci->second]));
        if (s >= GL_P || ri == row_of.end()) return PlanRefusal::at(PLAN_BAD_SIGMA, key(row, col), d);
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
    return PlanRefusal();
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
    op.in0 = (uint32_t)cells.size();
    for_cols(oc.in, [&](uint32_t col) { if (col < R && cell_slot[key(row, col)] != UNSET) cells.push_back((uint32_t)key(row, col)); });  // a cell without a slot reads as zero
    op.in1 = op.out0 = (uint32_t)cells.size();
    for_cols(oc.out, [&](uint32_t col) {
      if (col >= R) return;
      uint32_t &s = cell_slot[key(row, col)];
      if (s == UNSET) s = slots++;
      cells.push_back((uint32_t)key(row, col));
    });
    op.out1 = (uint32_t)cells.size();
    ops.push_back(op);
    return (uint32_t)ops.size() - 1;
  }

  void row_ops(uint32_t row) {
    const GateDesc &g = c.gates[c.row_gate[row]];
    auto LC = [&](uint32_t i) { return i < ngc ? c.gconsts[(size_t)i * n + row] : (gl_t)0; };
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
  // seeds first, then the generators, then the rows in order; levels; what the schedule did not reach.  order: the ops by
  // (level, creation order)
  PlanRefusal schedule(const std::vector<PlanSeed> &seeds, const PlanGenList &gens, std::vector<uint32_t> &order,
                       std::vector<uint32_t> &level_off) {
    const size_t tot = (size_t)R * n;
    if (!gens.empty() && tot >= WRITER) {  // (a table word keeps the key below its writer bit)
      PlanRefusal r;
      r.kind = PLAN_TOO_LARGE;
      return r;
    }
    // ---- ops: seeds first, then the generators, then the rows in order ----
    for (size_t i = 0; i < seeds.size(); i++) {
      const PlanSeed cell = seeds[i];
      HostOp op;
      op.code = OP_SEED; op.row = (uint32_t)i; op.sub = 0;
      op.in0 = op.in1 = op.out0 = (uint32_t)cells.size();
      if (cell.col < R) {
        uint32_t &s = cell_slot[key(cell.row, cell.col)];
        if (s == UNSET) s = slots++;
        cells.push_back((uint32_t)key(cell.row, cell.col));
      }
      op.out1 = (uint32_t)cells.size();
      ops.push_back(op);
    }
    gen_off = gens.off.data();
    for (size_t i = 0; i < gens.size(); i++) {
      HostOp op;
      op.code = gens.code(i); op.row = (uint32_t)i; op.sub = gens.field(i);
      op.in0 = (uint32_t)cells.size();
      for (uint32_t e = gens.off[i]; e < gens.off[i + 1]; e++) {
        const uint32_t v = (uint32_t)key(gens.cells[2 * (size_t)e], gens.cells[2 * (size_t)e + 1]);
        if (cell_slot[v] == UNSET) cell_slot[v] = slots++;
        cells.push_back(v);
        gen_table.push_back(v);
      }
      op.in1 = op.out0 = op.in0 + gens.ins(i);
      op.out1 = (uint32_t)cells.size();
      ops.push_back(op);
    }
    for (size_t row = 0; row < n; row++) row_ops((uint32_t)row);
    if (slots >= WRITER || ops.size() >= ((size_t)1 << 32)) {
      PlanRefusal r;
      r.kind = PLAN_TOO_LARGE;
      return r;
    }
    // ---- levels ----
    auto slot_of = [&](const HostOp &, uint32_t k) -> uint32_t & { return cell_slot[cells[k]]; };
    // where op o keeps the writer bit of its output cell k: a generator in its table word, every other op in cell_slot
    auto writer_word = [&](const HostOp &o, uint32_t k) -> uint32_t & {
      return op_is_listed_generator(o.code) ? gen_table[(size_t)gen_off[o.row] + (k - o.in0)] : cell_slot[cells[k]];
    };
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
          const uint32_t s = slot_of(o, k) & ~WRITER;
          if (slot_level[s] < 0) { slot_level[s] = lvl; fresh.push_back(s); writer_word(o, k) |= WRITER; }
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
    if (stuck != SIZE_MAX) return PlanRefusal::at(PLAN_SEED_MISSING, stuck, d);
    if (cyc != SIZE_MAX) return PlanRefusal::at(PLAN_CYCLE, cyc, d);
    return PlanRefusal();
  }
};

}  // namespace planhost

// the plan of circuit `in` for `seeds` (already through plan_seeds) and `gens` (already through plan_generators)
inline PlanRefusal plan_compile_host(const PlanInput &in, const std::vector<PlanSeed> &seeds, const PlanGenList &gens, HostPlan &out) {
  planhost::Compiler K(in);
  if (PlanRefusal r = K.classes()) return r;
  std::vector<uint32_t> order;
  if (PlanRefusal r = K.schedule(seeds, gens, order, out.level_off)) return r;
  out.ops.clear();
  out.ops.reserve(order.size());
  for (uint32_t i : order) out.ops.push_back((uint64_t)K.ops[i].row | ((uint64_t)(K.ops[i].code | (K.ops[i].sub << 8)) << 32));
  out.cell_slot.swap(K.cell_slot);
  out.gen_table.swap(K.gen_table);
  out.gen_off = gens.off;
  out.levels = (uint32_t)out.level_off.size() - 1;
  out.slots = K.slots;
  out.widest = 0;
  for (uint32_t l = 0; l < out.levels; l++) out.widest = std::max(out.widest, out.level_off[l + 1] - out.level_off[l]);
  return PlanRefusal();
}

}  // namespace p2
