/*
 * p2gpu.h -- C ABI of libp2gpu.so: the MI355X (gfx950) implementation of the
 * `prove` hot path of eryxcoop/acvm-backend-plonky2.
 *
 * What each entry point replaces in the reference (there is no FFI today; the
 * seam is a Rust method call into the plonky2 crate):
 *
 *   p2gpu_circuit_create   <- the prover-side part of `builder.build::<C>()`
 *                             plonky2-backend/src/circuit_translation/mod.rs:80-82
 *                             (constants/sigmas LDE + Merkle tree, root tables,
 *                             circuit digest), once per circuit
 *   p2gpu_prove            <- `circuit_data.prove(witnesses).unwrap()`
 *                             plonky2-backend/src/actions/prove_action.rs:91-97,
 *                             after witness generation (input = full wire matrix)
 *   p2gpu_prove_dev        <- same, wire matrix already resident in HBM
 *   p2gpu_prove_sparse     <- same as p2gpu_prove for a witness whose unused wires are given as one value each
 *   p2gpu_fill_witness / p2gpu_prove_routed
 *                          <- the row-local tail of `generate_partial_witness`: the gates' own
 *                             SimpleGenerators (e.g. arithmetic_u32.rs:376-426)
 *   p2gpu_witness_plan_create / p2gpu_witness_plan_build / p2gpu_generate_witness / p2gpu_prove_seeds
 *                          <- all of `generate_partial_witness` (plonky2 iop/generator.rs, called by `prove`): the caller
 *                             hands over the `pw.set_target` values only, generators and copy constraints run on the GPU
 *   p2gpu_witness_plan_create_gen / p2gpu_witness_plan_build_gen
 *                          <- the same plans for a circuit that holds generators which are no gate's own: the
 *                             EqualityGenerators of `builder.is_equal` (gadgets/arithmetic.rs), which the memory writes of
 *                             the ACIR translation are made of (circuit_translation/memory_translator.rs:89-112)
 *   p2gpu_witness_plan_create_genv / p2gpu_witness_plan_build_genv
 *                          <- the same with generators of any number of cells: the BigUintDivRemGenerator of
 *                             `div_rem_biguint` (plonky2_ecdsa/biguint/biguint.rs:231-262, :317-344), whose cells are limbs
 *   p2gpu_generate_witness_batch
 *                          <- the same for many value sets of one circuit at once (the reference has no counterpart: it
 *                             calls `prove` once per witness)
 *   p2gpu_prove_batch_dev / p2gpu_prove_seeds_batch
 *                          <- `circuit_data.prove(witnesses)` for many witnesses of one small circuit (degree_bits <=
 *                             P2GPU_PROVE_BATCH_MAX_DEGREE_BITS) in one call: the reference calls `prove` once per witness and so
 *                             does p2gpu_prove_dev; here every launch covers a slab of proofs and the transcripts run on the GPU
 *   p2gpu_check_witness / p2gpu_check_witness_dev / p2gpu_check_seeds
 *                          <- the panic of plonky2's witness generator that names a partition (iop/generator.rs), for a matrix
 *                             that arrives complete: which gate row and which copy constraint a witness breaks
 *   p2gpu_last_error       <- the `anyhow::Error` text the reference unwraps
 *   p2gpu_ifft_batch / p2gpu_lde_batch / p2gpu_commit_values
 *                          <- plonky2 PolynomialValues::ifft,
 *                             PolynomialCoeffs::lde+coset_fft,
 *                             PolynomialBatch::from_values (stage-level operators)
 *
 * Conventions: plain C, little-endian, field elements are canonical u64 < p =
 * 2^64 - 2^32 + 1.  Return 0 = ok, < 0 = error (see P2GPU_E_*); no exception or
 * abort crosses the ABI.  The caller owns every host buffer; the library owns
 * device memory until p2gpu_circuit_destroy.  One in-flight prove per circuit
 * handle; distinct handles may be used from distinct threads.
 *
 * ---------------------------------------------------------------------------
 * Circuit blob (version 1), written once per circuit by the Rust side from
 * CommonCircuitData + ProverOnlyCircuitData:
 *
 *   u32 header[64]:
 *     [0] magic 0x43473250 "P2GC"   [1] version = 1      [2] degree_bits d
 *     [3] num_wires                 [4] num_routed_wires  [5] num_constants (selector + gate-constant columns)
 *     [6] num_selectors             [7] num_challenges    [8] quotient_degree_factor
 *     [9] rate_bits                 [10] cap_height       [11] proof_of_work_bits
 *     [12] num_query_rounds         [13] number of FRI reduction steps
 *     [14..21] reduction_arity_bits [22] hasher: 0 = KeccakHash<25> (the reference's KeccakGoldilocksConfig),
 *                                        1 = PoseidonHash (PoseidonGoldilocksConfig: Poseidon Merkle trees,
 *                                        challenger and circuit digest; digests are 4 field elements = 32 bytes)
 *     [23] num_gates                [24] num_public_inputs
 *     [25] flags: bit0 = circuit_digest present, bit1 = constants_sigmas_cap present
 *     [26] num_partial_products     [32..39] circuit_digest (25 bytes used)
 *   u32 gate[num_gates][12]  in `common.gates` order:
 *     kind, p0, p1, p2, p3, selector_index, group_start, group_end,
 *     num_constraints, degree, num_constants, reserved
 *   (flag bit1) u8 cap[2^cap_height][32]   expected constants_sigmas cap (25 bytes used)
 *   u64 k_is[num_routed_wires]
 *   u64 constants[num_constants][n]        values over the subgroup, column-major
 *   u64 sigmas[num_routed_wires][n]
 *
 * Gate kinds (closed registry, plonky2-backend/src/actions/write_vk_action.rs:35-62):
 *   0 Noop  1 Constant{p0=num_consts}  2 PublicInput  3 Arithmetic{p0=num_ops}
 *   4 BaseSum{p0=B,p1=num_limbs}  5 RandomAccess{p0=bits,p1=copies,p2=extra_consts}
 *   6 Poseidon (PoseidonGate, width 12)  7 U32Arithmetic{p0=num_ops}
 *   8 U32AddMany{p0=num_addends 0..16,p1=num_ops}  9 U32Subtraction{p0=num_ops}
 *   10 U32RangeCheck{p0=num_input_limbs}  11 Comparison{p0=num_bits,p1=num_chunks}
 *
 * Proof bytes: plonky2's uncompressed ProofWithPublicInputs::to_bytes layout
 * (SURVEY.md C.11).  Compression (prove_action.rs:75-78) stays in Rust.
 */
#ifndef P2GPU_H
#define P2GPU_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define P2GPU_OK 0
#define P2GPU_E_BLOB -1               /* malformed / unsupported circuit blob */
#define P2GPU_E_BUFFER -2             /* output buffer too small (proof_len holds the size needed) */
#define P2GPU_E_DEVICE -3             /* HIP error; see p2gpu_last_error */
#define P2GPU_E_OPENING_IN_SUBGROUP -4 /* zeta^n == 1 ("Opening point is in the subgroup.") */
#define P2GPU_E_UNSATISFIED -5        /* witness does not satisfy the circuit (self-check failed) */
#define P2GPU_E_CAP_MISMATCH -6       /* constants_sigmas cap differs from the one in the blob */
#define P2GPU_E_ARG -7
#define P2GPU_E_NOT_INIT -8
#define P2GPU_E_VERIFY -9             /* p2gpu_verify: the proof is not valid for this circuit */

typedef struct p2gpu_circuit p2gpu_circuit;

/* per-phase device time of the last proof (milliseconds, HIP events), phase
 * names follow plonky2's TimingTree labels */
typedef struct {
  double wires_commit_ms;    /* "compute wires commitment" */
  double zs_commit_ms;       /* "compute partial products" + commit */
  double quotient_ms;        /* "compute quotient polys" + commit */
  double openings_ms;        /* "construct the opening set" */
  double fri_ms;             /* "compute opening proofs" */
  double total_ms;           /* entry -> proof bytes on host */
  double h2d_ms;             /* wire matrix upload (0 for p2gpu_prove_dev) */
  uint64_t pow_witness;
} p2gpu_timings;

/* Select the device(s) of this process.  One id (or NULL = {device 0}): one process per GPU -- replicas, or the ranks of a
 * proof sharded over processes (p2gpu_circuit_set_shard*).  Several ids (at most 8, repeats allowed): THIS process drives
 * them all; every handle created afterwards is a device group and each prove call is ONE proof coset-sharded over the
 * group from threads inside the call (the shape `circuit_data.prove(pw)`, prove_action.rs:96, can call).  Out-of-range
 * ids or more than 8: P2GPU_E_ARG. */
int p2gpu_init(const int *device_ids, int n_devices);
/* Page-locked ("pinned") host memory for the wire matrix handed to p2gpu_prove / _routed / _sparse -- what the caller
 * would otherwise hold in a Vec<F> (the witness the reference builds before prove_action.rs:96).  Uploads from it are
 * direct DMA and do not occupy the calling thread; any other host pointer still works (the HIP runtime stages it).
 * NULL on failure (p2gpu_last_error). */
void *p2gpu_host_alloc(size_t bytes);
void p2gpu_host_free(void *p);

int p2gpu_circuit_create(const uint8_t *blob, size_t len, p2gpu_circuit **out);
/* The same on ONE named device of the p2gpu_init list -- a plain handle even when the list has several ids (then
 * p2gpu_circuit_create makes device groups): replicas across the GPUs of a node from one process, one host thread per handle.
 * (Counterpart: the same `circuit_data.prove` call, prove_action.rs:96, issued once per device.) */
int p2gpu_circuit_create_on(const uint8_t *blob, size_t len, int device_id, p2gpu_circuit **out);
void p2gpu_circuit_destroy(p2gpu_circuit *c);
/* bytes of one digest of this circuit's hasher: 25 (KeccakHash<25>) or 32 (PoseidonHash) */
int p2gpu_circuit_hash_bytes(const p2gpu_circuit *c);
/* 2^cap_height x hash_bytes */
int p2gpu_circuit_cap(const p2gpu_circuit *c, uint8_t *out);
/* hash_bytes */
int p2gpu_circuit_digest(const p2gpu_circuit *c, uint8_t *out);
/* HIP device index the handle lives on (< 0: verifier-only handle / bad argument) */
int p2gpu_circuit_device(const p2gpu_circuit *c);
/* The size in bytes of every proof of this circuit: a proof's length is fixed by its circuit (the value p2gpu_verify
 * asks of a proof), so a buffer of this size always suffices and a shorter one is refused with P2GPU_E_BUFFER. */
size_t p2gpu_proof_size_bound(const p2gpu_circuit *c);

/* wires: host pointer, [num_wires][n] column-major.  proof_len: in = capacity,
 * out = bytes used.  pow_hint: UINT64_MAX = grind for the minimum witness. */
int p2gpu_prove(p2gpu_circuit *c, const uint64_t *wires, const uint64_t *public_inputs, uint32_t n_pi,
                uint8_t *proof_out, size_t *proof_len, p2gpu_timings *opt_timings);
/* same, `wires_dev` is a device pointer (e.g. torch tensor data_ptr) on the
 * circuit's device; it is only read. */
int p2gpu_prove_dev(p2gpu_circuit *c, const uint64_t *wires_dev, const uint64_t *public_inputs, uint32_t n_pi,
                    uint8_t *proof_out, size_t *proof_len, p2gpu_timings *opt_timings);
/* ---- a batch of witnesses of one small circuit, proved in one call ----
 * A second, plain prover (csrc/provebatch.hip, csrc/provebatchcore.hpp) whose every launch covers a slab of proofs: each
 * proof's challenges, zeta, FRI betas, proof-of-work witness and query indices stay in device memory, the Fiat-Shamir transcript
 * runs on the device with one lane per proof, and the host synchronises once per slab -- a lone proof costs eleven round trips
 * and ~55 launches whatever its size, which is all a circuit of 2^2 .. 2^12 gates costs.  The number of launches per slab does
 * not depend on the batch (p2gpu_prove_batch_info).
 *   wires_dev      device, [batch][num_wires][n]: the layout of p2gpu_generate_witness_batch; only read
 *   public_inputs  host, [batch][n_pi]
 *   proofs_out     host, [batch][p2gpu_proof_size_bound(c)]
 *   status         host, [batch]: the code p2gpu_prove_dev returns for that matrix and those public inputs on this handle --
 *                  P2GPU_OK, P2GPU_E_UNSATISFIED (knob "self_check" at its default 1: the verifier's identity at zeta, checked per
 *                  proof on the device; with 0 the proof is emitted anyway, like the lone call) or P2GPU_E_OPENING_IN_SUBGROUP
 * Where status[b] is P2GPU_OK, proofs_out[b] holds exactly the bytes p2gpu_prove_dev writes, the minimal proof-of-work witness
 * included; the bytes of a failing member are zero.  Members do not affect each other.  Returns P2GPU_OK when every member is
 * good, otherwise the code of the lowest failing member, p2gpu_last_error reading "witness <b> of the batch: " and the lone
 * call's words.  P2GPU_E_ARG, decided before any device call and worded in p2gpu_last_error: a null handle, matrix, output or
 * status; batch == 0; n_pi different from the circuit's, or a public input >= p; a verifier-only handle; a device group or a
 * handle with sharding configured; degree_bits > P2GPU_PROVE_BATCH_MAX_DEGREE_BITS (a column of 2^12 elements is transformed by
 * one workgroup in LDS; above that the tuned lone path takes over: p2gpu_prove_dev).
 * MEASURED (profiles/prove_batch.md, one MI355X, 256 witnesses of the `arith` mix): 16x the lone-call loop and 4.5x four proofs in
 * flight at 2^3 gates, 10x and 3.0x at 2^10; at degree_bits 12 it still beats the loop (2.2x) but loses to four lone proofs in
 * flight on four handles (0.75x).  Do not use it above degree_bits 10 where four handles can be kept busy (11 is not measured).
 * Both hashers.  The "pow_hint" knob is not consulted: the batch always grinds for the minimum.  "half_gates", "zero_columns"
 * and "virtual_columns" have nothing to act on here.  The call works in slabs of proofs: as many as a byte budget
 * (SLAB_BUDGET_BYTES in csrc/provebatch.hip) and three quarters of the free device memory hold, or the knob "prove_batch_slab"
 * (proofs per slab, 0 = automatic).  The slab's buffers stay on the handle, grow to the largest slab seen and are freed by
 * p2gpu_circuit_destroy; a handle that never makes the call allocates nothing.  One call per handle at a time, as for every
 * entry point; other handles may prove beside it. */
#define P2GPU_PROVE_BATCH_MAX_DEGREE_BITS 12
int p2gpu_prove_batch_dev(p2gpu_circuit *c, const uint64_t *wires_dev, size_t batch, const uint64_t *public_inputs, uint32_t n_pi,
                          uint8_t *proofs_out, int *status);
/* the limit the library enforces (= P2GPU_PROVE_BATCH_MAX_DEGREE_BITS of the header it was built from) */
uint32_t p2gpu_prove_batch_max_degree_bits(void);
/* out: launches of the last slab, proofs in it, bytes of the slab buffers the handle holds, the byte budget.  Zeros before the
 * first call (and for a verifier-only handle). */
int p2gpu_prove_batch_info(const p2gpu_circuit *c, uint64_t out[4]);

/* Row-local witness generators on the GPU (the reference's SimpleGenerator
 * impls: arithmetic_u32.rs:376-426, add_many_u32.rs:329-378, subtraction_u32.rs:298-343,
 * range_check_u32.rs:198-220, comparison.rs:439-537 + the stock gates'): given a device wire
 * matrix whose gate INPUT wires are set (i.e. after copy-constraint propagation), derive every
 * other wire of each row in place. */
int p2gpu_fill_witness(p2gpu_circuit *c, uint64_t *wires_dev);
/* prove from the ROUTED columns only (host, [num_routed_wires][n]): the non-routed columns are
 * all gate-internal, so they are filled on the GPU instead of crossing PCIe (80 of 234 columns). */
int p2gpu_prove_routed(p2gpu_circuit *c, const uint64_t *routed, const uint64_t *public_inputs, uint32_t n_pi,
                       uint8_t *proof_out, size_t *proof_len, p2gpu_timings *opt_timings);
/* prove from the first `ncols` wire columns (host, [ncols][n]) plus ONE value for each of the others: column
 * j >= ncols is zero in every row but `row`, where it holds tail[j - ncols].  That is what plonky2 leaves in the
 * wires no gate of a circuit uses (circuit_builder.rs randomize_unused_pi_wires: one random value in the
 * PublicInputGate row; 154 of the 234 wires of wide_ecc_config in circuits without ECC gates,
 * circuit_translation/mod.rs:69), so a caller that knows its circuit ships 84 MB instead of 245 MB at 2^17
 * gates.  The columns are written in HBM and the proof is byte-identical to p2gpu_prove on the full matrix --
 * any ncols <= num_wires and any row work (the library classifies the columns it is given, it does not trust
 * the split); tail may be NULL when ncols == num_wires. */
int p2gpu_prove_sparse(p2gpu_circuit *c, const uint64_t *wires, uint32_t ncols, const uint64_t *tail, uint32_t row,
                       const uint64_t *public_inputs, uint32_t n_pi, uint8_t *proof_out, size_t *proof_len,
                       p2gpu_timings *opt_timings);

/* ---- the witness from the solver's values (`generate_partial_witness`, iop/generator.rs) ----
 * A plan is made once per circuit and seed set.  Seeds are the cells whose values the caller supplies per proof -- what the
 * Rust side passes to `pw.set_target` -- as (row, col) with col < num_wires; a seed on a gate-internal column or on a cell
 * outside every copy class is simply written (the PublicInputGate row's random wires arrive that way).  From the handle's sigma
 * polynomials the plan takes the copy classes of the routed cells, from its gate rows the generators (the closed registry
 * p2gpu_fill_witness runs, per ArithmeticGate / U32 operation, per RandomAccess copy, per row otherwise; BaseSum in the
 * direction the schedule reaches first), and sorts them into dependency levels.  P2GPU_E_ARG, with a cell in
 * p2gpu_last_error: a seed outside the matrix, a cell seeded twice, a copy class that no seed, constant or generator
 * reaches, a dependency cycle; also a verifier-only handle or a device group.  A plan must be destroyed before its circuit;
 * one call at a time per circuit handle, as for every entry point. */
typedef struct p2gpu_witness_plan p2gpu_witness_plan;
int p2gpu_witness_plan_create(p2gpu_circuit *c, const uint32_t *seed_cells /* [n_seeds][2] = (row, col) */, size_t n_seeds,
                              p2gpu_witness_plan **out);
/* The same plan compiled on the device, on the handle's stream (csrc/genplan.hip): the arguments, the refusals --
 * code, words and cell -- and every array of the plan are p2gpu_witness_plan_create's, and everything that takes a plan takes
 * either.  Nothing of the circuit is read back; the scratch is released before it returns. */
int p2gpu_witness_plan_build(p2gpu_circuit *c, const uint32_t *seed_cells /* [n_seeds][2] = (row, col) */, size_t n_seeds,
                             p2gpu_witness_plan **out);
/* ---- generators that are no gate's own ----
 * plonky2's `is_equal` registers an EqualityGenerator whose four targets lie in other gates' rows (the memory writes of the ACIR
 * translation are built from it); no gate row lists it, so the caller does: the Rust side passes the EqualityGenerators of
 * `builder.generators`.  The two entry points above are the case n_generators == 0 of these two; every rule of
 * the plan holds for a generator as for a row's op: it is created behind the seeds and in front of the rows, its
 * cells get value slots, the first op by level and creation order that reaches a slot writes it and every other one compares.
 * P2GPU_E_ARG, worded in p2gpu_last_error: an unknown kind, a cell outside [n] x [num_routed_wires] (with the generator's index
 * and the cell), n_generators > 0 with a null list; an input cell that nothing writes is the "a seed is missing" refusal.  A
 * contradiction of a generator at p2gpu_generate_witness reads "generator <i>: cell (row, column)".  These two entry points take
 * records of four cells and know the equality generator only (any other kind is an unknown kind here, as it always was); a
 * generator of another kind or number of cells goes through the _genv pair below, of which these are the case of equality
 * generators, shapes {1, 1, 1, 1}. */
#define P2GPU_GEN_EQUALITY 0   /* cells: x, y (read), equal, inv (set): equal = (x == y), inv = x == y ? 0 : 1 / (x - y) */
typedef struct { uint32_t kind; uint32_t cells[4][2]; /* (row, col), routed columns only */ } p2gpu_generator;
int p2gpu_witness_plan_create_gen(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds,
                                  const p2gpu_generator *generators, size_t n_generators, p2gpu_witness_plan **out);
/* the same arguments: compiled on the device */
int p2gpu_witness_plan_build_gen(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds,
                                 const p2gpu_generator *generators, size_t n_generators, p2gpu_witness_plan **out);
/* the plan's generator table, read back: [n_generators][4] words, cell key (col << d | row) | bit 31 = this generator writes the
 * cell's slot (its writer bits live here, not in cell_slot).  *n_generators is always filled; with table NULL nothing else happens.
 * P2GPU_E_ARG for a plan one of whose generators has another number of cells than four. */
int p2gpu_witness_plan_export_generators(const p2gpu_witness_plan *p, uint32_t *table, size_t *n_generators);
/* ---- generators with any number of cells ----
 * A record is a kind and a shape, the cell counts of the generator's four groups; the cells of all generators follow each other
 * in one flat (row, col) list, shape[0] + .. + shape[3] per generator, in list order.
 *   P2GPU_GEN_EQUALITY        {1, 1, 1, 1}: x, y (read), equal, inv (set)
 *   P2GPU_GEN_BIGUINT_DIVREM  {la, lb, ld, lr}: the limbs of a and of b (read), of div and of rem (set), least significant
 *                             first -- the BigUintDivRemGenerator that `div_rem_biguint` registers (plonky2_ecdsa/biguint/
 *                             biguint.rs:231-262, :317-344; the Rust side lists it at that call site).  a and b are
 *                             the integers sum limb_i 2^(32 i) over the canonical limb values (a limb >= 2^32 carries into the
 *                             next, as `get_biguint_target` folds them); (div, rem) = divmod(a, b) as 32-bit digits.  The shape
 *                             is div_rem_biguint's: 1 <= la <= 32, 1 <= lb <= 16, lr = lb, ld = lb > la + 1 ? 0 : la - lb + 1.
 *                             Where upstream panics, p2gpu_generate_witness answers P2GPU_E_UNSATISFIED with the generator and
 *                             a cell: b = 0 -> b's first cell; a quotient or remainder with more digits than its target has
 *                             limbs -> that target's top limb (a quotient for a target without limbs: a's first cell).
 * Every rule of the plan holds per cell position: a slot that several input positions name is one dependency;
 * among the outputs the first position that names a slot may write it, every later one compares.  The op record of a generator is
 * list index | code << 32, code 13 for equality and 14 for div-rem.  P2GPU_E_ARG, worded in p2gpu_last_error and checked before
 * anything indexes with a cell: an unknown kind, a shape that is not the kind's, n_cells different from the shapes' sum (fewer:
 * reported at the first generator whose cells run past the list, with the sum up to it), a cell
 * outside [n] x [num_routed_wires] (with the generator's index and the cell), a counted list behind a null pointer. */
#define P2GPU_GEN_BIGUINT_DIVREM 1
typedef struct { uint32_t kind; uint32_t shape[4]; } p2gpu_generator_v;
/* ---- the nonnative generators ----
 * The four generators that `add_nonnative`, `sub_nonnative`, `mul_nonnative` and `inv_nonnative` register (plonky2_ecdsa/biguint/
 * gadgets/nonnative.rs:185-215, :284-310, :312-341, :365-389; generators :446-715; the Rust side lists them at those call sites,
 * INTEGRATION.md).  The record's kind word carries the field in bits 8-15: kind | field << 8, the field one of the two `FF` the
 * reference instantiates.  M is the field's modulus, A = fold(a) mod M and B = fold(b) mod M with fold as the div-rem generator
 * folds limbs (upstream's FF::from_noncanonical_biguint); a field element has L = 8 limbs; what is set are 32-bit digits, least
 * significant first, zeros in the limbs beyond them.
 *   P2GPU_GEN_NONNATIVE_ADD  {la, lb, L, 1}: a, b (read), sum, overflow (set).  S = A + B; S > M (strictly): sum = S - M,
 *                            overflow = 1; otherwise sum = S, overflow = 0 -- A + B = M leaves sum = M, as upstream.
 *   P2GPU_GEN_NONNATIVE_SUB  {la, lb, L, 1}: a, b (read), diff, overflow (set).  A >= B: diff = A - B, overflow = 0; otherwise
 *                            diff = M + A - B, overflow = 1.  For both: 0 <= la, lb <= 16, la + lb >= 1 (`neg_nonnative` subtracts
 *                            from a target without limbs).
 *   P2GPU_GEN_NONNATIVE_MUL  {la, lb, L, la + lb - L}: a, b (read), prod, overflow (set).  (overflow, prod) = divmod(A B, M);
 *                            0 <= la, lb <= 16, la + lb >= L.
 *   P2GPU_GEN_NONNATIVE_INV  {lx, 0, lx, lx}: x (read), inv, div (set).  X = fold(x) mod M, inv = 1 / X mod M, div = (X inv) div M;
 *                            1 <= lx <= 16.
 * Where upstream panics, p2gpu_generate_witness answers P2GPU_E_UNSATISFIED with the generator and a cell: X = 0 -> x's first
 * cell; a value with more digits than its target has limbs -> that target's top limb (a target without limbs: the generator's
 * first cell).  The op record is list index | (code | field << 8) << 32, codes 15 .. 18 in the order above.  An unknown kind, as
 * above and with the whole word in the message: a field other than these two, a field on kinds 0 and 1, a bit above 15, a kind
 * above 5 (but for P2GPU_GEN_GLV_DECOMPOSE, below). */
#define P2GPU_GEN_NONNATIVE_ADD 2
#define P2GPU_GEN_NONNATIVE_SUB 3
#define P2GPU_GEN_NONNATIVE_MUL 4
#define P2GPU_GEN_NONNATIVE_INV 5
#define P2GPU_FIELD_SECP256K1_BASE 0   /* 2^256 - 2^32 - 977 */
#define P2GPU_FIELD_SECP256K1_SCALAR 1 /* 0xFFFFFFFF FFFFFFFF FFFFFFFF FFFFFFFE BAAEDCE6 AF48A03B BFD25E8C D0364141 */
/* ---- the GLV decomposition generator ----
 * The GLVDecompositionGenerator that `decompose_secp256k1_scalar` registers (plonky2_ecdsa/curve/gadgets/glv.rs:117-149; generator
 * :258-285, its arithmetic :50-88; the Rust side lists it at that call site).
 *   P2GPU_GEN_GLV_DECOMPOSE  {lk, 0, 8, 2}, 1 <= lk <= 16: k's limbs (read); k1's four limbs, then k2's four; k1_neg, k2_neg (set).
 *                            K = fold(k) mod N, N the order of the secp256k1 scalar field (P2GPU_FIELD_SECP256K1_SCALAR's modulus);
 *                            c1 = round(B2 K / N), c2 = round(MINUS_B1 K / N) (N is odd: no ties); k1_raw = K - c1 A1 - c2 A2,
 *                            k2_raw = c1 MINUS_B1 - c2 B2 modulo N; a raw value above (N - 1) / 2 is negative, and its magnitude
 *                            N - raw is what is set, as 32-bit digits; the signs are 0 or 1.
 * The kind word takes no field: it is 8, and any bit above bit 7 makes it an unknown kind, with the whole word in the message.  The
 * kind numbers 6 and 7 are reserved and stay unknown kinds.  A magnitude with more digits than four limbs -> that target's top
 * limb (P2GPU_E_UNSATISFIED, as above).  The op record is list index | 19 << 32.  Every other refusal is worded as above: shape,
 * cell count, cell outside the routed cells. */
#define P2GPU_GEN_GLV_DECOMPOSE 8
int p2gpu_witness_plan_create_genv(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator_v *generators,
                                   size_t n_generators, const uint32_t *cells /* [n_cells][2] = (row, col) */, size_t n_cells,
                                   p2gpu_witness_plan **out);
/* the same arguments: compiled on the device */
int p2gpu_witness_plan_build_genv(p2gpu_circuit *c, const uint32_t *seed_cells, size_t n_seeds, const p2gpu_generator_v *generators,
                                  size_t n_generators, const uint32_t *cells, size_t n_cells, p2gpu_witness_plan **out);
/* the plan's generator table of any plan, read back: off [n_generators + 1], the first table word of every generator, and table
 * [off[n_generators]], one word per cell in list order: cell key (col << d | row) | bit 31 = this naming writes the cell's slot.
 * sizes = { n_generators, off[n_generators] } is always filled; with both pointers NULL nothing else happens.  For a list of
 * equality generators the table is p2gpu_witness_plan_export_generators' byte for byte. */
int p2gpu_witness_plan_export_generators_v(const p2gpu_witness_plan *p, uint32_t *off, uint32_t *table, size_t sizes[2]);
/* The plan's three device arrays, read back: cell_slot [num_routed_wires][n] (the value slot of every routed cell, 0xFFFFFFFF:
 * none, bit 31: this cell's op writes the slot), ops [n_ops] (row | (code | sub << 8) << 32, by level and creation order),
 * level_off [levels + 1].  sizes = { num_routed_wires * n, n_ops, levels + 1 } is always filled; with all three pointers NULL
 * nothing else happens.  A plan from either entry point. */
int p2gpu_witness_plan_export(const p2gpu_witness_plan *p, uint32_t *cell_slot, uint64_t *ops, uint32_t *level_off, size_t sizes[3]);
void p2gpu_witness_plan_destroy(p2gpu_witness_plan *p);
/* counts: ops, levels, widest level, value slots, seeds; ms: plan compilation (wall time of _create or _build), level walk of
 * the last call (device) */
int p2gpu_witness_plan_info(const p2gpu_witness_plan *p, uint64_t counts[5], double ms[2]);
/* seed_values: host, [n_seeds] in the plan's order.  wires_dev_out: device, [num_wires][n], written completely.  One workgroup
 * walks the levels, a kernel copies the class values to the routed cells, p2gpu_fill_witness's kernel derives the rest.  A
 * generator whose output already has another value, or a seed >= p: P2GPU_E_UNSATISFIED, the first offender's cell in
 * p2gpu_last_error (the matrix is then not a witness). */
int p2gpu_generate_witness(p2gpu_witness_plan *p, const uint64_t *seed_values, uint64_t *wires_dev_out);
/* `batch` witnesses of one plan in one level walk: the lanes of a level take (op, witness) pairs, and groups of witnesses
 * (WALK_GROUP in csrc/genwit.hip) get a workgroup each; the cost per witness is not measured yet.  seed_values: host,
 * [batch][n_seeds].  wires_dev_out: device, [batch][num_wires][n], written completely.  status: host, [batch], P2GPU_OK or
 * P2GPU_E_UNSATISFIED per witness; bad_cells: host, [batch][2] = (row, col) of a failing witness's first contradiction,
 * UINT32_MAX twice for a good one; may be NULL.  Witnesses do not affect each other: every matrix whose status is P2GPU_OK is
 * the complete witness a lone call gives.  Returns P2GPU_OK when every witness is good, P2GPU_E_UNSATISFIED when one is not
 * (p2gpu_last_error: "witness <b> of the batch: " and the lone call's words for the lowest failing b), P2GPU_E_ARG for a null
 * plan, output or status, batch == 0, or null values for a plan with seeds.  The plan's buffers for a batch are allocated by the
 * first call that needs them and grow with the largest batch seen; p2gpu_witness_plan_destroy frees them.  ms[1] of
 * p2gpu_witness_plan_info is the walk of the last call, lone or batched. */
int p2gpu_generate_witness_batch(p2gpu_witness_plan *p, const uint64_t *seed_values /* host, [batch][n_seeds] */, size_t batch,
                                 uint64_t *wires_dev_out /* device, [batch][num_wires][n] */,
                                 int *status /* host, [batch]: P2GPU_OK or P2GPU_E_UNSATISFIED */,
                                 uint32_t *bad_cells /* host, [batch][2] = (row, col) of the first contradiction, may be NULL */);
/* p2gpu_generate_witness into the handle's own buffer, then p2gpu_prove_dev on it: the same proof bytes.  h2d_ms of the timings
 * holds the time the witness took. */
int p2gpu_prove_seeds(p2gpu_witness_plan *p, const uint64_t *seed_values, const uint64_t *public_inputs, uint32_t n_pi,
                      uint8_t *proof_out, size_t *proof_len, p2gpu_timings *opt_timings);
/* p2gpu_generate_witness_batch into a buffer the plan owns (it grows with the largest batch seen, like the plan's other batch
 * buffers), then p2gpu_prove_batch_dev on the members the level walk accepted: the same proofs.  seed_values: host,
 * [batch][n_seeds]; the other arguments are p2gpu_prove_batch_dev's.  A member the walk refuses keeps the walk's status and, in
 * bad_cells ([batch][2], may be NULL), its cell; its proof bytes are zero.  The return value and p2gpu_last_error speak for the
 * lowest failing member, whichever stage refused it. */
int p2gpu_prove_seeds_batch(p2gpu_witness_plan *p, const uint64_t *seed_values /* host, [batch][n_seeds] */, size_t batch,
                            const uint64_t *public_inputs, uint32_t n_pi, uint8_t *proofs_out, int *status,
                            uint32_t *bad_cells /* [batch][2], may be NULL */);

/* ---- why a witness is wrong: the gate rows and copy constraints it breaks, found on the GPU ----
 * The prover's self-check answers P2GPU_E_UNSATISFIED after the commitments and names nothing; these entry points evaluate the
 * circuit on the n base rows of a wire matrix and say where it fails (the reference's user gets a panic of plonky2's witness
 * generator that names a partition; there is no counterpart for a matrix that arrives complete).  All of it is decided on the
 * device, per witness, from the handle's own tables:
 *   gates      row r fails when a constraint of gates[row_gate[r]] -- unfiltered, with the row's gate constants and the
 *              Poseidon hash of the witness's public inputs, the prover's `public_inputs_hash` -- is non-zero; constraints are
 *              numbered in the order the gate emits them (csrc/gates.hpp eval_gate, the reference's order)
 *   copies     routed cell x is flagged when its value differs from the value of sigma(x), sigma decoded from the handle's
 *              sigma columns (the decode of the witness plan); a cell sigma maps to itself is never flagged
 *   canonicity a word >= p anywhere in the matrix is counted and named; the two checks above use it reduced once (v - p)
 * Cells are ordered by the key col << degree_bits | row, as sigma is laid out.  Witnesses of a batch do not affect each other.
 * The scratch (sigma's partner cells, the per-row and per-cell results, the counters) is allocated per call and released
 * before it returns; nothing is kept on the handle. */
typedef struct {
  uint64_t gate_rows_failed;    /* rows with at least one non-zero constraint */
  uint64_t copy_cells_failed;   /* routed cells x with value(x) != value(sigma(x)) */
  uint64_t noncanonical_cells;  /* cells of the whole matrix with a word >= p */
  uint32_t gate_row, gate_index, gate_kind, constraint;  /* lowest failing row; lowest failing constraint in it */
  uint64_t constraint_value;
  uint32_t copy_cell[2], copy_partner[2];   /* (row, col): the flagged cell with the lowest key col << d | row, and sigma of it */
  uint64_t copy_values[2];                  /* the matrix's words in those two cells */
  uint32_t noncanonical_cell[2];            /* lowest key */
} p2gpu_witness_report;                      /* the "first" fields are UINT32_MAX / 0 where the count is 0 */
/* wires_dev: device, [batch][num_wires][n] (the layout of p2gpu_generate_witness_batch), only read.  Returns P2GPU_OK when every
 * report is clean; P2GPU_E_UNSATISFIED when one is not, p2gpu_last_error then words the first finding of the lowest failing
 * witness -- gates before copies before canonicity: "row 3 (U32SubtractionGate, gate 6): constraint 2 = 0x...",
 * "copy (2, 8) = 0x... != (3, 0) = 0x..." with cells as (row, col), "cell (5, 1) = 0x... is not a canonical field element" --
 * behind "witness <b> of the batch: " when batch > 1; P2GPU_E_ARG, decided before any device call: a null handle, matrix or
 * reports, batch == 0, n_pi different from the circuit's (or a public input >= p), a verifier-only handle, a device group.  The
 * reports are complete either way. */
int p2gpu_check_witness_dev(p2gpu_circuit *c, const uint64_t *wires_dev, size_t batch,
                            const uint64_t *public_inputs /* host, [batch][n_pi] */, uint32_t n_pi,
                            p2gpu_witness_report *reports /* host, [batch] */,
                            uint16_t *row_status /* host, [batch][n]: first failing constraint of the row, 0xFFFF = none; may be NULL */,
                            uint8_t *cell_flags /* host, [batch][num_routed_wires][n]: 1 = flagged copy cell; may be NULL */);
/* the same for one matrix in host memory: an upload, then the device form with batch == 1 */
int p2gpu_check_witness(p2gpu_circuit *c, const uint64_t *wires /* host, [num_wires][n] */, const uint64_t *public_inputs,
                        uint32_t n_pi, p2gpu_witness_report *report, uint16_t *row_status, uint8_t *cell_flags);
/* p2gpu_generate_witness into the handle's own buffer (as p2gpu_prove_seeds does), then the check of that matrix.  A witness the
 * level walk already refuses comes back with p2gpu_generate_witness's code and words, the report untouched. */
int p2gpu_check_seeds(p2gpu_witness_plan *p, const uint64_t *seed_values, const uint64_t *public_inputs, uint32_t n_pi,
                      p2gpu_witness_report *report, uint16_t *row_status, uint8_t *cell_flags);

/* ---- N2: prover-side precompute of `builder.build::<C>()` (host code; circuit_translation/mod.rs:80-82) ----
 * From the gate instances and the copy constraints: selector columns + groups (gates/selectors.rs), the
 * sigma polynomials (plonk/permutation_argument.rs WirePartition), k_is and the FRI arities; output is the
 * circuit blob for p2gpu_circuit_create, which does the GPU part (constants/sigmas commitment, digest).
 *   gates:  in CommonCircuitData.gates order, i.e. sorted by (degree, id); kind / p as in the blob
 *   row_gate[n]: index into `gates` of the gate instance on each row
 *   row_constants[max num_constants][n]: the gate constants of each row, column-major (NULL if no gate has any)
 *   copies[num_copies][4]: (row_a, col_a, row_b, col_b) pairs of routed cells that must be equal
 * blob_out == NULL: only report the size in *blob_len. */
typedef struct {
  uint32_t degree_bits, num_wires, num_routed_wires, num_challenges, quotient_degree_factor, rate_bits, cap_height,
      proof_of_work_bits, num_query_rounds, num_public_inputs;
} p2gpu_build_params;
typedef struct {
  uint32_t kind, p[4], degree, num_constants;
} p2gpu_gate_decl;
int p2gpu_build_blob(const p2gpu_build_params *params, const p2gpu_gate_decl *gates, uint32_t num_gates, const uint32_t *row_gate,
                     const uint64_t *row_constants, const uint32_t *copies, size_t num_copies, uint8_t *blob_out,
                     size_t *blob_len);

/* build() on the device: the arguments of p2gpu_build_blob, plus the hasher of header word 22 (0 = KeccakHash<25>,
 * 1 = PoseidonHash), to a prover handle.  The arrays are uploaded as they are; selector columns, row -> gate and the sigma
 * polynomials (connected components of the copy pairs, then one cycle per class) are made by kernels, and no blob passes
 * through host memory.  The handle equals, in every byte it can report or prove, p2gpu_circuit_create(p2gpu_build_blob(...)).
 * Follows the rules of p2gpu_circuit_create: after p2gpu_init with several ids the result is a device group and each device
 * runs the build itself; _on makes a plain handle on one named device.  A row_gate entry >= num_gates, a constant >= p or a
 * copy pair outside [n] x [num_routed_wires] is found on the device before anything indexes with it: P2GPU_E_ARG, *out = NULL.
 * Without a HIP device: P2GPU_E_DEVICE (argument errors that need no device are still P2GPU_E_ARG). */
int p2gpu_circuit_build(const p2gpu_build_params *params, const p2gpu_gate_decl *gates, uint32_t num_gates, const uint32_t *row_gate,
                        const uint64_t *row_constants, const uint32_t *copies, size_t num_copies, uint32_t hasher, p2gpu_circuit **out);
int p2gpu_circuit_build_on(const p2gpu_build_params *params, const p2gpu_gate_decl *gates, uint32_t num_gates, const uint32_t *row_gate,
                           const uint64_t *row_constants, const uint32_t *copies, size_t num_copies, uint32_t hasher, int device_id,
                           p2gpu_circuit **out);
/* The circuit blob of a prover handle, read back from the device (to cache a circuit that was built once).  out == NULL: only
 * report the size in *len.  For a handle made by p2gpu_circuit_build: exactly the bytes p2gpu_build_blob writes (flags 0, the
 * hasher in word 22).  For one made from a blob: that blob's prefix, the selector columns in their canonical form.
 * The read-back runs on the handle's own stream: like every call on a handle it must not run while another thread proves
 * on the same handle.  A device group answers from its first device (every device holds the same tables). */
int p2gpu_circuit_export_blob(const p2gpu_circuit *c, uint8_t *out, size_t *len);

/* ---- verification (host code only; needs no GPU) ------------------------------------------------
 * The counterpart of the reference's `verify` action (plonky2-backend/src/actions/verify_action.rs:11-17)
 * and of the `circuit_data.verify(proof)` assertion its tests end with (tests/factories/utils.rs:26-27),
 * on the uncompressed proof bytes p2gpu_prove writes.  Returns P2GPU_OK or P2GPU_E_VERIFY (the failed
 * check is in p2gpu_last_error).  Accepts a prover handle or a verifier-only one. */
int p2gpu_verify(const p2gpu_circuit *c, const uint8_t *proof, size_t len);

/* ---- a batch of proofs of one circuit, with a verdict per proof ----
 * The checks are p2gpu_verify's, in its order, and so is every verdict: the same functions (csrc/verifycore.hpp) run as
 * kernels -- one lane per proof for the transcript, the plonk identity at zeta and the proof-of-work bits, one lane per
 * (proof, query) for the Merkle paths, the folds and the final polynomial.
 *   status  P2GPU_OK or P2GPU_E_VERIFY
 *   reason  P2GPU_VR_*: the check that failed (0: none); there is one per rejection of p2gpu_verify
 *   query   the query the reason names, index: the initial oracle or the fold step it names; UINT32_MAX where it names none.
 *           For P2GPU_VR_LENGTH the two hold the length given and the length the circuit fixes.
 * proofs: host bytes; proof b is proofs[offsets[b] .. offsets[b + 1]) (uncompressed, as p2gpu_prove writes it: for the
 * on-disk format there is p2gpu_verify_batch_compressed below); reports: host, [batch], complete whatever the return value is.
 * Returns P2GPU_OK when every proof is valid and P2GPU_E_VERIFY when one is not: p2gpu_last_error then words the lowest
 * failing proof exactly as p2gpu_verify would, behind "proof <b> of the batch: " when batch > 1.  Proofs of a batch do not
 * affect each other.  A proof whose length is not the circuit's is answered on the host (truncated or non-canonical header,
 * else the length) and never uploaded.  P2GPU_E_ARG, decided before any device call: a null pointer, batch == 0, decreasing
 * offsets, a device group (use a plain handle).
 * p2gpu_verify_batch accepts a plain prover handle (its device and stream) and a verifier-only handle (the handle stays free
 * of device state: its few kilobytes -- gate table, cap, digest, k_is, round constants -- are uploaded per call to the first
 * device of p2gpu_init).  Scratch and the upload of the proofs are allocated per call and released before it returns.
 * The handle is const with one exception: on a prover handle whose "profile" knob is set, the two kernels are timed like every
 * other launch on its stream and added to its kernel statistics (p2gpu_kernel_stats) -- so, like every call on a prover handle,
 * it must not run while another thread uses the same handle.  A verifier-only handle is never written.
 * Without a HIP device: P2GPU_E_DEVICE -- it never falls back to the host loop.
 * p2gpu_verify_batch_host runs the same core in a plain loop on the calling thread and touches no device: the core's test
 * bed and its sanitised build, not a fallback.
 * p2gpu_verify_reason writes the wording of a report, NUL-terminated: the text behind "proof rejected: " in p2gpu_verify's
 * message for that proof ("accepted" for reason 0); P2GPU_E_BUFFER when cap is too small. */
#define P2GPU_VR_OK 0
#define P2GPU_VR_HEADER 1          /* truncated or non-canonical header (caps / openings) */
#define P2GPU_VR_ARITY 2           /* the circuit's reduction arities do not fit its size */
#define P2GPU_VR_LENGTH 3          /* not the length the circuit fixes */
#define P2GPU_VR_TAIL 4            /* non-canonical final polynomial, PoW witness or public input */
#define P2GPU_VR_ZETA 5            /* zeta lies in the subgroup */
#define P2GPU_VR_IDENTITY 6        /* vanishing(zeta) != Z_H(zeta) * quotient(zeta) */
#define P2GPU_VR_POW 7             /* proof-of-work bits */
#define P2GPU_VR_QUERY_INIT_SHAPE 8   /* query, oracle: path-length byte of an initial opening */
#define P2GPU_VR_QUERY_LEAF 9         /* query: non-canonical leaf element */
#define P2GPU_VR_QUERY_INIT_PATH 10   /* query, oracle: Merkle path of an initial oracle */
#define P2GPU_VR_QUERY_STEP_SHAPE 11  /* query, step: non-canonical fold value or path-length byte */
#define P2GPU_VR_QUERY_FOLD 12        /* query, step: the step does not continue the previous value */
#define P2GPU_VR_QUERY_STEP_PATH 13   /* query, step: Merkle path of a fold step */
#define P2GPU_VR_QUERY_FINAL 14       /* query: final polynomial at the folded point */
#define P2GPU_VR_QUERY_SIZE 15        /* (query section of the wrong size: unreachable once the length is the circuit's) */
typedef struct {
  int32_t status;
  uint32_t reason, query, index;
} p2gpu_verify_report;
int p2gpu_verify_batch(const p2gpu_circuit *c, const uint8_t *proofs, const size_t *offsets /* [batch + 1] */, size_t batch,
                       p2gpu_verify_report *reports);
int p2gpu_verify_batch_host(const p2gpu_circuit *c, const uint8_t *proofs, const size_t *offsets /* [batch + 1] */, size_t batch,
                            p2gpu_verify_report *reports);
int p2gpu_verify_reason(const p2gpu_verify_report *r, char *out, size_t cap);

/* ---- a batch of compressed proofs of one circuit (the on-disk format, see p2gpu_proof_compress below) ----
 * p2gpu_verify_batch_compressed is p2gpu_verify_batch for the bytes `plonky2-backend prove` writes: the decompression runs on
 * the device too (csrc/decompresscore.hpp as kernels, csrc/decompressdev.hip) -- one wave per proof scatters head, tail and
 * leaves, one lane per proof replays the transcript once, one lane per (proof, query) infers the dropped evaluation of every
 * fold step, one wave per (proof, tree) rebuilds the Merkle paths layer by layer -- and the uncompressed bytes exist only in
 * device memory, where the query kernel of p2gpu_verify_batch then reads them.
 * The verdict of proof b is p2gpu_verify_compressed's on that byte string: the first failure in its order, the reject sites of
 * the decompression first (P2GPU_VR_C_*, one per site; query and index are UINT32_MAX), then p2gpu_verify's (P2GPU_VR_* above).
 * p2gpu_verify_reason writes, for a P2GPU_VR_C_* code, the text behind "malformed proof: " in p2gpu_verify_compressed's message.
 * cproofs: host bytes; proof b is cproofs[offsets[b] .. offsets[b + 1]); reports: host, [batch], complete whatever the return
 * value is.  Returns P2GPU_OK when every proof is valid and P2GPU_E_VERIFY when one is not: p2gpu_last_error then words the lowest
 * failing proof exactly as p2gpu_verify_compressed would, behind "proof <b> of the batch: " when batch > 1.
 * The host only walks the container (lengths and indices: no hash, no field arithmetic) and uploads each proof at its own
 * length with a table of offsets.  A proof the walk cannot get through -- it runs out of bytes, a path is longer than its tree,
 * a stored index is >= the size of the domain, bytes trail -- is answered on the host by p2gpu_verify_compressed and never
 * uploaded.  Handles, P2GPU_E_ARG (before any device call), P2GPU_E_DEVICE (no HIP device: there is no host fallback), scratch
 * and the "profile" knob: as for p2gpu_verify_batch.
 * p2gpu_verify_batch_compressed_host runs the same core in a plain loop on the calling thread and touches no device: the core's
 * test bed and its sanitised build, not a fallback.
 * p2gpu_proof_decompress_batch runs the device stages up to the rebuilt bytes and reads them back: out is host memory,
 * [batch][p2gpu_proof_size_bound bytes]; status[b] is what p2gpu_proof_decompress returns for proof b, and where it is P2GPU_OK
 * the bytes are that call's; the bytes of every other proof are zero.  It does not judge a proof.  Returns P2GPU_OK when the
 * call itself went through, whatever the statuses are. */
#define P2GPU_VR_C_ARITY 16        /* bad reduction arity in circuit */
#define P2GPU_VR_C_HEADER 17       /* caps / openings */
#define P2GPU_VR_C_INDICES 18      /* query indices */
#define P2GPU_VR_C_INIT_ENTRY 19   /* initial tree entry */
#define P2GPU_VR_C_STEP_ENTRY 20   /* fold step entry */
#define P2GPU_VR_C_LENGTH 21       /* final polynomial / length */
#define P2GPU_VR_C_TAIL 22         /* final polynomial / public inputs */
#define P2GPU_VR_C_INDEX_CHECK 23  /* query indices differ from the transcript's */
#define P2GPU_VR_C_INIT_PATH 24    /* compressed Merkle path (initial tree) */
#define P2GPU_VR_C_STEP_PATH 25    /* compressed Merkle path (fold step) */
#define P2GPU_VR_C_FOLD_CHAIN 26   /* fold chain (unreachable: an equal leaf at one step implies equal leaves after) */
int p2gpu_verify_batch_compressed(const p2gpu_circuit *c, const uint8_t *cproofs, const size_t *offsets /* [batch + 1] */, size_t batch,
                                  p2gpu_verify_report *reports);
int p2gpu_verify_batch_compressed_host(const p2gpu_circuit *c, const uint8_t *cproofs, const size_t *offsets /* [batch + 1] */, size_t batch,
                                       p2gpu_verify_report *reports);
int p2gpu_proof_decompress_batch(const p2gpu_circuit *c, const uint8_t *cproofs, const size_t *offsets /* [batch + 1] */, size_t batch,
                                 uint8_t *out /* host, [batch][proof length of the circuit] */, int32_t *status /* [batch] */);
/* The verifier's share of a circuit -- header, gate table, constants_sigmas cap, circuit digest, k_is
 * (the blob prefix up to the constants table, flags 0b11) -- like the VK file of
 * actions/write_vk_action.rs:65-81.  out == NULL: only report the size in *len. */
int p2gpu_circuit_export_vk(const p2gpu_circuit *c, uint8_t *out, size_t *len);
/* Handle from such a blob (a full circuit blob with flags 0b11 works too: only its prefix is read).
 * No device is touched; the prove / fill / shard entry points reject it with P2GPU_E_ARG. */
int p2gpu_verifier_create(const uint8_t *blob, size_t len, p2gpu_circuit **out);
/* The same verifier key in the reference's own file format: `VerifierCircuitData::to_bytes(&BackendGateSerializer)`
 * as `write_vk` stores it (plonky2-backend/src/actions/write_vk_action.rs:65-81) and `verify` reads it
 * (noir_and_plonky2_serialization.rs:16-22).  UNPINNED: the layout is plonky2 0.2.2's util/serialization (a crate
 * that is not in the reference tree) restated from recollection -- no VK file exists there to check it against;
 * only the gate tag order (write_vk_action.rs:39-61) and the custom gates' bodies are taken from reference
 * source.  Exact inverse pair: create_plonky2(export_plonky2(c)) verifies what c verifies.
 * hasher: 0 = KeccakGoldilocksConfig (the reference), 1 = PoseidonGoldilocksConfig (the digest width is not
 * in the bytes).  out == NULL: only report the size in *len. */
int p2gpu_circuit_export_vk_plonky2(const p2gpu_circuit *c, uint8_t *out, size_t *len);
int p2gpu_verifier_create_plonky2(const uint8_t *vk, size_t len, int hasher, p2gpu_circuit **out);

/* ---- the reference's on-disk proof format (host code only) ------------------------------------
 * `plonky2-backend prove` writes hex(proof.compress(..).to_bytes()) (prove_action.rs:38-42,75-78) and
 * `verify` reads it back with verify_compressed (verify_action.rs:11-17).  compress / decompress
 * convert between p2gpu_prove's uncompressed bytes and that compressed layout (binary; hex is the
 * caller's business); out == NULL: only report the size in *out_len.  decompress rebuilds what was
 * dropped but does not judge the proof -- p2gpu_verify_compressed = decompress + p2gpu_verify. */
int p2gpu_proof_compress(const p2gpu_circuit *c, const uint8_t *proof, size_t len, uint8_t *out, size_t *out_len);
int p2gpu_proof_decompress(const p2gpu_circuit *c, const uint8_t *cproof, size_t len, uint8_t *out, size_t *out_len);
int p2gpu_verify_compressed(const p2gpu_circuit *c, const uint8_t *cproof, size_t len);

/* optional knobs: "pow_hint" (u64; UINT64_MAX = grind), "self_check" (0/1, default 1: evaluate the
 * verifier's plonk identity at zeta on the host before FRI and return P2GPU_E_UNSATISFIED when the
 * witness does not satisfy the circuit; 0 = emit the proof anyway like upstream), "shard_exercise" (0/1: with world = 1, still run the exchange steps of a sharded proof through the
 * configured transport -- how the RCCL path is tested on a one-GPU machine), "profile" (0 / 1 / 2: time kernel
 * launches with HIP events on the launch stream -- 1 = the launches that move >= 32 MB, 2 = every launch;
 * resets the statistics), "zero_columns" (0/1, default 1: one pass over the witness finds the wire columns that
 * are zero in every row -- the wires no gate of the circuit uses -- and stores zeros instead of running their
 * inverse transform and LDE; the proof bytes do not depend on it), "virtual_columns" (0/1, default 1: structured
 * wire columns that only the leaf hash and the query gather read are never stored -- both recompute them as scalar x
 * LDE(unit column); the proof bytes do not depend on it), "blocking_sync" (0/1, default 0: at the eleven transcript sync
 * points of a proof the calling thread spins in hipStreamSynchronize -- lowest latency; 1 = it sleeps on a blocking event,
 * ~10-30 us later per sync but without burning a CPU per proof in flight: for hosts with fewer CPUs than proving threads),
 * "half_gates" (0/1/2, default 1: the folded constraint sums of gates of degree <= 4 -- the reference's five custom gates,
 * BaseSum<4> -- are evaluated on the four even LDE cosets and interpolated to the odd ones where the circuit is large enough
 * for that to pay (constraints x gates >= 12 M); 2 = whatever the size, 0 = never; exact, the proof bytes do not depend on it), "shard_intt" (0/1, default 0; sharded proofs only: every rank runs the inverse transforms of ITS block of
 * the dense wire / Z-partial-product columns and the coefficient blocks are all-gathered in place, instead of every rank
 * transforming every column -- SURVEY 8(e) steps 1-2; the proof bytes do not depend on it; every rank must set it alike),
 * "shard_zs" (0/1, default 0; sharded proofs only: the chunk quotients of the permutation argument are computed for n / ranks rows
 * per rank and all-gathered in place -- SURVEY 8(e) step 5), "shard_reduce" (0/1, default 0; sharded proofs only: every rank
 * batch-reduces only its block of the opened polynomials for FRI, the partial sums are all-gathered and added -- step 8); same
 * rules: no proof byte depends on them, every rank sets them alike; "prove_batch_slab" (default 0: p2gpu_prove_batch_dev sizes its
 * slabs from its byte budget and the free memory; otherwise proofs per slab; no proof byte depends on it) */
int p2gpu_circuit_set(p2gpu_circuit *c, const char *key, uint64_t value);
/* statistics accumulated while "profile" = 1, one entry per kernel symbol:
 * names[64*i] (NUL-terminated), total milliseconds, total algorithmic bytes,
 * launch count.  Returns the number of entries written (<= cap). */
int p2gpu_kernel_stats(p2gpu_circuit *c, char *names, double *ms, double *bytes, uint64_t *launches, int cap);

/* ---- one proof over several GPUs (one process per GPU) --------------------------------------
 * Coset sharding: rank q of `world` keeps the LDE cosets {r : r mod world == q}
 * of the per-proof oracles -- whole Merkle-cap subtrees -- and only three things are exchanged
 * per proof, all through `fn` (an all-gather the host side implements with torch.distributed /
 * RCCL on the device buffers it is handed): the cap entries of each commitment (16 x 25 B), the
 * per-coset quotient interpolants (2 * N * 8 B), and the query openings.  Every rank runs the
 * transcript and returns the same proof bytes.  `fn(ctx, send_dev, recv_dev, bytes)` must gather
 * `bytes` from every rank's send buffer into recv_dev[rank * bytes ...] and return 0 when done. */
typedef int (*p2gpu_allgather_fn)(void *ctx, uint64_t send_dev, uint64_t recv_dev, uint64_t bytes_per_rank);
int p2gpu_circuit_set_shard(p2gpu_circuit *c, int rank, int world, p2gpu_allgather_fn fn, void *ctx);
/* The same with RCCL inside the library (the production transport on a multi-GPU node: xGMI): rank 0
 * obtains a 128-byte id (ncclGetUniqueId), the host side broadcasts it to the other ranks by any means
 * (torch.distributed, MPI, a file), every rank then calls p2gpu_circuit_set_shard_rccl with its rank.
 * The collectives (ncclAllGather) are enqueued on the circuit's own HIP stream -- no host synchronisation
 * around them.  RCCL is resolved with dlopen("librccl.so.1") at this point, not at link time: the copy
 * the process already uses (torch's) is taken when there is one. */
int p2gpu_shard_unique_id(uint8_t id_out[128]);
/* Host-only piece of the sharded commitment, exposed for callers that run the exchange themselves and for
 * the CPU-side tests: the Merkle cap in plonky2 order (2^cap_h x 25 B) from the all-gather of every rank's
 * local subtree roots, gathered = [world][2^rate_bits / world local cosets][2^(cap_h - rate_bits)] digests
 * of 32 B (25 used); rank q's local coset z is the global coset q + z * world. */
int p2gpu_shard_assemble_cap(int world, unsigned rate_bits, unsigned cap_h, const uint8_t *gathered, uint8_t *cap_out);
int p2gpu_circuit_set_shard_rccl(p2gpu_circuit *c, int rank, int world, const uint8_t id[128]);

/* stage-level operators (host buffers in/out; used by the parity tests) */
/* values [ncols][2^d] -> coefficients [ncols][2^d], natural order */
int p2gpu_ifft_batch(const uint64_t *vals, size_t ncols, unsigned d, uint64_t *coeffs_out);
/* coefficients [ncols][2^d] -> LDE values [ncols][2^(d+rate_bits)] on the coset g<w> (g = 14293326489335486720, plonky2's coset shift), natural order */
int p2gpu_lde_batch(const uint64_t *coeffs, size_t ncols, unsigned d, unsigned rate_bits, uint64_t *lde_out);
/* PolynomialBatch::from_values: commit value columns, return the Merkle cap (2^cap_h x 25 B) */
int p2gpu_commit_values(const uint64_t *vals, size_t ncols, unsigned d, unsigned rate_bits, unsigned cap_h,
                        uint8_t *cap_out);
/* KeccakHash<25>::hash_no_pad of `n_rows` rows of `row_len` elements (row-major) -> n_rows x 25 B */
int p2gpu_hash_rows(const uint64_t *rows, size_t n_rows, size_t row_len, uint8_t *digests_out);
/* Self-test of the device field arithmetic (the carry-chain forms of csrc/gl.hpp and the NTT's power-of-two
 * multipliers) against the portable code the host and the oracle run, on the n pairs (a[i], b[i]) of arbitrary
 * 64-bit words.  bad_out[k] = mismatches of: 0 canon, 1 add, 2 sub, 3 reduce128, 4 mul, 5 mul_add,
 * 6 x * 2^e for e = 1..95, 7 the 160-bit accumulator -- the EIGHT words p2gpu_field_selftest writes (its contract since
 * round 1); p2gpu_field_selftest16 writes SIXTEEN: those, then 8 mul_nc, 9 mul_add_nc, 10 reduce128_nc (the congruent-word
 * forms: any u64 in, some congruent u64 out), 11 add / 12 sub with a non-canonical first operand, 13 chains of those, 14 the
 * product by a 32-bit constant (multipliers: both halves of b[i], 0, 1, 7, 2^32 - 1), 15 x * 2^e for e = 96..191.  All zero on
 * a correct build. */
int p2gpu_field_selftest(const uint64_t *a, const uint64_t *b, size_t n, uint64_t bad_out[8]);
int p2gpu_field_selftest16(const uint64_t *a, const uint64_t *b, size_t n, uint64_t bad_out[16]);
/* The arithmetic that exists in device form only -- the Poseidon layers' unreduced dot products, the gate evaluator's small
 * dot product, limb recomposition, seventh power and range product, the 160-bit accumulator past three terms -- on operands the
 * caller chooses: n cases, in [n][in words], aux [n][aux words], out [n][out words], host memory.  out holds the RAW device
 * words: "congruent" below means some u64 congruent to the value mod p, not necessarily below p; comparing is the caller's.
 * No proof calls this.  Per form: in | aux | out
 *   MDS       12 words, any u64 | - | 12 congruent words: one linear layer
 *   SBOX      1 word, any u64 | - | 2 congruent words: x^7 by the permutation's and by the gate evaluator's form
 *   FUSED3    12 words, any u64 | c1, c2 < p | 12 congruent words: three layers, word 0 <- (word 0 + c1)^7 after the first and
 *             (word 0 + c2)^7 after the second;  FUSED2: two layers and the c1 step (c2 is read, not used)
 *   PERMUTE   12 words < p | - | the permutation, 12 words < p (one lane per state)
 *   COOP      12 words < p | NULL, or 4 words (any u64) for the idle lanes of the state's 16-lane group | the permutation, 12
 *             words < p (twelve lanes per state, four states per wave, sixteen per block)
 *   SMALLDOT  12 words, any u64 | 12 multipliers < 2^32, their sum < 2^31 | sum of word * multiplier: canonical, congruent
 *   HORNER    32 words < p | 32 bit counts, each 1..63, a 0 ends the case, their sum <= 63 | acc <- acc * 2^bits + word over
 *             the pushes, canonical
 *   ACC160    a < p, c any u64 | T, 1 <= T <= 2^24 | T * a * c, canonical
 *   RANGE4    1 word < p | - | v (v - 1) (v - 2) (v - 3), congruent
 * P2GPU_E_ARG: an unknown form, a null pointer, n = 0 or n > 2^24, an operand outside the ranges above. */
#define P2GPU_FORM_MDS 0
#define P2GPU_FORM_SBOX 1
#define P2GPU_FORM_FUSED3 2
#define P2GPU_FORM_FUSED2 3
#define P2GPU_FORM_PERMUTE 4
#define P2GPU_FORM_COOP 5
#define P2GPU_FORM_SMALLDOT 6
#define P2GPU_FORM_HORNER 7
#define P2GPU_FORM_ACC160 8
#define P2GPU_FORM_RANGE4 9
int p2gpu_forms_selftest(unsigned form, const uint64_t *in, size_t n, const uint64_t *aux, uint64_t *out);
/* Prover phases 1-3 (wires commitment; Z and partial products; quotient) on challenges the CALLER chooses, their raw results
 * read back: a test bed for the permutation argument and the quotient kernels.  No proof calls this.  It runs the phase
 * functions a proof runs, with betas / gammas / alphas [num_challenges] in place of the transcript's and pi_hash[4] in place
 * of the hash of public inputs; the wires [num_wires][n] need not satisfy the circuit.  With K = num_challenges,
 * PP = num_partial_products, C = 2^rate_bits, all buffers in host memory:
 *   zp_in      NULL, or [K (1 + PP)][n]: replaces the Z / partial-product values of phase 2 before they are committed
 *   zp_out     [K (1 + PP)][n]: what phase 2 computed (Z of every challenge, then the partial products), before zp_in
 *   qvals_out  [K][C][n]: the quotient values; coset r, index k is the LDE point g w_N^(C k + r)
 *   quot_out   [K C][n]: the coefficients of the quotient chunk polynomials, natural order
 *   caps_out   [3][2^cap_height][hash bytes]: the wires, Z / partial-product and quotient caps
 * The handle's knobs (half_gates, zero_columns, virtual_columns, profile) and the P2GPU_* environment switches apply as in
 * a proof; a proof on the handle afterwards is unaffected.  P2GPU_E_ARG, decided before any device call: a null pointer
 * (other than zp_in), a verifier-only handle, a device group or a sharded handle, a word >= p in any input. */
int p2gpu_plonk_stages(p2gpu_circuit *c, const uint64_t *wires, const uint64_t *pi_hash, const uint64_t *betas, const uint64_t *gammas,
                       const uint64_t *alphas, const uint64_t *zp_in, uint64_t *zp_out, uint64_t *qvals_out, uint64_t *quot_out,
                       uint8_t *caps_out);

const char *p2gpu_last_error(void);
/* name/arch of the device in use, and peak numbers the bench prints */
int p2gpu_device_info(char *name_out, size_t name_cap, int *cu_count, size_t *hbm_bytes);
/* Peer access between the devices of the last p2gpu_init (device groups, section "multi-GPU" of DESIGN.md):
 * matrix_out[a * n + b] = 1: device a reaches device b's memory directly (hipDeviceEnablePeerAccess succeeded: peer copies
 * travel over xGMI), 0: it does not (peer copies are staged through host memory), -1: a and b are the same device.
 * matrix_out may be NULL.  Returns n (>= 1), P2GPU_E_BUFFER when cap < n * n, or another error code.
 * (No reference counterpart: plonky2's prover is single-device; prove_action.rs:96 is the one call this serves.) */
int p2gpu_peer_access(int *matrix_out, int cap);

#ifdef __cplusplus
}
#endif
#endif
