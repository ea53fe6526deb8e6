"""ACIR opcodes -> Plonky2 circuit: a restatement of the slice of the reference's translation layer that
BASELINE's named circuits need, on top of the library's own `build()` (p2gpu_build_blob).

Mirrors, with the reference's names:
  * ``CircuitBuilderFromAcirToPlonky2`` (plonky2-backend/src/circuit_translation/mod.rs:37-330):
    `translate_circuit`, `binary_number_target_for_witness/_constant`, `convert_binary_number_to_number`;
  * ``AssertZeroTranslator`` (assert_zero_translator.rs:25-38, 60-115);
  * ``MemoryOperationsTranslator`` (memory_translator.rs:11-171): MemoryInit, MemoryOp reads (RandomAccessGate) and
    writes (`is_equal` + `_if` per position), the <= check on the index;
  * ``Sha256CompressionTranslator`` (sha256_translator.rs:61-273) and ``BinaryDigitsTarget``
    (binary_digits_target.rs: rotate_right 19-41, shift_right 43-64, choose 66-83, majority 85-106, xor/and
    121-149, bit_xor 181-187, add_module_32_bits 189-224);
  * in builder.py the part of plonky2 0.2.2's ``CircuitBuilder`` those reach (gadgets/arithmetic.rs `arithmetic` with its
    constant-folding special cases, `mul/add/sub/mul_sub/mul_add/mul_const_add`, `and/or/not/select`,
    `assert_bool`, gadgets/split_join.rs `split_le` / `le_sum` with BaseSumGate<2>, constants in ConstantGates,
    the PublicInputGate row of `build()`, Noop padding; for the memory opcodes `is_equal` with its EqualityGenerator,
    `_if`, `random_access` with RandomAccessGate rows and their extra constants -- these UNPINNED, see their docstrings)
    -- recollection of an un-vendored crate, checked by what can be checked here: every circuit it emits is satisfiable only
    by the right values (the reference's own SHA-256 compression vector, tests/test_sha256_internal.rs:481-549, comes out of
    it), and the oracle and the GPU prove it to identical bytes;
  * ``EcdsaSecp256k1Translator`` (ecdsa_secp256k1_translator.rs:38-121), quirks kept (see the class);
  * in gadgets_u32.py, gadgets_biguint.py and gadgets_nonnative.py the three traits of the reference's own tree above it
    (plonky2_ecdsa/biguint), and in gadgets_curve.py and gadgets_glv.py the split, curve and GLV traits above those
    (plonky2_ecdsa/biguint/gadgets/split_nonnative.rs, plonky2_ecdsa/curve/gadgets), as mixins: their docstrings say what is pinned.
This module composes them into `CircuitBuilder`, keeps the translators and re-exports every name callers reach as `translate.X`.

What it is NOT: an ACIR *reader*.  The reference deserialises gzip + bincode `Program` bytes through the acvm
crate (noir_and_plonky2_serialization.rs:42-64); no compiled program exists in the tree to test a reader on, so
programs are given as Python data: [("assert_zero", mul_terms, linear, q_c), ("sha256_compression", inputs16,
hash8, outputs8), ("range", w, num_bits), ("and" | "xor", lhs, rhs, output, num_bits), ("memory_init", block_id, [witnesses]),
("memory_op", block_id, operation, index_witness, value_witness), ("ecdsa_secp256k1", pkx32, pky32, signature64, hashed_message32,
output)] (mod.rs:105-180).

Host-side Python by design: translation runs once per circuit, off the hot path (north_star keeps this layer in
Rust; this file exists so that the named SHA256 circuit can be built and proved without it).
"""
import numpy as np

from . import builder
from .builder import (BASE_SUM_LIMBS, G_ARITHMETIC, G_BASE_SUM, G_CONSTANT, G_NOOP, G_POSEIDON, G_PUBLIC_INPUT,  # noqa: F401
                      G_RANDOM_ACCESS, GENERATORS, NUM_CONSTANTS, NUM_OPS, NUM_ROUTED, NUM_WIRES, ROW_KINDS, Generator, Layout, P)
from .gadgets_biguint import CircuitBuilderBiguint
from .gadgets_curve import SECP256K1_GENERATOR_X, SECP256K1_GENERATOR_Y, CircuitBuilderCurve, CircuitBuilderSplit  # noqa: F401
from .gadgets_glv import A1, A2, B2, GLV_BETA, GLV_S, MINUS_B1, CircuitBuilderGlv, decompose_secp256k1_scalar  # noqa: F401
from .gadgets_nonnative import NONNATIVE_EVENTS, NONNATIVE_FIELDS, CircuitBuilderNonNative  # noqa: F401
from .gadgets_u32 import (G_COMPARISON, G_U32_ADD_MANY, G_U32_ARITHMETIC, G_U32_RANGE_CHECK, G_U32_SUBTRACTION,  # noqa: F401
                          MAX_NUM_ADDENDS, U32_MAX, CircuitBuilderU32)
from .prover import WitnessPlan

GEN_EQUALITY, GEN_BIGUINT_DIVREM = (WitnessPlan.GENERATOR_KINDS[k] for k in ("equality", "biguint_divrem"))      # p2gpu.h P2GPU_GEN_*
GEN_NONNATIVE_ADD, GEN_NONNATIVE_SUB, GEN_NONNATIVE_MUL, GEN_NONNATIVE_INV = (WitnessPlan.NONNATIVE_KINDS[k] for k in NONNATIVE_EVENTS.values())
GEN_GLV_DECOMPOSE = WitnessPlan.GLV_KINDS["glv_decompose"]


class CircuitBuilder(CircuitBuilderGlv, CircuitBuilderCurve, CircuitBuilderSplit, CircuitBuilderNonNative, CircuitBuilderBiguint, CircuitBuilderU32,
                     builder.CircuitBuilder):
    """plonky2's CircuitBuilder with the traits the reference's tree implements on it."""


class BinaryDigitsTarget:
    """binary_digits_target.rs: a number as its bits, most significant first."""

    def __init__(self, bits):
        self.bits = list(bits)

    @staticmethod
    def rotate_right(t, times, b):
        n = len(t.bits)
        new = []
        for i in list(range(n - times, n)) + list(range(0, n - times)):
            nb = b.add_virtual_bool_target_safe()
            b.connect(t.bits[i], nb)
            new.append(nb)
        return BinaryDigitsTarget(new)

    @staticmethod
    def shift_right(t, times, b):
        new = [b.constant(0) for _ in range(times)]
        for i in range(len(t.bits) - times):
            nb = b.add_virtual_bool_target_safe()
            b.connect(t.bits[i], nb)
            new.append(nb)
        return BinaryDigitsTarget(new)

    @staticmethod
    def choose(chooser, on_true, on_false, b):
        return BinaryDigitsTarget([b.select(c, t, f) for c, t, f in zip(chooser.bits, on_true.bits, on_false.bits)])

    @staticmethod
    def majority(a, bb, c, b):
        out = []
        for b0, b1, b2 in zip(c.bits, a.bits, bb.bits):
            on_true = b.or_(b1, b2)
            on_false = b.and_(b1, b2)
            out.append(b.select(b0, on_true, on_false))
        return BinaryDigitsTarget(out)

    @staticmethod
    def bit_xor(x, y, b):
        x_or_y = b.or_(x, y)
        x_and_y = b.and_(x, y)
        return b.and_(x_or_y, b.not_(x_and_y))

    @staticmethod
    def xor(x, y, b):
        return BinaryDigitsTarget([BinaryDigitsTarget.bit_xor(p, q, b) for p, q in zip(x.bits, y.bits)])

    @staticmethod
    def add_module_32_bits(x, y, b):
        assert len(x.bits) == len(y.bits)
        partial_sum = [BinaryDigitsTarget.bit_xor(p, q, b) for p, q in zip(x.bits, y.bits)]
        partial_carries = [b.and_(p, q) for p, q in zip(x.bits, y.bits)]
        carry_in = b._false()
        out = []
        for i in reversed(range(len(x.bits))):
            s = BinaryDigitsTarget.bit_xor(partial_sum[i], carry_in, b)
            pair = b.and_(carry_in, partial_sum[i])
            carry_in = b.or_(partial_carries[i], pair)
            out.append(s)
        out.reverse()
        return BinaryDigitsTarget(out)


SHA256_K = [
    0x428a2f98, 0x71374491, 0xb5c0fbcf, 0xe9b5dba5, 0x3956c25b, 0x59f111f1, 0x923f82a4, 0xab1c5ed5, 0xd807aa98, 0x12835b01,
    0x243185be, 0x550c7dc3, 0x72be5d74, 0x80deb1fe, 0x9bdc06a7, 0xc19bf174, 0xe49b69c1, 0xefbe4786, 0x0fc19dc6, 0x240ca1cc,
    0x2de92c6f, 0x4a7484aa, 0x5cb0a9dc, 0x76f988da, 0x983e5152, 0xa831c66d, 0xb00327c8, 0xbf597fc7, 0xc6e00bf3, 0xd5a79147,
    0x06ca6351, 0x14292967, 0x27b70a85, 0x2e1b2138, 0x4d2c6dfc, 0x53380d13, 0x650a7354, 0x766a0abb, 0x81c2c92e, 0x92722c85,
    0xa2bfe8a1, 0xa81a664b, 0xc24b8b70, 0xc76c51a3, 0xd192e819, 0xd6990624, 0xf40e3585, 0x106aa070, 0x19a4c116, 0x1e376c08,
    0x2748774c, 0x34b0bcb5, 0x391c0cb3, 0x4ed8aa4a, 0x5b9cca4f, 0x682e6ff3, 0x748f82ee, 0x78a5636f, 0x84c87814, 0x8cc70208,
    0x90befffa, 0xa4506ceb, 0xbef9a3f7, 0xc67178f2]


class MemoryOperationsTranslator:
    """memory_translator.rs:11-171, quirks kept: the block is padded with `zero` to a power of two and its real length kept
    beside it; the `predicate` of a MemoryOp is ignored; a write replaces EVERY position of the padded block."""

    def __init__(self, builder, witness_target_map, memory_blocks):
        self.builder, self.witness_target_map, self.memory_blocks = builder, witness_target_map, memory_blocks

    def _target(self, w):
        if w not in self.witness_target_map:
            self.witness_target_map[w] = self.builder.add_virtual_target()
        return self.witness_target_map[w]

    @staticmethod
    def _single_witness(e, what):
        """Expression::to_witness (the reference unwraps its None): `e` is a witness index, or an expression (mul_terms,
        linear, q_c) that is one witness with coefficient one and no constant term."""
        if isinstance(e, (int, np.integer)):
            return int(e)
        mul_terms, linear, q_c = e
        if mul_terms or len(linear) != 1 or linear[0][0] % P != 1 or q_c % P != 0:
            raise ValueError("memory operation: the %s is not a single witness" % what)
        return linear[0][1]

    # memory_translator.rs:128-151
    def translate_memory_init(self, init, block_id):
        targets = [self._target(w) for w in init]
        real = len(targets)
        padded = 1 << (real - 1).bit_length() if real else 0
        targets += [self.builder.zero() for _ in range(padded - real)]
        self.memory_blocks[block_id] = (targets, real)

    # memory_translator.rs:55-83
    @staticmethod
    def add_restrictions_to_assert_target_is_less_or_equal_to(max_allowed_value, target_index, builder):
        binary = [int(c) for c in format(max_allowed_value, "b")]
        bits = list(reversed(builder.split_le(target_index, len(binary))))
        acc = builder.one()
        for bound_bit, bit in zip(binary, bits):
            if bound_bit == 0:
                builder.assert_zero(builder.mul(bit, acc))
            else:
                acc = builder.mul(acc, bit)

    # memory_translator.rs:30-51
    def translate_memory_op(self, block_id, operation, index, value):
        wi, wv = self._single_witness(index, "index"), self._single_witness(value, "value")
        self._target(wi)
        self._target(wv)
        if isinstance(operation, tuple):
            if operation[0] or operation[1]:
                raise ValueError("memory operation: the operation is not a constant")
            operation = operation[2]
        if not isinstance(operation, (int, np.integer)):
            raise ValueError("memory operation: the operation is not a constant")
        block, real = self.memory_blocks[block_id]
        self.add_restrictions_to_assert_target_is_less_or_equal_to(real - 1, self._target(wi), self.builder)
        if operation % P == 0:      # :115-125
            self.witness_target_map[wv] = self.builder.random_access(self._target(wi), list(block))
        elif operation % P == 1:    # :89-112
            b = self.builder
            for position in range(len(block)):
                here = b.is_equal(self._target(wi), b.constant(position))
                block[position] = b._if(here, self._target(wv), block[position])
        else:
            raise ValueError("Backend encountered unknown memory operation code (nor 0 or 1)")


class EcdsaSecp256k1Translator:
    """ecdsa_secp256k1_translator.rs:38-121, quirks kept: each 32-byte string is read LITTLE-endian -- limb i is
    b[4i] + 2^8 b[4i+1] + 2^16 b[4i+2] + 2^24 b[4i+3], limb 0 the least significant -- and the output is `cmp_biguint(r, R.x)`,
    which is r <= R.x, not equality.  So the circuit proves r <= R.x for R = (h / s) G + (r / s) Q over those readings, not the
    ECDSA verification of the big-endian values.  The public key is not checked to be on the curve, as upstream."""

    def __init__(self, translator, hashed_msg, public_key_x, public_key_y, signature, output):
        self.translator, self.builder = translator, translator.builder
        self.hashed_msg, self.public_key_x, self.public_key_y = list(hashed_msg), list(public_key_x), list(public_key_y)
        self.signature, self.output = list(signature), output
        assert len(self.hashed_msg) == len(self.public_key_x) == len(self.public_key_y) == 32 and len(self.signature) == 64

    # :38-59
    def translate(self):
        b = self.builder
        public_key = self._public_key_target()
        r = self._32_bytes_to_field_element(self.signature[:32], "secp256k1_scalar")
        s = self._32_bytes_to_field_element(self.signature[32:], "secp256k1_scalar")
        h = self._32_bytes_to_field_element(self.hashed_msg, "secp256k1_scalar")
        r_point = self._calculate_r(public_key, r, s, h)
        does_signature_verify = b.cmp_biguint(r, r_point[0])
        b.connect(does_signature_verify, self.translator._target(self.output))

    # :61-87
    def _calculate_r(self, public_key, r, s, h):
        b, field = self.builder, "secp256k1_scalar"
        s1 = b.inv_nonnative(s, field)
        u_1 = b.mul_nonnative(h, s1, field)
        u_2 = b.mul_nonnative(r, s1, field)
        generator = b.curve_generator_constant()
        r_factor_1 = b.glv_mul(generator, u_1)
        r_factor_2 = b.glv_mul(public_key, u_2)
        return b.curve_add(r_factor_1, r_factor_2)

    # :89-93
    def _public_key_target(self):
        x = self._32_bytes_to_field_element(self.public_key_x, "secp256k1_base")
        y = self._32_bytes_to_field_element(self.public_key_y, "secp256k1_base")
        return x, y

    # :95-121
    def _32_bytes_to_field_element(self, byte_witnesses, field):
        b = self.builder
        byte_targets = [self.translator._target(w) for w in byte_witnesses]
        u32_limbs = []
        for i in range(8):
            target_0 = byte_targets[4 * i]
            target_1 = b.mul_const(1 << 8, byte_targets[4 * i + 1])
            target_2 = b.mul_const(1 << 16, byte_targets[4 * i + 2])
            target_3 = b.mul_const(1 << 24, byte_targets[4 * i + 3])
            u32_limbs.append(b.add_many([target_0, target_1, target_2, target_3]))
        return b.biguint_to_nonnative(u32_limbs, field)


class CircuitBuilderFromAcirToPlonky2:
    """mod.rs:37-330, for programs given as Python data (see the module docstring)."""

    def __init__(self, num_wires=NUM_WIRES):
        self.builder = CircuitBuilder(num_wires=num_wires)
        self.witness_target_map = {}
        self.memory_blocks = {}     # block id -> ([targets, padded to a power of two], real length)  (mod.rs:47)

    def _target(self, w):
        if w not in self.witness_target_map:
            self.witness_target_map[w] = self.builder.add_virtual_target()
        return self.witness_target_map[w]

    def binary_number_target_for_witness(self, w, digits):
        return BinaryDigitsTarget(reversed(self.builder.split_le(self._target(w), digits)))

    def binary_number_target_for_constant(self, constant, digits):
        return BinaryDigitsTarget(reversed([self.builder.constant_bool(bool(constant & (1 << i))) for i in range(digits)]))

    def convert_binary_number_to_number(self, a):
        return self.builder.le_sum(reversed(a.bits))

    # assert_zero_translator.rs:25-38
    def translate_assert_zero(self, mul_terms, linear, q_c):
        b = self.builder
        for _, w1, w2 in mul_terms:
            self._target(w1)
            self._target(w2)
        for _, w in linear:
            self._target(w)
        acc = b.constant(q_c)
        for f, w in linear:
            acc = b.add(b.mul_const(f, self._target(w)), acc)
        for f, w1, w2 in mul_terms:
            acc = b.add(b.mul_const(f, b.mul(self._target(w1), self._target(w2))), acc)
        b.assert_zero(acc)

    # sha256_translator.rs:61-117
    def translate_sha256_compression(self, inputs, hash_values, outputs):
        b, B = self.builder, BinaryDigitsTarget
        w = [self.binary_number_target_for_witness(i, 32) for i in inputs]

        def sig(t, r1, r2, r3, last_is_shift):
            x1, x2 = B.rotate_right(t, r1, b), B.rotate_right(t, r2, b)
            x3 = B.shift_right(t, r3, b) if last_is_shift else B.rotate_right(t, r3, b)
            return B.xor(B.xor(x1, x2, b), x3, b)

        for t in range(16, 64):
            s1 = B.add_module_32_bits(sig(w[t - 2], 17, 19, 10, True), w[t - 7], b)
            s2 = B.add_module_32_bits(sig(w[t - 15], 7, 18, 3, True), w[t - 16], b)
            w.append(B.add_module_32_bits(s1, s2, b))
        k = [self.binary_number_target_for_constant(c, 32) for c in SHA256_K]
        h0 = [self.binary_number_target_for_witness(i, 32) for i in hash_values]
        a, bb, c, d, e, f, g, h = h0
        for t in range(64):
            big1 = sig(e, 6, 11, 25, False)
            ch = B.choose(e, f, g, b)
            s0 = B.add_module_32_bits(k[t], w[t], b)
            s1 = B.add_module_32_bits(h, big1, b)
            s2 = B.add_module_32_bits(ch, s0, b)
            t1 = B.add_module_32_bits(s1, s2, b)
            big0 = sig(a, 2, 13, 22, False)
            maj = B.majority(a, bb, c, b)
            t2 = B.add_module_32_bits(big0, maj, b)
            a, bb, c, d, e, f, g, h = B.add_module_32_bits(t1, t2, b), a, bb, c, B.add_module_32_bits(d, t1, b), e, f, g
        for ow, x0, x1 in zip(outputs, h0, (a, bb, c, d, e, f, g, h)):
            self.witness_target_map[ow] = self.convert_binary_number_to_number(B.add_module_32_bits(x0, x1, b))

    # mod.rs:131-139: BlackBoxFuncCall::RANGE -> builder.range_check = split_le
    def translate_range(self, w, num_bits):
        assert num_bits <= 33, "Range checks with more than 33 bits are not allowed yet while using Plonky2 prover"
        self.builder.split_le(self._target(w), num_bits)

    # mod.rs:140-155, 222-238: AND / XOR through the bit decompositions
    def translate_bitwise(self, lhs, rhs, output, num_bits, xor):
        x = self.binary_number_target_for_witness(lhs, num_bits)
        y = self.binary_number_target_for_witness(rhs, num_bits)
        b = self.builder
        bits = ([BinaryDigitsTarget.bit_xor(p, q, b) for p, q in zip(x.bits, y.bits)] if xor
                else [b.and_(p, q) for p, q in zip(x.bits, y.bits)])
        self.witness_target_map[output] = self.convert_binary_number_to_number(BinaryDigitsTarget(bits))

    def translate_circuit(self, opcodes, public_parameters=(), private_parameters=()):
        # mod.rs:290-310 _register_witnesses_from_acir_circuit: public parameters first -- a fresh target each, registered as a
        # Plonky2 public input -- then the private ones (return values are NOT public inputs).  The reference holds
        # both in BTreeSets (acir Circuit::public_parameters / private_parameters): iteration is by ascending witness index
        # whatever order the caller lists them in, and that order fixes the public-input order (hence the in-circuit
        # Poseidon hash, the circuit digest and the proof bytes)
        for w in sorted(set(public_parameters)):
            t = self.builder.add_virtual_target()
            self.builder.register_public_input(t)
            self.witness_target_map[w] = t
        for w in sorted(set(private_parameters)):
            self._target(w)
        self.opcode_first_row = []            # per opcode: the builder rows that existed when its translation began, then their final count (explain)
        for op in opcodes:
            self.opcode_first_row.append(len(self.builder.rows))
            if op[0] == "assert_zero":
                self.translate_assert_zero(*op[1:])
            elif op[0] == "sha256_compression":
                self.translate_sha256_compression(*op[1:])
            elif op[0] == "range":
                self.translate_range(*op[1:])
            elif op[0] in ("and", "xor"):
                self.translate_bitwise(*op[1:], xor=op[0] == "xor")
            elif op[0] == "memory_init":
                MemoryOperationsTranslator(self.builder, self.witness_target_map, self.memory_blocks).translate_memory_init(op[2], op[1])
            elif op[0] == "memory_op":
                MemoryOperationsTranslator(self.builder, self.witness_target_map, self.memory_blocks).translate_memory_op(*op[1:])
            elif op[0] == "ecdsa_secp256k1":      # mod.rs:166-180, :203-216
                pkx, pky, signature, hashed_message, output = op[1:]
                EcdsaSecp256k1Translator(self, hashed_message, pkx, pky, signature, output).translate()
            else:
                raise NotImplementedError(op[0])
        self.opcode_first_row.append(len(self.builder.rows))      # (the rows build() adds behind them are no opcode's)

    def build(self, acir_witness):
        """acir_witness: {witness index: value} for every witness the solver would hand over (at least the
        inputs; outputs given are checked against what the circuit forces).  Returns (blob, wires)."""
        vals = {self.witness_target_map[w]: v for w, v in acir_witness.items() if w in self.witness_target_map}
        return self.builder.build(vals)

    def witness_seeds(self, acir_witness):
        """(seed cells, seed values) for CircuitData.witness_plan(cells).prove(values): the inputs of `acir_witness`
        ({witness index: value}) without build()'s event loop.  Outputs the solver also knows may be given; only the
        circuit's inputs are read."""
        b = self.builder
        vals = {self.witness_target_map[w]: v for w, v in acir_witness.items() if w in self.witness_target_map}
        _, roots = b._seed_classes()
        roots = set(roots)
        return b.seed_cells(), b.seed_values({t: v for t, v in vals.items() if b.find(t) in roots})

    def witness_generators(self):
        """The generators that are no gate's own (the equality generators of the memory writes, the big-integer ones of ECDSA), for
        CircuitData.witness_plan(cells, generators=...) beside witness_seeds()."""
        return self.builder.generators()

    def blob(self):
        """The circuit blob alone (build() without the witness)."""
        return self.builder.blob()

    def explain(self, report):
        """``CircuitBuilder.explain`` of a WitnessReport, with the ACIR opcode whose translation created the failing row.  (A row
        that holds several operations is shared: its later operations may serve later opcodes)"""
        text = self.builder.explain(report)
        if report.first_gate is not None and report.first_gate[0] < len(self.builder.rows):
            first = getattr(self, "opcode_first_row", [])
            i = sum(1 for r in first if r <= report.first_gate[0]) - 1
            if 0 <= i < len(first) - 1:
                text += "; the row was created by ACIR opcode %d" % i
        return text

    def public_inputs(self):
        """Values of the registered public inputs, in order (after build): what p2gpu_prove takes beside the wires."""
        return list(self.builder.public_input_values)

    def witness_value(self, w):
        return self.builder.value_of(self.witness_target_map[w])
