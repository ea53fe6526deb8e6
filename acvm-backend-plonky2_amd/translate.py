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
  * the part of plonky2 0.2.2's ``CircuitBuilder`` those reach (gadgets/arithmetic.rs `arithmetic` with its
    constant-folding special cases, `mul/add/sub/mul_sub/mul_add/mul_const_add`, `and/or/not/select`,
    `assert_bool`, gadgets/split_join.rs `split_le` / `le_sum` with BaseSumGate<2>, constants in ConstantGates,
    the PublicInputGate row of `build()`, Noop padding; for the memory opcodes `is_equal` with its EqualityGenerator,
    `_if`, `random_access` with RandomAccessGate rows and their extra constants -- these UNPINNED, see their docstrings)
    -- recollection of an un-vendored crate, checked by what
    can be checked here: every circuit it emits is satisfiable only by the right values (the reference's own
    SHA-256 compression vector, tests/test_sha256_internal.rs:481-549, comes out of it), and the oracle and the
    GPU prove it to identical bytes.

  * the u32 and biguint gadgets of the reference's own tree (plonky2_ecdsa/biguint/gadgets/arithmetic_u32.rs,
    multiple_comparison.rs, range_check_u32.rs, biguint/biguint.rs) over its five gates (biguint/gates/*.rs: shapes, wire
    positions, degrees and ids are read off that source, so they are pinned), with the BigUintDivRemGenerator of
    `div_rem_biguint` as the event "divrem".  Only `find_slot`, plonky2's row sharing, is UNPINNED (see `_u32_slot`).
  * the nonnative gadgets above them (plonky2_ecdsa/biguint/gadgets/nonnative.rs:131-443, `CircuitBuilderNonNative`), the field
    an argument (a name of NONNATIVE_FIELDS), with their four generators as the events "nnadd", "nnsub", "nnmul", "nninv".
    `add_many_nonnative` is left out (nothing on the ECDSA path calls it).

What it is NOT: an ACIR *reader*.  The reference deserialises gzip + bincode `Program` bytes through the acvm
crate (noir_and_plonky2_serialization.rs:42-64); no compiled program exists in the tree to test a reader on, so
programs are given as Python data: [("assert_zero", mul_terms, linear, q_c), ("sha256_compression", inputs16,
hash8, outputs8), ("range", w, num_bits), ("and" | "xor", lhs, rhs, output, num_bits), ("memory_init", block_id, [witnesses]),
("memory_op", block_id, operation, index_witness, value_witness)] (mod.rs:105-155).  Public parameters (which add PoseidonGate rows in `build()`) are not supported here.

Host-side Python by design: translation runs once per circuit, off the hot path (north_star keeps this layer in
Rust; this file exists so that the named SHA256 circuit can be built and proved without it).
"""
import numpy as np

from .prover import build_blob
from .synth import poseidon_gate_row

P = 0xFFFFFFFF00000001
NUM_WIRES, NUM_ROUTED, NUM_OPS, BASE_SUM_LIMBS = 234, 80, 20, 63
G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC, G_BASE_SUM, G_RANDOM_ACCESS, G_POSEIDON = 0, 1, 2, 3, 4, 5, 6
NUM_CONSTANTS = 2            # CircuitConfig::num_constants of both configurations
GEN_EQUALITY = 0             # p2gpu.h P2GPU_GEN_EQUALITY
GEN_BIGUINT_DIVREM = 1       # p2gpu.h P2GPU_GEN_BIGUINT_DIVREM
GEN_NONNATIVE_ADD, GEN_NONNATIVE_SUB, GEN_NONNATIVE_MUL, GEN_NONNATIVE_INV = 2, 3, 4, 5   # p2gpu.h P2GPU_GEN_NONNATIVE_*
# the two `FF` the reference instantiates (plonky2_ecdsa/curve/secp256k1.rs, glv.rs): name -> (p2gpu.h P2GPU_FIELD_*, order)
NONNATIVE_FIELDS = {"secp256k1_base": (0, 2**256 - 2**32 - 977),
                    "secp256k1_scalar": (1, 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141)}
NONNATIVE_EVENTS = {"nnadd": "nonnative_add", "nnsub": "nonnative_sub", "nnmul": "nonnative_mul", "nninv": "nonnative_inv"}
G_U32_ARITHMETIC, G_U32_ADD_MANY, G_U32_SUBTRACTION, G_U32_RANGE_CHECK, G_COMPARISON = 7, 8, 9, 10, 11   # p2gpu.h gate kinds
MAX_NUM_ADDENDS = 16         # gates/add_many_u32.rs:24
U32_MAX = 0xFFFFFFFF
_PHANTOM = "_phantom: PhantomData<plonky2_field::goldilocks_field::GoldilocksField>"


class CircuitBuilder:
    """The slice of plonky2's CircuitBuilder<GoldilocksField, 2> (wide_ecc_config, mod.rs:69) the translators use."""

    def __init__(self, seed=2024, num_wires=NUM_WIRES):
        # num_wires: 234 = wide_ecc_config (what the reference builds with today, mod.rs:69); 135 = standard_recursion_config
        # (what the two proofs the reference ships were built with: tests/test_translate.py reproduces their circuits).
        # Both have 80 routed wires, so ArithmeticGate holds 20 operations and BaseSumGate<2> 63 limbs in either.
        self.num_wires = num_wires
        self.public_inputs = []   # targets, in registration order (circuit_builder.rs register_public_input)
        self.parent = []
        self.const_of, self.consts = {}, {}
        self.rows = []            # gate instances in creation order
        self.free_arith = {}      # (c0, c1) -> row with a free slot
        self.arith_results = {}   # (c0, c1, m0, m1, addend) -> output target of the identical earlier operation
        self.events = []          # witness generators in creation order
        self.free_ra = {}         # bits -> RandomAccess row with a free copy
        self.free_u32 = {}        # (gate, params) -> U32 row with a free operation
        self.rng = np.random.default_rng(seed)
        self._lay = None          # what _layout() made

    # -- targets, copy constraints --------------------------------------------------------------
    def add_virtual_target(self):
        self.parent.append(len(self.parent))
        return len(self.parent) - 1

    def find(self, x):
        p = self.parent
        r = x
        while p[r] != r:
            r = p[r]
        while p[x] != r:
            p[x], x = r, p[x]
        return r

    def connect(self, a, b):
        ra, rb = self.find(a), self.find(b)
        if ra != rb:
            if ra < rb:
                self.parent[rb] = ra
            else:
                self.parent[ra] = rb

    def constant(self, c):
        c %= P
        t = self.consts.get(c)
        if t is None:
            t = self.add_virtual_target()
            self.consts[c] = t
            self.const_of[t] = c
        return t

    def zero(self):
        return self.constant(0)

    def one(self):
        return self.constant(1)

    def two(self):
        return self.constant(2)

    def constant_bool(self, b):
        return self.constant(1 if b else 0)

    def _false(self):
        return self.constant_bool(False)

    def assert_zero(self, x):
        self.connect(x, self.zero())

    def register_public_input(self, t):
        self.public_inputs.append(t)

    # -- gadgets/arithmetic.rs --------------------------------------------------------------------
    def arithmetic(self, c0, c1, m0, m1, addend):
        c0 %= P
        c1 %= P
        zero = self.zero()
        k0, k1, ka = self.const_of.get(m0), self.const_of.get(m1), self.const_of.get(addend)
        first_zero = c0 == 0 or m0 == zero or m1 == zero
        second_zero = c1 == 0 or addend == zero
        first_const = 0 if first_zero else (k0 * k1 * c0 % P if k0 is not None and k1 is not None else None)
        second_const = 0 if second_zero else (ka * c1 % P if ka is not None else None)
        if first_const is not None and second_const is not None:
            return self.constant((first_const + second_const) % P)
        if first_zero and c1 == 1:
            return addend
        if second_zero:
            if k0 is not None and k0 * c0 % P == 1:
                return m1
            if k1 is not None and k1 * c0 % P == 1:
                return m0
        # plonky2's `base_arithmetic_results`: an identical operation (same constants, same targets) returns the earlier
        # output instead of a fresh ArithmeticGate slot (gadgets/arithmetic.rs CircuitBuilder::arithmetic)
        op = (c0, c1, m0, m1, addend)
        cached = self.arith_results.get(op)
        if cached is not None:
            return cached
        key = (c0, c1)
        r = self.free_arith.get(key)
        if r is None or len(self.rows[r]["ops"]) == NUM_OPS:
            r = len(self.rows)
            self.rows.append({"kind": "arith", "c": key, "ops": []})
            self.free_arith[key] = r
        out = self.add_virtual_target()
        self.rows[r]["ops"].append((m0, m1, addend, out))
        self.events.append(("arith", c0, c1, m0, m1, addend, out))
        self.arith_results[op] = out
        return out

    def mul(self, x, y):
        return self.arithmetic(1, 0, x, y, x)

    def add(self, x, y):
        return self.arithmetic(1, 1, x, self.one(), y)

    def sub(self, x, y):
        return self.arithmetic(1, P - 1, x, self.one(), y)

    def mul_add(self, x, y, z):
        return self.arithmetic(1, 1, x, y, z)

    def mul_sub(self, x, y, z):
        return self.arithmetic(1, P - 1, x, y, z)

    def mul_const(self, c, x):
        return self.mul(self.constant(c), x)

    def mul_const_add(self, c, x, y):
        return self.mul_add(self.constant(c), x, y)

    # -- booleans (gadgets/arithmetic.rs, gadgets/select.rs) ---------------------------------------
    def assert_bool(self, b):
        self.connect(self.mul_sub(b, b, b), self.zero())

    def add_virtual_bool_target_safe(self):
        b = self.add_virtual_target()
        self.assert_bool(b)
        return b

    def add_virtual_bool_target_unsafe(self):
        """circuit_builder.rs add_virtual_bool_target_unsafe: nothing constrains it to a bit"""
        return self.add_virtual_target()

    def and_(self, a, b):
        return self.mul(a, b)

    def or_(self, a, b):
        return self.add(self.arithmetic(P - 1, 1, a, b, a), b)

    def not_(self, b):
        return self.sub(self.one(), b)

    def select(self, b, x, y):
        return self.mul_sub(b, x, self.mul_sub(b, y, y))

    def _if(self, b, x, y):
        return self.select(b, x, y)

    def is_equal(self, x, y):
        """gadgets/arithmetic.rs `is_equal` -- UNPINNED: the order of its steps is a recollection of plonky2 0.2.2.  The
        EqualityGenerator it registers belongs to no gate row: its four targets lie in ArithmeticGate rows (event "equal")."""
        zero = self.zero()
        equal = self.add_virtual_target()              # add_virtual_bool_target_unsafe
        not_equal = self.not_(equal)
        inv = self.add_virtual_target()
        self.events.append(("equal", x, y, equal, inv))
        diff = self.sub(x, y)
        not_equal_check = self.mul(diff, inv)
        diff_normalized = self.mul(diff, equal)
        self.connect(diff_normalized, zero)
        self.connect(not_equal, not_equal_check)
        return equal

    # -- gadgets/random_access.rs, gates/random_access.rs ------------------------------------------
    def _ra_shape(self, bits):
        """RandomAccessGate::new_from_config -- UNPINNED (recollection): (copies, extra constants)."""
        vec = 1 << bits
        copies = min(NUM_ROUTED // (2 + vec), self.num_wires // (2 + vec + bits))
        return copies, min(NUM_ROUTED - (2 + vec) * copies, NUM_CONSTANTS)

    def random_access(self, index, v):
        """UNPINNED (recollection of plonky2 0.2.2): a copy of a RandomAccessGate row shared per `bits` until it is full
        (find_slot); a fresh virtual target, connected to the claimed-element wire, is returned."""
        v = list(v)
        bits = (len(v) - 1).bit_length()
        assert len(v) == 1 << bits, "random_access: the list's length must be a power of two"
        if len(v) == 1:
            return v[0]
        r = self.free_ra.get(bits)
        copies, extra = self._ra_shape(bits)
        if r is None or len(self.rows[r]["copies"]) == copies:
            r = len(self.rows)
            self.rows.append({"kind": "ra", "bits": bits, "num_copies": copies, "extra": extra, "copies": []})
            self.free_ra[bits] = r
        claimed = self.add_virtual_target()
        self.rows[r]["copies"].append((index, claimed, v))
        self.events.append(("ra", index, v, claimed))
        return claimed

    # -- gadgets/split_join.rs ----------------------------------------------------------------------
    def _base_sum_row(self, num_limbs):
        row = {"kind": "basesum", "L": num_limbs, "sum": self.add_virtual_target(),
               "limbs": [self.add_virtual_target() for _ in range(num_limbs)]}
        self.rows.append(row)
        return row

    def split_le(self, integer, num_bits):
        if num_bits == 0:
            return []
        k = -(-num_bits // BASE_SUM_LIMBS)
        gates = [self._base_sum_row(BASE_SUM_LIMBS) for _ in range(k)]
        bits = [t for g in gates for t in g["limbs"]]
        for b in bits[num_bits:]:
            self.assert_zero(b)
        bits = bits[:num_bits]
        acc = self.zero()
        for g in reversed(gates):
            acc = self.mul_const_add(pow(2, BASE_SUM_LIMBS, P), acc, g["sum"])
        self.connect(acc, integer)
        self.events.append(("split", integer, gates))
        return bits

    def le_sum(self, bits):
        bits = list(bits)
        n = len(bits)
        if n == 0:
            return self.zero()
        if n - 1 <= NUM_OPS:
            s = bits[-1]
            for b in reversed(bits[:-1]):
                s = self.mul_add(self.two(), s, b)
            return s
        row = self._base_sum_row(n)
        for b, l in zip(bits, row["limbs"]):
            self.connect(b, l)
        self.events.append(("lesum", row))
        return row["sum"]

    # -- plonky2_ecdsa/biguint/gadgets/arithmetic_u32.rs: a U32Target is a target that is assumed to hold 32 bits ------------
    def u32_gate_ops(self, kind, num_addends=0):
        """Operations per row: U32ArithmeticGate::num_ops (gates/arithmetic_u32.rs:39-42: 6 routed wires and 32 two-bit limbs
        per op), U32AddManyGate::num_ops (add_many_u32.rs:43-48: num_addends + 3 routed, 18 limbs), U32SubtractionGate::num_ops
        (subtraction_u32.rs:39-43: 5 routed, 16 limbs).  135 wires: 3 / 135 // (a + 21) / 6; 234 wires: 6 / min(234 // (a + 21),
        80 // (a + 3)) / 11."""
        routed, limbs = {"u32arith": (6, 32), "u32addmany": (num_addends + 3, 18), "u32sub": (5, 16)}[kind]
        return min(self.num_wires // (routed + limbs), NUM_ROUTED // routed)

    def _u32_slot(self, kind, num_addends=0):
        """circuit_builder.rs `find_slot(gate, params, constants)` -- UNPINNED (recollection of plonky2 0.2.2, restated as
        `random_access` restates it): one open row per (gate, params) until it is full.  The operations of a shared row that
        nobody takes stay unconnected: their wires are what the gate's generator derives from zeros (build() fills them so, and
        so does the device: an op without a slot is left to fill_witness)."""
        key = (kind, num_addends)
        r = self.free_u32.get(key)
        if r is None or len(self.rows[r]["ops"]) == self.rows[r]["num_ops"]:
            r = len(self.rows)
            self.rows.append({"kind": kind, "na": num_addends, "num_ops": self.u32_gate_ops(kind, num_addends), "ops": []})
            self.free_u32[key] = r
        return self.rows[r]

    def add_virtual_u32_target(self):
        """arithmetic_u32.rs:79-81"""
        return self.add_virtual_target()

    def add_virtual_u32_targets(self, n):
        """arithmetic_u32.rs:83-88"""
        return [self.add_virtual_target() for _ in range(n)]

    def constant_u32(self, c):
        """arithmetic_u32.rs:91-93"""
        assert 0 <= c <= U32_MAX
        return self.constant(c)

    def zero_u32(self):
        """arithmetic_u32.rs:95-97"""
        return self.zero()

    def one_u32(self):
        """arithmetic_u32.rs:99-101"""
        return self.one()

    def connect_u32(self, x, y):
        """arithmetic_u32.rs:103-105"""
        self.connect(x, y)

    def assert_zero_u32(self, x):
        """arithmetic_u32.rs:107-109"""
        self.assert_zero(x)

    def assert_one(self, x):
        """circuit_builder.rs assert_one (biguint.rs:259 calls it)"""
        self.connect(x, self.one())

    def target_as_constant(self, t):
        """circuit_builder.rs target_as_constant: the constant of a target `constant()` returned, else None."""
        return self.const_of.get(t)

    def arithmetic_u32_special_cases(self, x, y, z):
        """arithmetic_u32.rs:114-138: all three constant -> the two halves of x * y + z as constants, no gate."""
        kx, ky, kz = self.target_as_constant(x), self.target_as_constant(y), self.target_as_constant(z)
        if kx is None or ky is None or kz is None:
            return None
        total = (kx * ky + kz) % P
        return self.constant_u32(total & U32_MAX), self.constant_u32(total >> 32)

    def mul_add_u32(self, x, y, z):
        """arithmetic_u32.rs:141-157: (low, high) of x * y + z in a U32ArithmeticGate operation."""
        special = self.arithmetic_u32_special_cases(x, y, z)
        if special is not None:
            return special
        row = self._u32_slot("u32arith")
        low, high = self.add_virtual_target(), self.add_virtual_target()
        row["ops"].append((x, y, z, low, high))
        self.events.append(("u32arith", x, y, z, low, high))
        return low, high

    def add_u32(self, a, b):
        """arithmetic_u32.rs:159-162"""
        return self.mul_add_u32(a, self.one_u32(), b)

    def _add_many_gate(self, to_add, carry):
        if len(to_add) > MAX_NUM_ADDENDS:
            raise ValueError("U32AddManyGate: %d addends, MAX_NUM_ADDENDS is %d" % (len(to_add), MAX_NUM_ADDENDS))
        row = self._u32_slot("u32addmany", len(to_add))
        result, out_carry = self.add_virtual_target(), self.add_virtual_target()
        row["ops"].append(tuple(to_add) + (carry, result, out_carry))
        self.events.append(("u32addmany", tuple(to_add), carry, result, out_carry))
        return result, out_carry

    def add_many_u32(self, to_add):
        """arithmetic_u32.rs:164-190: no gate for 0 or 1 addends, add_u32 for 2, else a U32AddManyGate operation per distinct
        number of addends (find_slot's params), its carry wire tied to zero."""
        to_add = list(to_add)
        if len(to_add) == 0:
            return self.zero_u32(), self.zero_u32()
        if len(to_add) == 1:
            return to_add[0], self.zero_u32()
        if len(to_add) == 2:
            return self.add_u32(to_add[0], to_add[1])
        return self._add_many_gate(to_add, self.zero())

    def add_u32s_with_carry(self, to_add, carry):
        """arithmetic_u32.rs:192-218.  An empty `to_add` is a U32AddManyGate { num_addends: 0 } operation, result = carry, as
        upstream places it (mul_biguint by a target without limbs: div_rem_biguint with b_len > a_len + 1)."""
        to_add = list(to_add)
        if len(to_add) == 1:
            return self.add_u32(to_add[0], carry)
        return self._add_many_gate(to_add, carry)

    def mul_u32(self, a, b):
        """arithmetic_u32.rs:220-223"""
        return self.mul_add_u32(a, b, self.zero_u32())

    def sub_u32(self, x, y, borrow):
        """arithmetic_u32.rs:226-241: (x - y - borrow mod 2^32, the borrow out) in a U32SubtractionGate operation."""
        row = self._u32_slot("u32sub")
        result, out_borrow = self.add_virtual_target(), self.add_virtual_target()
        row["ops"].append((x, y, borrow, result, out_borrow))
        self.events.append(("u32sub", x, y, borrow, result, out_borrow))
        return result, out_borrow

    def range_check_u32(self, vals):
        """gadgets/range_check_u32.rs:9-20: one U32RangeCheckGate row (add_gate: never shared) over all of `vals`."""
        vals = list(vals)
        if 17 * len(vals) > self.num_wires:
            raise ValueError("U32RangeCheckGate: %d limbs need %d wires" % (len(vals), 17 * len(vals)))
        self.rows.append({"kind": "u32range", "limbs": vals})
        self.events.append(("u32range", tuple(vals)))

    # -- gadgets/multiple_comparison.rs ------------------------------------------------------------------------------------
    def list_le(self, a, b, num_bits):
        """multiple_comparison.rs:15-66: a <= b as little-endian lists of `num_bits`-bit limbs: per limb two ComparisonGate rows
        (add_gate: never shared) with chunk_bits = 2, then mul, sub, mul_add.  The result is boolean by construction."""
        a, b = list(a), list(b)
        assert len(a) == len(b), "Comparison must be between same number of inputs and outputs"
        num_chunks = -(-num_bits // 2)
        one = self.one()
        result = one
        for x, y in zip(a, b):
            res = []
            for first, second in ((x, y), (y, x)):
                out = self.add_virtual_target()
                self.rows.append({"kind": "cmp", "bits": num_bits, "chunks": num_chunks, "a": first, "b": second, "res": out})
                self.events.append(("cmp", first, second, out))
                res.append(out)
            a_le_b, b_le_a = res
            these_limbs_equal = self.mul(a_le_b, b_le_a)
            these_limbs_less_than = self.sub(one, b_le_a)
            result = self.mul_add(these_limbs_equal, result, these_limbs_less_than)
        return result

    def list_le_u32(self, a, b):
        """multiple_comparison.rs:69-78"""
        return self.list_le(a, b, 32)

    # -- plonky2_ecdsa/biguint/biguint.rs: a BigUintTarget is the list of its U32Target limbs, least significant first ------
    def constant_biguint(self, value):
        """biguint.rs:81-86 (`to_u32_digits`: zero has no limbs)"""
        limbs = []
        while value:
            limbs.append(self.constant_u32(value & U32_MAX))
            value >>= 32
        return limbs

    def zero_biguint(self):
        """biguint.rs:88-90"""
        return self.constant_biguint(0)

    def connect_biguint(self, lhs, rhs):
        """biguint.rs:92-104: the common limbs are connected, the others are zero."""
        m = min(len(lhs), len(rhs))
        for x, y in zip(lhs[:m], rhs[:m]):
            self.connect_u32(x, y)
        for x in lhs[m:] + rhs[m:]:
            self.assert_zero_u32(x)

    def pad_biguints(self, a, b):
        """biguint.rs:106-126"""
        n = max(len(a), len(b))
        return list(a) + [self.zero_u32()] * (n - len(a)), list(b) + [self.zero_u32()] * (n - len(b))

    def cmp_biguint(self, a, b):
        """biguint.rs:128-132: a <= b"""
        a, b = self.pad_biguints(a, b)
        return self.list_le_u32(a, b)

    def add_virtual_biguint_target(self, num_limbs):
        """biguint.rs:134-138"""
        return self.add_virtual_u32_targets(num_limbs)

    def add_biguint(self, a, b):
        """biguint.rs:140-162: max(len) + 1 limbs"""
        out, carry = [], self.zero_u32()
        for i in range(max(len(a), len(b))):
            x = a[i] if i < len(a) else self.zero_u32()
            y = b[i] if i < len(b) else self.zero_u32()
            limb, carry = self.add_many_u32([carry, x, y])
            out.append(limb)
        return out + [carry]

    def sub_biguint(self, a, b):
        """biguint.rs:164-181: a - b for a >= b (the last borrow is not constrained, as upstream)"""
        a, b = self.pad_biguints(a, b)
        out, borrow = [], self.zero_u32()
        for x, y in zip(a, b):
            limb, borrow = self.sub_u32(x, y, borrow)
            out.append(limb)
        return out

    def mul_biguint(self, a, b):
        """biguint.rs:183-207: len(a) + len(b) + 1 limbs"""
        to_add = [[] for _ in range(len(a) + len(b))]
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                product, carry = self.mul_u32(x, y)
                to_add[i + j].append(product)
                to_add[i + j + 1].append(carry)
        out, carry = [], self.zero_u32()
        for summands in to_add:
            limb, carry = self.add_u32s_with_carry(summands, carry)
            out.append(limb)
        return out + [carry]

    def mul_biguint_by_bool(self, a, b):
        """biguint.rs:209-219"""
        return [self.mul(l, b) for l in a]

    def mul_add_biguint(self, x, y, z):
        """biguint.rs:221-229"""
        return self.add_biguint(self.mul_biguint(x, y), z)

    def div_rem_biguint(self, a, b):
        """biguint.rs:231-262: (div, rem) from the BigUintDivRemGenerator (event "divrem": no gate's own), then
        a == div * b + rem and rem <= b as upstream states it."""
        a, b = list(a), list(b)
        div = self.add_virtual_biguint_target(0 if len(b) > len(a) + 1 else len(a) - len(b) + 1)
        rem = self.add_virtual_biguint_target(len(b))
        self.events.append(("divrem", tuple(a), tuple(b), tuple(div), tuple(rem)))
        div_b_plus_rem = self.add_biguint(self.mul_biguint(div, b), rem)
        self.connect_biguint(a, div_b_plus_rem)
        self.assert_one(self.cmp_biguint(rem, b))
        return div, rem

    def div_biguint(self, a, b):
        """biguint.rs:264-267"""
        return self.div_rem_biguint(a, b)[0]

    def rem_biguint(self, a, b):
        """biguint.rs:269-272"""
        return self.div_rem_biguint(a, b)[1]

    @staticmethod
    def divrem_values(a_limbs, b_limbs, div_limbs, rem_limbs):
        """BigUintDivRemGenerator::run_once (biguint.rs:337-344) on limb values: a and b are the integers sum limb_i 2^(32 i)
        over the canonical limb values (`get_biguint_target`: a limb >= 2^32 carries into the next), (div, rem) = divmod(a, b)
        as `div_limbs` and `rem_limbs` 32-bit digits.  ValueError where upstream panics: b = 0, or more digits than limbs."""
        a = sum(v << (32 * i) for i, v in enumerate(a_limbs))
        b = sum(v << (32 * i) for i, v in enumerate(b_limbs))
        if b == 0:
            raise ValueError("unsatisfiable: div_rem_biguint divides by zero")
        q, r = divmod(a, b)
        if q >> (32 * div_limbs) or r >> (32 * rem_limbs):
            raise ValueError("unsatisfiable: div_rem_biguint: the quotient or the remainder has more digits than its target has limbs")
        return ([(q >> (32 * i)) & U32_MAX for i in range(div_limbs)], [(r >> (32 * i)) & U32_MAX for i in range(rem_limbs)])

    # -- plonky2_ecdsa/biguint/gadgets/nonnative.rs: a NonNativeTarget<FF> is the list of its limbs, as a BigUintTarget is; FF is
    # the `field` argument, a name of NONNATIVE_FIELDS ---------------------------------------------------------------------
    @staticmethod
    def nonnative_order(field):
        """FF::order()"""
        return NONNATIVE_FIELDS[field][1]

    @staticmethod
    def num_nonnative_limbs(field):
        """nonnative.rs:127-129: ceil_div_usize(FF::BITS, 32)"""
        return -(-NONNATIVE_FIELDS[field][1].bit_length() // 32)

    def biguint_to_nonnative(self, x, field):
        """nonnative.rs:131-136"""
        return list(x)

    def nonnative_to_canonical_biguint(self, x, field):
        """nonnative.rs:138-143"""
        return list(x)

    def constant_nonnative(self, x, field):
        """nonnative.rs:145-148: `x` an element of the field, as a Python integer"""
        assert 0 <= x < self.nonnative_order(field)
        return self.biguint_to_nonnative(self.constant_biguint(x), field)

    def zero_nonnative(self, field):
        """nonnative.rs:150-152"""
        return self.constant_nonnative(0, field)

    def connect_nonnative(self, lhs, rhs, field):
        """nonnative.rs:155-161: both assumed to be in reduced form"""
        self.connect_biguint(lhs, rhs)

    def add_virtual_nonnative_target(self, field):
        """nonnative.rs:163-171"""
        return self.add_virtual_biguint_target(self.num_nonnative_limbs(field))

    def add_virtual_nonnative_target_sized(self, num_limbs, field):
        """nonnative.rs:173-183"""
        return self.add_virtual_biguint_target(num_limbs)

    def add_nonnative(self, a, b, field):
        """nonnative.rs:185-215: (sum, overflow) from the NonNativeAdditionGenerator (event "nnadd": no gate's own), then
        a + b == sum + overflow * modulus and sum <= modulus (`cmp_biguint` is <=: sum = modulus passes, as upstream)."""
        a, b = list(a), list(b)
        total = self.add_virtual_nonnative_target(field)
        overflow = self.add_virtual_bool_target_unsafe()
        self.events.append(("nnadd", tuple(a), tuple(b), tuple(total), (overflow,), field))
        sum_expected = self.add_biguint(a, b)
        modulus = self.constant_biguint(self.nonnative_order(field))
        mod_times_overflow = self.mul_biguint_by_bool(modulus, overflow)
        sum_actual = self.add_biguint(total, mod_times_overflow)
        self.connect_biguint(sum_expected, sum_actual)
        self.connect(self.cmp_biguint(total, modulus), self.one())
        return total

    def mul_nonnative_by_bool(self, a, b, field):
        """nonnative.rs:217-226"""
        return self.mul_biguint_by_bool(a, b)

    def if_nonnative(self, b, x, y, field):
        """nonnative.rs:228-238"""
        not_b = self.not_(b)
        maybe_x = self.mul_nonnative_by_bool(x, b, field)
        maybe_y = self.mul_nonnative_by_bool(y, not_b, field)
        return self.add_nonnative(maybe_x, maybe_y, field)

    def sub_nonnative(self, a, b, field):
        """nonnative.rs:284-310: (diff, overflow) from the NonNativeSubtractionGenerator (event "nnsub"), diff's limbs range-checked
        in one U32RangeCheckGate row, overflow a bit, then a == diff + b - overflow * modulus."""
        a, b = list(a), list(b)
        diff = self.add_virtual_nonnative_target(field)
        overflow = self.add_virtual_bool_target_unsafe()
        self.events.append(("nnsub", tuple(a), tuple(b), tuple(diff), (overflow,), field))
        self.range_check_u32(diff)
        self.assert_bool(overflow)
        diff_plus_b = self.add_biguint(diff, b)
        modulus = self.constant_biguint(self.nonnative_order(field))
        mod_times_overflow = self.mul_biguint_by_bool(modulus, overflow)
        diff_plus_b_reduced = self.sub_biguint(diff_plus_b, mod_times_overflow)
        self.connect_biguint(a, diff_plus_b_reduced)
        return diff

    def mul_nonnative(self, a, b, field):
        """nonnative.rs:312-341: (prod, overflow) from the NonNativeMultiplicationGenerator (event "nnmul"), both range-checked,
        then a * b == prod + modulus * overflow.  overflow has len(a) + len(b) - 8 limbs (fewer than 8 operand limbs in all
        underflow upstream: ValueError).  A range check over no limbs (len(a) + len(b) == 8) places no row here: upstream's
        U32RangeCheckGate { num_input_limbs: 0 } constrains nothing and the gate table takes 1 limb at least."""
        a, b = list(a), list(b)
        prod = self.add_virtual_nonnative_target(field)
        modulus = self.constant_biguint(self.nonnative_order(field))
        if len(a) + len(b) < len(modulus):
            raise ValueError("mul_nonnative: %d + %d operand limbs are fewer than the modulus has" % (len(a), len(b)))
        overflow = self.add_virtual_biguint_target(len(a) + len(b) - len(modulus))
        self.events.append(("nnmul", tuple(a), tuple(b), tuple(prod), tuple(overflow), field))
        self.range_check_u32(prod)
        if overflow:
            self.range_check_u32(overflow)
        prod_expected = self.mul_biguint(a, b)
        mod_times_overflow = self.mul_biguint(modulus, overflow)
        prod_actual = self.add_biguint(prod, mod_times_overflow)
        self.connect_biguint(prod_expected, prod_actual)
        return prod

    def mul_many_nonnative(self, to_mul, field):
        """nonnative.rs:343-356"""
        to_mul = list(to_mul)
        if len(to_mul) == 1:
            return to_mul[0]
        acc = self.mul_nonnative(to_mul[0], to_mul[1], field)
        for t in to_mul[2:]:
            acc = self.mul_nonnative(acc, t, field)
        return acc

    def neg_nonnative(self, x, field):
        """nonnative.rs:358-363: zero minus x, the zero a target without limbs"""
        zero_ff = self.biguint_to_nonnative(self.constant_biguint(0), field)
        return self.sub_nonnative(zero_ff, x, field)

    def inv_nonnative(self, x, field):
        """nonnative.rs:365-389: (inv, div) from the NonNativeInverseGenerator (event "nninv"), both with x's limbs, then
        x * inv == modulus * div + 1."""
        x = list(x)
        inv = self.add_virtual_biguint_target(len(x))
        div = self.add_virtual_biguint_target(len(x))
        self.events.append(("nninv", tuple(x), (), tuple(inv), tuple(div), field))
        product = self.mul_biguint(x, inv)
        modulus = self.constant_biguint(self.nonnative_order(field))
        mod_times_div = self.mul_biguint(modulus, div)
        expected_product = self.add_biguint(mod_times_div, self.constant_biguint(1))
        self.connect_biguint(product, expected_product)
        return inv

    def reduce(self, x, field):
        """nonnative.rs:391-401: x % |FF| through `rem_biguint`"""
        return self.rem_biguint(x, self.constant_biguint(self.nonnative_order(field)))

    def reduce_nonnative(self, x, field):
        """nonnative.rs:403-406"""
        return self.reduce(self.nonnative_to_canonical_biguint(x, field), field)

    def bool_to_nonnative(self, b, field):
        """nonnative.rs:408-416: one limb"""
        return [b]

    def split_nonnative_to_bits(self, x, field):
        """nonnative.rs:418-430: 32 bits per limb, least significant first"""
        return [bit for limb in x for bit in self.split_le(limb, 32)]

    def nonnative_conditional_neg(self, x, b, field):
        """nonnative.rs:432-443"""
        not_b = self.not_(b)
        neg = self.neg_nonnative(x, field)
        x_if_true = self.mul_nonnative_by_bool(neg, b, field)
        x_if_false = self.mul_nonnative_by_bool(x, not_b, field)
        return self.add_nonnative(x_if_true, x_if_false, field)

    @staticmethod
    def nonnative_values(event, field, a_limbs, b_limbs, first_limbs, second_limbs):
        """The four generators' run_once (nonnative.rs:469-484, :589-604, :645-658, :691-703) on limb values: A and B are the
        operands' integers sum limb_i 2^(32 i) (`get_biguint_target`) reduced modulo the order (FF::from_noncanonical_biguint).
        Returns the two targets' 32-bit digits.  ValueError where upstream panics: the inverse of zero, or more digits than limbs
        (`set_biguint_target`)."""
        m = NONNATIVE_FIELDS[field][1]
        a = sum(v << (32 * i) for i, v in enumerate(a_limbs)) % m
        b = sum(v << (32 * i) for i, v in enumerate(b_limbs)) % m
        if event == "nnadd":
            s = a + b
            first, second = (s - m, 1) if s > m else (s, 0)          # (strictly: a + b == m leaves sum = m)
        elif event == "nnsub":
            first, second = (a - b, 0) if a >= b else (m + a - b, 1)
        elif event == "nnmul":
            second, first = divmod(a * b, m)
        else:
            if a == 0:
                raise ValueError("unsatisfiable: inv_nonnative inverts zero")
            first = pow(a, -1, m)
            second = a * first // m
        if first >> (32 * first_limbs) or second >> (32 * second_limbs):
            raise ValueError("unsatisfiable: a nonnative generator's value has more digits than its target has limbs")
        return ([(first >> (32 * i)) & U32_MAX for i in range(first_limbs)], [(second >> (32 * i)) & U32_MAX for i in range(second_limbs)])

    # -- build(): rows -> blob (library) + witness ----------------------------------------------------
    def _layout(self):
        """The circuit half of build(): rows -> blob, and the cells of every copy class.  Runs once; build(), seed_cells() and
        seed_values() share its result."""
        if self._lay is not None:
            return self._lay
        zero = self.zero()
        # fill_batched_gates: the unused copies of a RandomAccess row read position `zero` of a list of `zero`s into a fresh
        # claimed element
        for g in self.rows:
            if g["kind"] == "ra":
                while len(g["copies"]) < g["num_copies"]:
                    claimed = self.add_virtual_target()
                    lst = [zero] * (1 << g["bits"])
                    g["copies"].append((zero, claimed, lst))
                    self.events.append(("ra", zero, lst, claimed))
        # circuit_builder.rs build(): the public inputs are hashed IN CIRCUIT -- hash_n_to_hash_no_pad::<PoseidonHash>, an
        # overwrite-mode sponge: one PoseidonGate row per 8 inputs, swap wire tied to zero, the state starts as twelve copies of
        # `zero` -- and the first four outputs are routed to a PublicInputGate added right behind; no public inputs: the hash is
        # four copies of `zero` and no PoseidonGate exists (the reference's basic_div / basic_if circuits show both cases)
        state = [zero] * 12
        for off in range(0, len(self.public_inputs), 8):
            chunk = self.public_inputs[off:off + 8]
            state = list(chunk) + state[len(chunk):]
            row = {"kind": "poseidon", "in": state, "out": [self.add_virtual_target() for _ in range(12)], "swap": zero}
            self.rows.append(row)
            self.events.append(("poseidon", row))
            state = row["out"]
        pi_hash = state[:4]
        rows = list(self.rows)
        pi_row = len(rows)
        # ConstantGate rows: plonky2 walks constants_to_targets sorted by the constant's canonical value, two per gate (both
        # reference circuits: 0, 1 | 2^63, p - 1 and 0, 1 | p - 1, -)
        # UNPINNED (recollected rule of build()): in that order the constants go first to the extra-constant wires of the gates
        # that have some (RandomAccessGate), rows in creation order, and only the rest to ConstantGate rows
        const_list = sorted(self.consts.items())
        extra_wires = [(r, i) for r, g in enumerate(rows) if g["kind"] == "ra" for i in range(g["extra"])]
        extra_consts, const_list = const_list[:len(extra_wires)], const_list[len(extra_wires):]
        const_rows = (len(const_list) + 1) // 2
        used = pi_row + 1 + const_rows
        d = max(2, (used - 1).bit_length())
        n = 1 << d
        # gate set, sorted by (degree, id) like CommonCircuitData.gates
        kinds = {("noop",)} if used < n else set()
        kinds |= {("const",), ("pi",)} if const_rows else {("pi",)}
        def gate_key(g):
            k = g["kind"]
            return ((k, g["bits"]) if k == "ra" else ("basesum", g["L"]) if k == "basesum" else (k, g["na"]) if k == "u32addmany" else
                    (k, len(g["limbs"])) if k == "u32range" else (k, g["bits"], g["chunks"]) if k == "cmp" else (k,))

        for r in rows:
            kinds.add(gate_key(r))
        spec = {("noop",): (0, "NoopGate", (G_NOOP, (0, 0, 0, 0), 0, 0)),
                ("const",): (1, "ConstantGate { num_consts: 2 }", (G_CONSTANT, (2, 0, 0, 0), 1, 2)),
                ("pi",): (1, "PublicInputGate", (G_PUBLIC_INPUT, (0, 0, 0, 0), 1, 0)),
                ("arith",): (3, "ArithmeticGate { num_ops: 20 }", (G_ARITHMETIC, (NUM_OPS, 0, 0, 0), 3, 2)),
                ("poseidon",): (7, "PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=12>",
                                (G_POSEIDON, (0, 0, 0, 0), 7, 0))}
        for k in kinds:
            if k[0] == "basesum":
                spec[k] = (2, "BaseSumGate { num_limbs: %d } + Base: 2" % k[1], (G_BASE_SUM, (2, k[1], 0, 0), 2, 0))
            elif k[0] == "ra":
                # UNPINNED: the id as plonky2 0.2.2 prints it, format!("{self:?}<D={D}>"), as recollected
                copies, extra = self._ra_shape(k[1])
                spec[k] = (k[1] + 1, "RandomAccessGate { bits: %d, num_copies: %d, num_extra_constants: %d, _phantom: "
                           "PhantomData<plonky2_field::goldilocks_field::GoldilocksField> }<D=2>" % (k[1], copies, extra),
                           (G_RANDOM_ACCESS, (k[1], copies, extra, 0), k[1] + 1, extra))
            # the five gates of plonky2_ecdsa/biguint/gates: id() = format!("{self:?}") (ComparisonGate: + "<D=2>"), degree
            # 1 << limb_bits = 4 (range check: BASE = 4; comparison: 1 << chunk_bits), no constants
            elif k[0] == "u32arith":
                ops = self.u32_gate_ops("u32arith")
                spec[k] = (4, "U32ArithmeticGate { num_ops: %d, %s }" % (ops, _PHANTOM), (G_U32_ARITHMETIC, (ops, 0, 0, 0), 4, 0))
            elif k[0] == "u32addmany":
                ops = self.u32_gate_ops("u32addmany", k[1])
                spec[k] = (4, "U32AddManyGate { num_addends: %d, num_ops: %d, %s }" % (k[1], ops, _PHANTOM),
                           (G_U32_ADD_MANY, (k[1], ops, 0, 0), 4, 0))
            elif k[0] == "u32sub":
                ops = self.u32_gate_ops("u32sub")
                spec[k] = (4, "U32SubtractionGate { num_ops: %d, %s }" % (ops, _PHANTOM), (G_U32_SUBTRACTION, (ops, 0, 0, 0), 4, 0))
            elif k[0] == "u32range":
                spec[k] = (4, "U32RangeCheckGate { num_input_limbs: %d, %s }" % (k[1], _PHANTOM), (G_U32_RANGE_CHECK, (k[1], 0, 0, 0), 4, 0))
            elif k[0] == "cmp":
                chunk_bits = -(-k[1] // k[2])
                spec[k] = (1 << chunk_bits, "ComparisonGate { num_bits: %d, num_chunks: %d, %s }<D=2>" % (k[1], k[2], _PHANTOM),
                           (G_COMPARISON, (k[1], k[2], 0, 0), 1 << chunk_bits, 0))
        order = sorted(kinds, key=lambda k: (spec[k][0], spec[k][1]))
        index = {k: i for i, k in enumerate(order)}
        gates = [spec[k][2] for k in order]
        row_gate = np.zeros(n, dtype=np.uint32)
        row_consts = np.zeros((2, n), dtype=np.uint64)
        cells = {}                                  # class root -> [(row, col)]

        def put(t, r, c):
            cells.setdefault(self.find(t), []).append((r, c))

        for r, g in enumerate(rows):
            if g["kind"] == "arith":
                row_gate[r] = index[("arith",)]
                row_consts[0, r], row_consts[1, r] = g["c"]
                for k, op in enumerate(g["ops"]):
                    for j, t in enumerate(op):
                        put(t, r, 4 * k + j)
            elif g["kind"] == "poseidon":
                row_gate[r] = index[("poseidon",)]
                g["row"] = r
                for j, t in enumerate(g["in"]):
                    put(t, r, j)
                for j, t in enumerate(g["out"]):
                    put(t, r, 12 + j)
                put(g["swap"], r, 24)
            elif g["kind"] == "ra":
                row_gate[r] = index[("ra", g["bits"])]
                g["row"] = r
                vec = 1 << g["bits"]
                for k, (idx, claimed, lst) in enumerate(g["copies"]):
                    put(idx, r, (2 + vec) * k)
                    put(claimed, r, (2 + vec) * k + 1)
                    for j, t in enumerate(lst):
                        put(t, r, (2 + vec) * k + 2 + j)
            elif g["kind"] == "basesum":
                row_gate[r] = index[("basesum", g["L"])]
                put(g["sum"], r, 0)
                for j, t in enumerate(g["limbs"]):
                    put(t, r, 1 + j)
            else:
                # the five gates of plonky2_ecdsa/biguint/gates: an operation's routed wires follow each other (arithmetic_u32.rs
                # :44-69 six per op, add_many_u32.rs:50-70 addends, carry, result, carry out, subtraction_u32.rs:45-65 five per op)
                row_gate[r] = index[gate_key(g)]
                g["row"] = r
                if g["kind"] == "u32range":          # range_check_u32.rs:40-43
                    for j, t in enumerate(g["limbs"]):
                        put(t, r, j)
                elif g["kind"] == "cmp":             # comparison.rs:52-62
                    put(g["a"], r, 0)
                    put(g["b"], r, 1)
                    put(g["res"], r, 2)
                else:
                    stride = 6 if g["kind"] == "u32arith" else 5 if g["kind"] == "u32sub" else g["na"] + 3
                    for k, op in enumerate(g["ops"]):
                        for j, t in enumerate(op):
                            put(t, r, stride * k + j)
        row_gate[pi_row] = index[("pi",)]
        for i in range(4):                          # (no public inputs: four copies of `zero`)
            put(pi_hash[i], pi_row, i)
        for (c, t), (r, i) in zip(extra_consts, extra_wires):
            row_consts[i, r] = c
            put(t, r, (2 + (1 << rows[r]["bits"])) * rows[r]["num_copies"] + i)
        for i, (c, t) in enumerate(const_list):
            r = pi_row + 1 + i // 2
            row_gate[r] = index[("const",)]
            row_consts[i % 2, r] = c
            put(t, r, i % 2)
        if const_rows:
            row_gate[pi_row + 1:pi_row + 1 + const_rows] = index[("const",)]
        if used < n:
            row_gate[used:] = index[("noop",)]
        copies = []
        for cl in cells.values():
            for (r0, c0), (r1, c1) in zip(cl, cl[1:]):
                copies.append((r0, c0, r1, c1))
        blob = build_blob(d, gates, row_gate, row_consts, np.array(copies, dtype=np.uint32).reshape(-1, 4),
                          num_public_inputs=len(self.public_inputs), num_wires=self.num_wires)
        self.pi_row = pi_row
        self._lay = (blob, rows, pi_row, extra_consts + const_list, cells, n)
        return self._lay

    def build(self, witness_values):
        """witness_values: {target: value}.  Returns (blob, wires) for CircuitData(blob).prove(wires)."""
        blob, rows, pi_row, const_list, cells, n = self._layout()
        # witness: the generators, in creation order, until nothing changes
        val = {}
        for c, t in const_list:
            val[self.find(t)] = c
        for t, v in witness_values.items():
            rt = self.find(t)
            v %= P
            if rt in val and val[rt] != v:
                raise ValueError("witness value contradicts the circuit")
            val[rt] = v
        pending = list(self.events)
        while pending:
            rest = []
            for ev in pending:
                if ev[0] == "arith":
                    _, c0, c1, m0, m1, ad, out = ev
                    a = val.get(self.find(m0)) if c0 else 0
                    b = val.get(self.find(m1)) if c0 else 0
                    c = val.get(self.find(ad)) if c1 else 0
                    if a is None or b is None or c is None:
                        rest.append(ev)
                        continue
                    self._set(val, out, (c0 * a % P * b + c1 * c) % P)
                elif ev[0] == "poseidon":
                    ins = [val.get(self.find(t)) for t in ev[1]["in"]]
                    if any(v is None for v in ins):
                        rest.append(ev)
                        continue
                    ev[1]["wires"] = poseidon_gate_row(ins)
                    for j, t in enumerate(ev[1]["out"]):
                        self._set(val, t, int(ev[1]["wires"][12 + j]))
                elif ev[0] == "equal":
                    _, x, y, equal, inv = ev
                    a, b = val.get(self.find(x)), val.get(self.find(y))
                    if a is None or b is None:
                        rest.append(ev)
                        continue
                    self._set(val, equal, 1 if a == b else 0)
                    self._set(val, inv, pow((a - b) % P, P - 2, P))      # (0 when they are equal)
                elif ev[0] == "ra":
                    _, idx, lst, claimed = ev
                    vs = [val.get(self.find(t)) for t in [idx] + lst]
                    if any(v is None for v in vs):
                        rest.append(ev)
                        continue
                    if vs[0] >= len(lst):
                        raise ValueError("unsatisfiable: a random access reads position %d of %d" % (vs[0], len(lst)))
                    self._set(val, claimed, vs[1 + vs[0]])
                elif ev[0] in ("u32arith", "u32addmany", "u32sub", "u32range", "cmp", "divrem"):
                    ins = {"u32arith": ev[1:4], "u32sub": ev[1:4], "cmp": ev[1:3], "u32range": ev[1]}.get(ev[0])
                    if ev[0] == "u32addmany":
                        ins = ev[1] + (ev[2],)
                    elif ev[0] == "divrem":
                        ins = ev[1] + ev[2]
                    vs = [val.get(self.find(t)) for t in ins]
                    if any(v is None for v in vs):
                        rest.append(ev)
                        continue
                    if ev[0] == "u32arith":          # U32ArithmeticGenerator, arithmetic_u32.rs:376-426
                        o = (vs[0] * vs[1] + vs[2]) % P
                        self._set(val, ev[4], o & U32_MAX)
                        self._set(val, ev[5], o >> 32)
                    elif ev[0] == "u32addmany":      # U32AddManyGenerator, add_many_u32.rs:329-378
                        o = sum(vs) % P
                        self._set(val, ev[3], o & U32_MAX)
                        self._set(val, ev[4], o >> 32)
                    elif ev[0] == "u32sub":          # U32SubtractionGenerator, subtraction_u32.rs:298-343
                        init = (vs[0] - vs[1] - vs[2]) % P
                        borrow = 1 if init > 1 << 32 else 0
                        self._set(val, ev[4], (init + (borrow << 32)) % P)
                        self._set(val, ev[5], borrow)
                    elif ev[0] == "u32range":        # (no target is set; a limb of more than 32 bits has no two-bit limbs)
                        if any(v > U32_MAX for v in vs):
                            raise ValueError("unsatisfiable: a range-checked limb has more than 32 bits")
                    elif ev[0] == "cmp":             # ComparisonGenerator, comparison.rs:439-537
                        self._set(val, ev[3], 1 if vs[0] <= vs[1] else 0)
                    else:                            # BigUintDivRemGenerator, biguint.rs:337-344
                        _, a, b, div, rem = ev
                        q, r = self.divrem_values(vs[:len(a)], vs[len(a):], len(div), len(rem))
                        for t, v in zip(div + rem, q + r):
                            self._set(val, t, v)
                elif ev[0] in NONNATIVE_EVENTS:
                    _, a, b, first, second, field = ev
                    vs = [val.get(self.find(t)) for t in a + b]
                    if any(v is None for v in vs):
                        rest.append(ev)
                        continue
                    x, y = self.nonnative_values(ev[0], field, vs[:len(a)], vs[len(a):], len(first), len(second))
                    for t, v in zip(first + second, x + y):
                        self._set(val, t, v)
                elif ev[0] == "split":
                    v = val.get(self.find(ev[1]))
                    if v is None:
                        rest.append(ev)
                        continue
                    for g in ev[2]:
                        part = v & ((1 << g["L"]) - 1)
                        v >>= g["L"]
                        self._set(val, g["sum"], part)
                        for j, l in enumerate(g["limbs"]):
                            self._set(val, l, (part >> j) & 1)
                else:
                    bits = [val.get(self.find(l)) for l in ev[1]["limbs"]]
                    if any(b is None for b in bits):
                        rest.append(ev)
                        continue
                    self._set(val, ev[1]["sum"], sum(b << j for j, b in enumerate(bits)) % P)
            if len(rest) == len(pending):
                raise ValueError("witness generation is stuck: some inputs were not assigned")
            pending = rest
        W = self.num_wires
        wires = np.zeros((W, n), dtype=np.uint64)
        for g in rows:                              # the PoseidonGate's internal wires (deltas, S-box inputs): its generator's
            if g["kind"] == "poseidon":
                wires[:135, g["row"]] = g["wires"]
        for rt, cl in cells.items():
            v = val.get(rt)
            if v is None:
                # the dummy addend of a product-only op whose operand is otherwise unconstrained
                raise ValueError("a wire has no value")
            for (r, c) in cl:
                wires[c, r] = v
        for g in rows:                              # RandomAccessGenerator: the index bits, in the non-routed wires
            if g["kind"] == "ra":
                bits, vec = g["bits"], 1 << g["bits"]
                routed = (2 + vec) * g["num_copies"] + g["extra"]
                for k, (idx, _, _) in enumerate(g["copies"]):
                    for i in range(bits):
                        wires[routed + k * bits + i, g["row"]] = (val[self.find(idx)] >> i) & 1
        for g in rows:                              # the U32 and comparison rows: every operation's generator, the unused ones' too
            if g["kind"] in ("u32arith", "u32addmany", "u32sub", "u32range", "cmp"):
                self._fill_u32_row(wires, g)
        # circuit_builder.rs randomize_unused_pi_wires: every wire of the PublicInputGate row after the hash, routed
        # or not, gets a random value (so no wire column of a real witness is zero in every row)
        wires[4:NUM_ROUTED, pi_row] = self.rng.integers(0, P, size=NUM_ROUTED - 4, dtype=np.uint64)
        wires[NUM_ROUTED:, pi_row] = self.rng.integers(0, P, size=W - NUM_ROUTED, dtype=np.uint64)
        self.public_input_values = [val[self.find(t)] for t in self.public_inputs]
        self.values = val
        return blob, wires

    def _fill_u32_row(self, wires, g):
        """The row's generator(s) as the reference states them, on the row's routed inputs as they stand in `wires` (zeros for
        an operation nobody took): the outputs and the gate-internal columns -- two-bit limbs, the inverse of u32::MAX - high,
        the comparison's chunks, equalities, intermediate values and the bits of the most significant difference."""
        r = g["row"]

        def get(c):
            return int(wires[c, r])

        def limbs(base, v, count):
            for j in range(count):
                wires[base + j, r] = (v >> (2 * j)) & 3

        if g["kind"] == "u32arith":                  # arithmetic_u32.rs:376-426; wires :44-85
            ops = g["num_ops"]
            for i in range(ops):
                o = (get(6 * i) * get(6 * i + 1) + get(6 * i + 2)) % P
                low, high = o & U32_MAX, o >> 32
                wires[6 * i + 3, r], wires[6 * i + 4, r] = low, high
                wires[6 * i + 5, r] = pow(U32_MAX - high, P - 2, P)      # (0 when high is u32::MAX)
                limbs(6 * ops + 32 * i, o, 32)
        elif g["kind"] == "u32addmany":              # add_many_u32.rs:329-378; wires :50-86
            na, ops = g["na"], g["num_ops"]
            for i in range(ops):
                b = (na + 3) * i
                o = sum(get(b + j) for j in range(na + 1)) % P
                wires[b + na + 1, r], wires[b + na + 2, r] = o & U32_MAX, o >> 32
                limbs((na + 3) * ops + 18 * i, o & U32_MAX, 16)
                limbs((na + 3) * ops + 18 * i + 16, o >> 32, 2)
        elif g["kind"] == "u32sub":                  # subtraction_u32.rs:298-343; wires :45-79
            ops = g["num_ops"]
            for i in range(ops):
                init = (get(5 * i) - get(5 * i + 1) - get(5 * i + 2)) % P
                borrow = 1 if init > 1 << 32 else 0
                res = (init + (borrow << 32)) % P
                wires[5 * i + 3, r], wires[5 * i + 4, r] = res, borrow
                limbs(5 * ops + 16 * i, res, 16)
        elif g["kind"] == "u32range":                # range_check_u32.rs:198-220; wires :40-51
            nl = len(g["limbs"])
            for i in range(nl):
                limbs(nl + 16 * i, get(i) & U32_MAX, 16)
        else:                                        # comparison.rs:439-537; wires :52-96
            nb, nc = g["bits"], g["chunks"]
            cb = -(-nb // nc)
            a, b = get(0), get(1)
            wires[2, r] = 1 if a <= b else 0
            msd = 0
            for i in range(nc):
                f, s2 = (a >> (cb * i)) & ((1 << cb) - 1), (b >> (cb * i)) & ((1 << cb) - 1)
                wires[4 + i, r], wires[4 + nc + i, r] = f, s2
                wires[4 + 2 * nc + i, r] = 1 if f == s2 else pow((s2 - f) % P, P - 2, P)
                wires[4 + 3 * nc + i, r] = 1 if f == s2 else 0
                if f != s2:
                    msd = (s2 - f) % P
                    wires[4 + 4 * nc + i, r] = 0
                else:
                    wires[4 + 4 * nc + i, r] = msd
            wires[3, r] = msd
            v = ((1 << cb) + msd) % P
            for i in range(cb + 1):
                wires[4 + 5 * nc + i, r] = (v >> i) & 1

    # -- the witness on the GPU: what the caller still has to supply ------------------------------------
    def _seed_classes(self):
        """(cells, roots) of the seeds that carry a value of the program: one cell per copy class that holds no constant and
        no generator's output -- the targets `pw.set_target` is called on -- in the order of the classes' first targets."""
        _, _, _, _, cells, _ = self._layout()
        derived = {self.find(t) for t in self.const_of}
        # the operands of a div-rem generator are the program's when nothing created before it derives them: `div_rem_biguint`
        # connects a to div * b + rem afterwards, which compares (biguint.rs:254-256) and does not make `a` an output.  (A seed
        # names the first cell of its class: an operand that enters the circuit nowhere before div_rem_biguint has that result
        # column as its only cell, and the row op then shares the cell's writer bit with the seed -- DESIGN.md 11.6.)
        given = set()
        for ev in self.events:
            if ev[0] == "divrem" or ev[0] in NONNATIVE_EVENTS:     # (the nonnative gadgets connect their operands the same way)
                given.update(self.find(t) for t in ev[1] + ev[2] if self.find(t) not in derived)
            if ev[0] == "arith":
                derived.add(self.find(ev[6]))
            elif ev[0] == "poseidon":
                derived.update(self.find(t) for t in ev[1]["out"])
            elif ev[0] == "equal":
                derived.update((self.find(ev[3]), self.find(ev[4])))
            elif ev[0] == "ra":
                derived.add(self.find(ev[3]))
            elif ev[0] in ("u32arith", "u32sub"):
                derived.update((self.find(ev[4]), self.find(ev[5])))
            elif ev[0] == "u32addmany":
                derived.update((self.find(ev[3]), self.find(ev[4])))
            elif ev[0] == "cmp":
                derived.add(self.find(ev[3]))
            elif ev[0] == "divrem" or ev[0] in NONNATIVE_EVENTS:
                derived.update(self.find(t) for t in ev[3] + ev[4])
            elif ev[0] == "u32range":
                pass
            elif ev[0] == "split":
                assert len(ev[2]) == 1, "a split over several BaseSum rows spans rows: not a gate-local generator"
                derived.update(self.find(t) for t in ev[2][0]["limbs"])
            else:
                derived.add(self.find(ev[1]["sum"]))
        roots = sorted(rt for rt in cells if rt not in derived or rt in given)
        return [cells[rt][0] for rt in roots], roots

    def seed_cells(self):
        """[(row, col)] for CircuitData.witness_plan: the input classes, then every wire of the PublicInputGate row behind
        the public-input hash (build() fills those with random values: they are the caller's, not a generator's)."""
        cl, _ = self._seed_classes()
        return cl + [(self.pi_row, c) for c in range(4, self.num_wires)]

    def seed_values(self, witness_values):
        """The values of seed_cells(), without running build()'s event loop: witness_values {target: value} must name one
        target of every input class; the PublicInputGate row is drawn from the builder's generator as build() draws it."""
        _, roots = self._seed_classes()
        given = {}
        for t, v in witness_values.items():
            rt, v = self.find(t), v % P
            if given.setdefault(rt, v) != v:
                raise ValueError("witness value contradicts the circuit")
        missing = [rt for rt in roots if rt not in given]
        if missing:
            raise ValueError("witness generation is stuck: some inputs were not assigned")
        out = [given[rt] for rt in roots]
        out += [int(x) for x in self.rng.integers(0, P, size=NUM_ROUTED - 4, dtype=np.uint64)]
        out += [int(x) for x in self.rng.integers(0, P, size=self.num_wires - NUM_ROUTED, dtype=np.uint64)]
        return out

    def generators(self):
        """The generators that are no gate's own, for CircuitData.witness_plan(..., generators=): ("equality", (cell_x, cell_y,
        cell_equal, cell_inv)), ("biguint_divrem", (a_cells, b_cells, div_cells, rem_cells)) and, for the four nonnative
        generators, ("nonnative_add" | "_sub" | "_mul" | "_inv", (a_cells, b_cells, first target's cells, second target's cells),
        field name) in creation order; a target's cell -- a limb's too -- is the first cell of its copy class."""
        _, _, _, _, cells, _ = self._layout()
        out = []
        for ev in self.events:
            if ev[0] == "equal":
                cl = [cells.get(self.find(t)) for t in ev[1:]]
                if any(c is None for c in cl):
                    raise ValueError("is_equal: a target of the equality generator lies in no gate row")
                out.append(("equality", tuple(c[0] for c in cl)))
            elif ev[0] == "divrem":
                groups = [[cells.get(self.find(t)) for t in grp] for grp in ev[1:]]
                if any(c is None for grp in groups for c in grp):
                    raise ValueError("div_rem_biguint: a limb of the div-rem generator lies in no gate row")
                out.append(("biguint_divrem", tuple(tuple(c[0] for c in grp) for grp in groups)))
            elif ev[0] in NONNATIVE_EVENTS:
                groups = [[cells.get(self.find(t)) for t in grp] for grp in ev[1:5]]
                if any(c is None for grp in groups for c in grp):
                    raise ValueError("%s: a limb of the generator lies in no gate row" % NONNATIVE_EVENTS[ev[0]])
                out.append((NONNATIVE_EVENTS[ev[0]], tuple(tuple(c[0] for c in grp) for grp in groups), ev[5]))
        return out

    def _set(self, val, t, v):
        rt = self.find(t)
        if rt in val and val[rt] != v:
            raise ValueError("unsatisfiable: a generator contradicts an assigned value")
        val[rt] = v

    def value_of(self, t):
        return self.values[self.find(t)]


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
        for op in opcodes:
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
            else:
                raise NotImplementedError(op[0])

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
        """The generators that are no gate's own (the equality generators of the memory writes), for
        CircuitData.witness_plan(cells, generators=...) beside witness_seeds()."""
        return self.builder.generators()

    def blob(self):
        """The circuit blob alone (build() without the witness)."""
        return self.builder._layout()[0]

    def public_inputs(self):
        """Values of the registered public inputs, in order (after build): what p2gpu_prove takes beside the wires."""
        return list(self.builder.public_input_values)

    def witness_value(self, w):
        return self.builder.value_of(self.witness_target_map[w])
