"""The u32 gadgets of the reference's own tree (plonky2_ecdsa/biguint/gadgets/arithmetic_u32.rs `CircuitBuilderU32`,
range_check_u32.rs, multiple_comparison.rs) over its five gates (biguint/gates/*.rs: shapes, wire positions, degrees and ids are
read off that source, so they are pinned), as a mixin of builder.CircuitBuilder, with the gates' generators and row kinds.
A U32Target is a target that is assumed to hold 32 bits.  Only `find_slot`, plonky2's row sharing, is UNPINNED (see `_u32_op`)."""
from .builder import GENERATORS, NUM_ROUTED, P, ROW_KINDS, ROW_OPS, CircuitBuilder, Generator, GeneratorKind, RowKind, op_cells

G_U32_ARITHMETIC, G_U32_ADD_MANY, G_U32_SUBTRACTION, G_U32_RANGE_CHECK, G_COMPARISON = 7, 8, 9, 10, 11   # p2gpu.h gate kinds
MAX_NUM_ADDENDS, U32_MAX = 16, 0xFFFFFFFF      # gates/add_many_u32.rs:24
_PHANTOM = "_phantom: PhantomData<plonky2_field::goldilocks_field::GoldilocksField>"
# per gate with operations: (routed wires beside the addends, two-bit limbs) of one operation
_OP_SHAPE = {"u32arith": (6, 32), "u32addmany": (3, 18), "u32sub": (5, 16)}


def _halves(o):
    return [o & U32_MAX, o >> 32]


def _sub_u32(x, y, borrow):                          # U32SubtractionGenerator, subtraction_u32.rs:298-343
    init = (x - y - borrow) % P
    out_borrow = 1 if init > 1 << 32 else 0
    return [(init + (out_borrow << 32)) % P, out_borrow]


def _range_body(ev, vs):                             # (no target is set; a limb of more than 32 bits has no two-bit limbs)
    if any(v > U32_MAX for v in vs):
        raise ValueError("unsatisfiable: a range-checked limb has more than 32 bits")
    return []


GENERATORS.update({
    "u32arith": GeneratorKind(lambda ev, vs: _halves((vs[0] * vs[1] + vs[2]) % P)),      # U32ArithmeticGenerator, arithmetic_u32.rs:376-426
    "u32addmany": GeneratorKind(lambda ev, vs: _halves(sum(vs) % P)),                    # U32AddManyGenerator, add_many_u32.rs:329-378
    "u32sub": GeneratorKind(lambda ev, vs: _sub_u32(*vs)),
    "u32range": GeneratorKind(_range_body),
    "cmp": GeneratorKind(lambda ev, vs: [1 if vs[0] <= vs[1] else 0]),                   # ComparisonGenerator, comparison.rs:439-537
})


# -- the fills: a row's generator(s) as the reference states them, on its routed inputs as they stand in `wires` (zeros for an
# operation nobody took): the outputs and the gate-internal columns (two-bit limbs, inverses, the comparison's chunks and bits)
def _limbs(wires, r, base, v, count):
    for j in range(count):
        wires[base + j, r] = (v >> (2 * j)) & 3


def _fill_u32arith(wires, g):                        # arithmetic_u32.rs:376-426; wires :44-85
    r, ops = g["row"], g["num_ops"]
    for i in range(ops):
        o = (int(wires[6 * i, r]) * int(wires[6 * i + 1, r]) + int(wires[6 * i + 2, r])) % P
        low, high = _halves(o)
        wires[6 * i + 3, r], wires[6 * i + 4, r] = low, high
        wires[6 * i + 5, r] = pow(U32_MAX - high, P - 2, P)      # (0 when high is u32::MAX)
        _limbs(wires, r, 6 * ops + 32 * i, o, 32)


def _fill_u32addmany(wires, g):                      # add_many_u32.rs:329-378; wires :50-86
    r, na, ops = g["row"], g["na"], g["num_ops"]
    for i in range(ops):
        b = (na + 3) * i
        low, high = _halves(sum(int(wires[b + j, r]) for j in range(na + 1)) % P)
        wires[b + na + 1, r], wires[b + na + 2, r] = low, high
        _limbs(wires, r, (na + 3) * ops + 18 * i, low, 16)
        _limbs(wires, r, (na + 3) * ops + 18 * i + 16, high, 2)


def _fill_u32sub(wires, g):                          # subtraction_u32.rs:298-343; wires :45-79
    r, ops = g["row"], g["num_ops"]
    for i in range(ops):
        res, borrow = _sub_u32(*(int(wires[5 * i + j, r]) for j in range(3)))
        wires[5 * i + 3, r], wires[5 * i + 4, r] = res, borrow
        _limbs(wires, r, 5 * ops + 16 * i, res, 16)


def _fill_u32range(wires, g):                        # range_check_u32.rs:198-220; wires :40-51
    nl = len(g["limbs"])
    for i in range(nl):
        _limbs(wires, g["row"], nl + 16 * i, int(wires[i, g["row"]]) & U32_MAX, 16)


def _fill_cmp(wires, g):                             # comparison.rs:439-537; wires :52-96
    r, nb, nc = g["row"], g["bits"], g["chunks"]
    cb = -(-nb // nc)
    a, b = int(wires[0, r]), int(wires[1, r])
    wires[2, r] = 1 if a <= b else 0
    msd = 0
    for i in range(nc):
        f, s2 = (a >> (cb * i)) & ((1 << cb) - 1), (b >> (cb * i)) & ((1 << cb) - 1)
        wires[4 + i, r], wires[4 + nc + i, r] = f, s2
        wires[4 + 2 * nc + i, r] = 1 if f == s2 else pow((s2 - f) % P, P - 2, P)
        wires[4 + 3 * nc + i, r] = 1 if f == s2 else 0
        wires[4 + 4 * nc + i, r] = msd if f == s2 else 0
        if f != s2:
            msd = (s2 - f) % P
    wires[3, r] = msd
    v = ((1 << cb) + msd) % P
    for i in range(cb + 1):
        wires[4 + 5 * nc + i, r] = (v >> i) & 1


def _cmp_spec(b, bits, chunks):
    chunk_bits = -(-bits // chunks)
    return (1 << chunk_bits, "ComparisonGate { num_bits: %d, num_chunks: %d, %s }<D=2>" % (bits, chunks, _PHANTOM),
            (G_COMPARISON, (bits, chunks, 0, 0), 1 << chunk_bits, 0))


# id() = format!("{self:?}") (ComparisonGate: + "<D=2>"), degree 1 << limb_bits = 4 (range check: BASE = 4; comparison:
# 1 << chunk_bits), no constants.  An operation's routed wires follow each other (arithmetic_u32.rs:44-69 six per op, add_many_u32.rs
# :50-70 addends, carry, result, carry out, subtraction_u32.rs:45-65 five per op); range_check_u32.rs:40-43, comparison.rs:52-62
ROW_KINDS.update({
    "u32arith": RowKind(lambda g: (), lambda b: (4, "U32ArithmeticGate { num_ops: %d, %s }" % (b.u32_gate_ops("u32arith"), _PHANTOM),
                                                 (G_U32_ARITHMETIC, (b.u32_gate_ops("u32arith"), 0, 0, 0), 4, 0)),
                        lambda g: op_cells(g, 6), _fill_u32arith),
    "u32addmany": RowKind(lambda g: (g["na"],),
                          lambda b, na: (4, "U32AddManyGate { num_addends: %d, num_ops: %d, %s }" % (na, b.u32_gate_ops("u32addmany", na), _PHANTOM),
                                         (G_U32_ADD_MANY, (na, b.u32_gate_ops("u32addmany", na), 0, 0), 4, 0)),
                          lambda g: op_cells(g, g["na"] + 3), _fill_u32addmany),
    "u32sub": RowKind(lambda g: (), lambda b: (4, "U32SubtractionGate { num_ops: %d, %s }" % (b.u32_gate_ops("u32sub"), _PHANTOM),
                                               (G_U32_SUBTRACTION, (b.u32_gate_ops("u32sub"), 0, 0, 0), 4, 0)),
                      lambda g: op_cells(g, 5), _fill_u32sub),
    "u32range": RowKind(lambda g: (len(g["limbs"]),),
                        lambda b, nl: (4, "U32RangeCheckGate { num_input_limbs: %d, %s }" % (nl, _PHANTOM), (G_U32_RANGE_CHECK, (nl, 0, 0, 0), 4, 0)),
                        lambda g: list(zip(g["limbs"], range(len(g["limbs"])))), _fill_u32range),
    "cmp": RowKind(lambda g: (g["bits"], g["chunks"]), _cmp_spec, lambda g: [(g["a"], 0), (g["b"], 1), (g["res"], 2)], _fill_cmp),
})


# constraints per operation (gates.hpp: 2 + 32 limbs + 2, 1 + 18 + 2, 1 + 16 + 2; per range-checked limb 1 + 16)
ROW_OPS.update({"u32arith": (lambda g: 36, lambda g: g["ops"]), "u32addmany": (lambda g: 21, lambda g: g["ops"]),
                "u32sub": (lambda g: 19, lambda g: g["ops"]), "u32range": (lambda g: 17, lambda g: [[t] for t in g["limbs"]])})


class CircuitBuilderU32:
    """arithmetic_u32.rs `CircuitBuilderU32`, `range_check_u32` and `list_le` / `list_le_u32`."""

    def u32_gate_ops(self, kind, num_addends=0):
        """Operations per row: U32ArithmeticGate::num_ops (gates/arithmetic_u32.rs:39-42: 6 routed wires and 32 two-bit limbs
        per op), U32AddManyGate::num_ops (add_many_u32.rs:43-48: num_addends + 3 routed, 18 limbs), U32SubtractionGate::num_ops
        (subtraction_u32.rs:39-43: 5 routed, 16 limbs).  135 wires: 3 / 135 // (a + 21) / 6; 234 wires: 6 / min(234 // (a + 21),
        80 // (a + 3)) / 11."""
        routed, limbs = _OP_SHAPE[kind]
        return min(self.num_wires // (num_addends + routed + limbs), NUM_ROUTED // (num_addends + routed))

    def _u32_op(self, kind, ins, num_addends=0):
        """One operation of a shared row: `ins`, then two fresh targets, which are returned.  circuit_builder.rs
        `find_slot(gate, params, constants)` -- UNPINNED (recollection of plonky2 0.2.2, restated as `random_access` restates
        it): one open row per (gate, params) until it is full.  The operations of a shared row that nobody takes stay unconnected:
        their wires are what the gate's generator derives from zeros (build() and the device's fill_witness fill them so)."""
        key = (kind, num_addends)
        r = self.free_u32.get(key)
        if r is None or len(self.rows[r]["ops"]) == self.rows[r]["num_ops"]:
            r = len(self.rows)
            self.rows.append({"kind": kind, "na": num_addends, "num_ops": self.u32_gate_ops(kind, num_addends), "ops": []})
            self.free_u32[key] = r
        outs = (self.add_virtual_target(), self.add_virtual_target())
        self.rows[r]["ops"].append(tuple(ins) + outs)
        self.events.append(Generator(kind, ins, outs))
        return outs

    # arithmetic_u32.rs:79-81, :95-109: a U32Target is a Target
    add_virtual_u32_target, zero_u32, one_u32 = CircuitBuilder.add_virtual_target, CircuitBuilder.zero, CircuitBuilder.one
    connect_u32, assert_zero_u32 = CircuitBuilder.connect, CircuitBuilder.assert_zero

    def add_virtual_u32_targets(self, n):
        """arithmetic_u32.rs:83-88"""
        return [self.add_virtual_target() for _ in range(n)]

    def constant_u32(self, c):
        """arithmetic_u32.rs:91-93"""
        assert 0 <= c <= U32_MAX
        return self.constant(c)

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
        return special if special is not None else self._u32_op("u32arith", (x, y, z))

    def add_u32(self, a, b):
        """arithmetic_u32.rs:159-162"""
        return self.mul_add_u32(a, self.one_u32(), b)

    def _add_many_gate(self, to_add, carry):
        if len(to_add) > MAX_NUM_ADDENDS:
            raise ValueError("U32AddManyGate: %d addends, MAX_NUM_ADDENDS is %d" % (len(to_add), MAX_NUM_ADDENDS))
        return self._u32_op("u32addmany", tuple(to_add) + (carry,), len(to_add))

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
        return self._u32_op("u32sub", (x, y, borrow))

    def range_check_u32(self, vals):
        """gadgets/range_check_u32.rs:9-20: one U32RangeCheckGate row (add_gate: never shared) over all of `vals`."""
        vals = list(vals)
        if 17 * len(vals) > self.num_wires:
            raise ValueError("U32RangeCheckGate: %d limbs need %d wires" % (len(vals), 17 * len(vals)))
        self.rows.append({"kind": "u32range", "limbs": vals})
        self.events.append(Generator("u32range", tuple(vals), ()))

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
                self.events.append(Generator("cmp", (first, second), (out,)))
                res.append(out)
            a_le_b, b_le_a = res
            these_limbs_equal = self.mul(a_le_b, b_le_a)
            these_limbs_less_than = self.sub(one, b_le_a)
            result = self.mul_add(these_limbs_equal, result, these_limbs_less_than)
        return result

    def list_le_u32(self, a, b):
        """multiple_comparison.rs:69-78"""
        return self.list_le(a, b, 32)
