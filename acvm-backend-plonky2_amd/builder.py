"""The part of plonky2 0.2.2's ``CircuitBuilder`` the translators reach (see translate.py's docstring for what is pinned and
what is recollection): targets and copy constraints, constants, `arithmetic` and its helpers, booleans, `is_equal`,
`random_access`, split / join, and `build()` on top of the library's own `build_blob`.
Two tables state every kind once, GENERATORS and ROW_KINDS; the gadget modules add theirs next to the gadgets that emit them.  A
gadget records a `Generator` and appends row dicts; `_layout()`, `build()`, `_seed_classes()` and `generators()` know no kind.
"""
from collections import defaultdict, namedtuple
from itertools import chain

import numpy as np

from .prover import build_blob
from .synth import poseidon_gate_row

P = 0xFFFFFFFF00000001
NUM_WIRES, NUM_ROUTED, NUM_OPS, BASE_SUM_LIMBS, NUM_CONSTANTS = 234, 80, 20, 63, 2      # (CircuitConfig::num_constants of both configurations)
G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC, G_BASE_SUM, G_RANDOM_ACCESS, G_POSEIDON = 0, 1, 2, 3, 4, 5, 6


class Generator:
    """One witness generator (an "event"), in creation order in `CircuitBuilder.events`."""
    __slots__ = ("kind", "ins", "outs", "derives", "span", "groups", "field", "args", "row")      # (a SHA-256 block has 340 000)

    def __init__(self, kind, ins, outs, derives=None, span=1, groups=None, field=None, args=(), row=None):
        self.kind = kind                  # a key of GENERATORS
        self.ins = ins                    # the targets it reads (a tuple): it runs once all of them have values
        self.outs = outs                  # the targets it sets (a tuple), in the order its body returns their values
        # the outputs that make a copy class derived (no seed): all, but for a split, whose row sums sit in the integer's class
        self.derives = outs if derives is None else derives
        self.span = span                  # gate rows it writes in (the device's generators are gate-local: a split may span more)
        self.groups = groups              # a listed kind's targets as generators() names their cells, else None
        # a nonnative kind's field (a name of NONNATIVE_FIELDS), the body's constants, the gate row a body leaves something in
        self.field, self.args, self.row = field, args, row

    def __getitem__(self, i):
        """Read as the positional tuple this record replaced: [0] is the kind; of a kind the plan lists, (kind, *groups[, field])."""
        return ((self.kind,) + (self.groups or ()) + (() if self.field is None else (self.field,)))[i]


# body(ev, input values in ev.ins' order) -> output values in ev.outs' order, ValueError where the circuit is unsatisfiable.  A kind
# the witness plan lists has its plan name, the words of generators()'s error, and `given`: its operands are the program's own
# when nothing created earlier derives them.
GeneratorKind = namedtuple("GeneratorKind", "body plan missing given", defaults=(None, None, False))
# params(row) -> what tells two gates of the kind apart; spec(builder, *params) -> (degree, id string, gate declaration); cells(row)
# -> [(target, column)] in column order; fill(wires, row) writes wires[:, row["row"]]'s gate-internal columns from the routed ones.
RowKind = namedtuple("RowKind", "params spec cells fill", defaults=(None,))
Layout = namedtuple("Layout", "blob rows pi_row constants cells n")


def op_cells(g, stride):                          # a row of operations whose routed wires follow each other, `stride` per operation
    return [(t, stride * k + j) for k, op in enumerate(g["ops"]) for j, t in enumerate(op)]


def _arith_body(ev, vs):
    c0, c1 = ev.args                                  # (the product is read only when c0 != 0, the addend only when c1 != 0)
    return [((c0 * vs[0] % P * vs[1] if c0 else 0) + (c1 * vs[-1] if c1 else 0)) % P]


def _poseidon_body(ev, vs):                       # (the row keeps all 135 wire values for _fill_poseidon)
    ev.row["wires"] = poseidon_gate_row(vs)
    return [int(w) for w in ev.row["wires"][12:24]]


def _ra_body(ev, vs):
    if vs[0] >= len(vs) - 1:
        raise ValueError("unsatisfiable: a random access reads position %d of %d" % (vs[0], len(vs) - 1))
    return [vs[1 + vs[0]]]


def _split_body(ev, vs):
    base, rows, whole = ev.args                       # whole: the limbs must take all of the integer (split_le_base)
    v, out = vs[0], []
    for num_limbs in rows:                            # per row: the sum, then its limbs
        v, part = divmod(v, base ** num_limbs)
        limbs, rest = [], part
        for _ in range(num_limbs):
            rest, limb = divmod(rest, base)
            limbs.append(limb)
        out += [part] + limbs
    if whole and v:                                   # BaseSplitGenerator: "Integer too large to fit in given number of limbs"
        raise ValueError("unsatisfiable: split_le_base: the integer does not fit its limbs")
    return out


GENERATORS = {
    "arith": GeneratorKind(_arith_body),
    "poseidon": GeneratorKind(_poseidon_body),
    "equal": GeneratorKind(lambda ev, vs: [1 if vs[0] == vs[1] else 0, pow((vs[0] - vs[1]) % P, P - 2, P)],      # (inv: 0 when equal)
                           "equality", "is_equal: a target of the equality generator"),
    "ra": GeneratorKind(_ra_body),
    "split": GeneratorKind(_split_body),
    "lesum": GeneratorKind(lambda ev, vs: [sum(b << j for j, b in enumerate(vs)) % P]),
}


def _ra_spec(b, bits):
    # UNPINNED: the id as plonky2 0.2.2 prints it, format!("{self:?}<D={D}>"), as recollected
    copies, extra = b._ra_shape(bits)
    return (bits + 1, "RandomAccessGate { bits: %d, num_copies: %d, num_extra_constants: %d, _phantom: "
            "PhantomData<plonky2_field::goldilocks_field::GoldilocksField> }<D=2>" % (bits, copies, extra),
            (G_RANDOM_ACCESS, (bits, copies, extra, 0), bits + 1, extra))


def _ra_cells(g):
    stride = 2 + (1 << g["bits"])
    return [(t, stride * k + j) for k, (idx, claimed, lst) in enumerate(g["copies"]) for j, t in enumerate([idx, claimed] + lst)]


def _fill_ra(wires, g):                           # RandomAccessGenerator: the index bits, in the non-routed wires
    bits, stride, r = g["bits"], 2 + (1 << g["bits"]), g["row"]
    routed = stride * g["num_copies"] + g["extra"]
    for k in range(len(g["copies"])):
        for i in range(bits):
            wires[routed + k * bits + i, r] = (int(wires[stride * k, r]) >> i) & 1


def _fill_poseidon(wires, g):                     # the PoseidonGate's internal wires (deltas, S-box inputs): its generator's
    wires[:135, g["row"]] = g["wires"]


ROW_KINDS = {
    "arith": RowKind(lambda g: (), lambda b: (3, "ArithmeticGate { num_ops: 20 }", (G_ARITHMETIC, (NUM_OPS, 0, 0, 0), 3, 2)),
                     lambda g: op_cells(g, 4)),
    "poseidon": RowKind(lambda g: (), lambda b: (7, "PoseidonGate(PhantomData<plonky2_field::goldilocks_field::GoldilocksField>)<WIDTH=12>",
                                                 (G_POSEIDON, (0, 0, 0, 0), 7, 0)),
                        lambda g: list(zip(g["in"] + g["out"] + [g["swap"]], range(25))), _fill_poseidon),
    "ra": RowKind(lambda g: (g["bits"],), _ra_spec, _ra_cells, _fill_ra),
    # UNPINNED: the id as plonky2 0.2.2 prints it, format!("{self:?} + Base: {B}"), as recollected; degree() = B
    "basesum": RowKind(lambda g: (g["base"], g["L"]),
                       lambda b, base, L: (base, "BaseSumGate { num_limbs: %d } + Base: %d" % (L, base), (G_BASE_SUM, (base, L, 0, 0), base, 0)),
                       lambda g: list(zip([g["sum"]] + g["limbs"], range(1 + g["L"])))),
}
# The rows that hold several operations, for explain(): (constraints per operation -- an operation's constraints follow each other
# in the gate's evaluation order, csrc/gates.hpp --, row -> the targets of every operation)
ROW_OPS = {"arith": (lambda g: 1, lambda g: g["ops"]),
           "ra": (lambda g: g["bits"] + 2, lambda g: [[idx, claimed] + lst for idx, claimed, lst in g["copies"]])}
SPECIAL_ROWS = {("noop",): (0, "NoopGate", (G_NOOP, (0, 0, 0, 0), 0, 0)),
                ("const",): (1, "ConstantGate { num_consts: 2 }", (G_CONSTANT, (2, 0, 0, 0), 1, 2)),
                ("pi",): (1, "PublicInputGate", (G_PUBLIC_INPUT, (0, 0, 0, 0), 1, 0))}


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
        self.rows = []            # gate instances in creation order: dicts, "kind" a key of ROW_KINDS
        self.free_arith = {}      # (c0, c1) -> row with a free slot
        self.arith_results = {}   # (c0, c1, m0, m1, addend) -> output target of the identical earlier operation
        self.events = []          # witness generators (Generator) in creation order
        self.free_ra = {}         # bits -> RandomAccess row with a free copy
        self.free_u32 = {}        # (gate, params) -> U32 row with a free operation
        self.rng = np.random.default_rng(seed)
        self._lay = None          # what _layout() made

    # -- targets, copy constraints --------------------------------------------------------------
    def add_virtual_target(self):
        t = len(self.parent)
        self.parent.append(t)
        return t

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

    def assert_one(self, x):
        """circuit_builder.rs assert_one (biguint.rs:259 calls it)"""
        self.connect(x, self.one())

    def target_as_constant(self, t):
        """circuit_builder.rs target_as_constant: the constant of a target `constant()` returned, else None."""
        return self.const_of.get(t)

    def register_public_input(self, t):
        self.public_inputs.append(t)

    # -- gadgets/arithmetic.rs --------------------------------------------------------------------
    def arithmetic(self, c0, c1, m0, m1, addend):
        c0 %= P
        c1 %= P
        zero = self.consts[0] if 0 in self.consts else self.zero()
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
        # (the product is read only when c0 != 0, the addend only when c1 != 0; both zero is a constant, above)
        self.events.append(Generator("arith", (m0, m1, addend) if c0 and c1 else (m0, m1) if c0 else (addend,), (out,), args=self.rows[r]["c"]))
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

    def add_many(self, terms):
        """gadgets/arithmetic.rs `add_many` -- UNPINNED (recollection of plonky2 0.2.2): a fold with `add` from `zero()`."""
        acc = self.zero()
        for t in terms:
            acc = self.add(acc, t)
        return acc

    # -- booleans (gadgets/arithmetic.rs, gadgets/select.rs) ---------------------------------------
    def assert_bool(self, b):
        self.connect(self.mul_sub(b, b, b), self.zero())

    def add_virtual_bool_target_safe(self):
        b = self.add_virtual_target()
        self.assert_bool(b)
        return b

    add_virtual_bool_target_unsafe = add_virtual_target      # (circuit_builder.rs: nothing constrains it to a bit)
    and_ = mul

    def or_(self, a, b):
        return self.add(self.arithmetic(P - 1, 1, a, b, a), b)

    def not_(self, b):
        return self.sub(self.one(), b)

    def select(self, b, x, y):
        return self.mul_sub(b, x, self.mul_sub(b, y, y))

    _if = select

    def is_equal(self, x, y):
        """gadgets/arithmetic.rs `is_equal` -- UNPINNED: the order of its steps is a recollection of plonky2 0.2.2.  The
        EqualityGenerator it registers belongs to no gate row: its four targets lie in ArithmeticGate rows (event "equal")."""
        zero = self.zero()
        equal = self.add_virtual_target()              # add_virtual_bool_target_unsafe
        not_equal = self.not_(equal)
        inv = self.add_virtual_target()
        self.events.append(Generator("equal", (x, y), (equal, inv), groups=(x, y, equal, inv)))
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

    def _ra_copy(self, row, index, v):
        claimed = self.add_virtual_target()
        row["copies"].append((index, claimed, v))
        self.events.append(Generator("ra", (index, *v), (claimed,)))
        return claimed

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
        return self._ra_copy(self.rows[r], index, v)

    # -- gadgets/split_join.rs ----------------------------------------------------------------------
    def _base_sum_row(self, num_limbs, base=2):
        row = {"kind": "basesum", "base": base, "L": num_limbs, "sum": self.add_virtual_target(),
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
        acc = self.zero()
        for g in reversed(gates):
            acc = self.mul_const_add(pow(2, BASE_SUM_LIMBS, P), acc, g["sum"])
        self.connect(acc, integer)
        self.events.append(Generator("split", (integer,), tuple(t for g in gates for t in [g["sum"]] + g["limbs"]), tuple(bits),
                                     span=k, args=(2, (BASE_SUM_LIMBS,) * k, False)))
        return bits[:num_bits]

    def split_le_base(self, x, num_limbs, base=4):
        """gadgets/split_base.rs `split_le_base::<B>` -- UNPINNED (recollection of plonky2 0.2.2): one BaseSumGate<B> row of
        `num_limbs` limbs, `x` connected to its sum wire, the limb wires returned; nothing else is constrained.  The generator is
        the row's own BaseSplitGenerator, which panics when x does not fit."""
        row = self._base_sum_row(num_limbs, base)
        self.connect(x, row["sum"])
        self.events.append(Generator("split", (x,), tuple([row["sum"]] + row["limbs"]), tuple(row["limbs"]), args=(base, (num_limbs,), True)))
        return list(row["limbs"])

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
        self.events.append(Generator("lesum", tuple(row["limbs"]), (row["sum"],)))
        return row["sum"]

    # -- build(): rows -> blob (library) + witness ----------------------------------------------------
    def _layout(self):
        """The circuit half of build(): rows -> blob, and the cells of every copy class, as a Layout.  Runs once; build(),
        seed_cells() and seed_values() share its result."""
        if self._lay is not None:
            return self._lay
        zero = self.zero()
        # fill_batched_gates: the unused copies of a RandomAccess row read position `zero` of a list of `zero`s into a fresh
        # claimed element
        for g in self.rows:
            if g["kind"] == "ra":
                while len(g["copies"]) < g["num_copies"]:
                    self._ra_copy(g, zero, [zero] * (1 << g["bits"]))
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
            self.events.append(Generator("poseidon", tuple(state), tuple(row["out"]), row=row))
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
        keys = [(g["kind"],) + ROW_KINDS[g["kind"]].params(g) for g in rows]
        spec = {k: ROW_KINDS[k[0]].spec(self, *k[1:]) for k in set(keys)}
        spec.update({k: SPECIAL_ROWS[k] for k in [("pi",)] + ([("const",)] if const_rows else []) + ([("noop",)] if used < n else [])})
        order = sorted(spec, key=lambda k: spec[k][:2])
        index = {k: i for i, k in enumerate(order)}
        gates = [spec[k][2] for k in order]
        row_gate = np.zeros(n, dtype=np.uint32)
        row_consts = np.zeros((2, n), dtype=np.uint64)
        cells, find = defaultdict(list), self.find  # class root -> [(row, col)]

        def put(t, r, c):
            cells[find(t)].append((r, c))

        for r, (g, k) in enumerate(zip(rows, keys)):
            row_gate[r] = index[k]
            g["row"] = r
            for i, c in enumerate(g.get("c", ())):  # (an ArithmeticGate row's c0, c1)
                row_consts[i, r] = c
            for t, c in ROW_KINDS[g["kind"]].cells(g):
                cells[find(t)].append((r, c))
        row_gate[pi_row] = index[("pi",)]
        for i in range(4):                          # (no public inputs: four copies of `zero`)
            put(pi_hash[i], pi_row, i)
        for (c, t), (r, i) in zip(extra_consts, extra_wires):
            row_consts[i, r] = c
            put(t, r, (2 + (1 << rows[r]["bits"])) * rows[r]["num_copies"] + i)
        for i, (c, t) in enumerate(const_list):
            r = pi_row + 1 + i // 2
            row_consts[i % 2, r] = c
            put(t, r, i % 2)
        if const_rows:
            row_gate[pi_row + 1:pi_row + 1 + const_rows] = index[("const",)]
        if used < n:
            row_gate[used:] = index[("noop",)]
        flat = np.fromiter(chain.from_iterable(chain.from_iterable(cells.values())), dtype=np.uint32).reshape(-1, 2)
        last = np.cumsum([len(cl) for cl in cells.values()]) - 1      # (copy pairs: a class's last cell starts none)
        blob = build_blob(d, gates, row_gate, row_consts, np.delete(np.hstack([flat[:-1], flat[1:]]), last[:-1], axis=0),
                          num_public_inputs=len(self.public_inputs), num_wires=self.num_wires)
        self.pi_row = pi_row
        self._lay = Layout(blob, rows, pi_row, extra_consts + const_list, dict(cells), n)
        return self._lay

    def blob(self):
        """The circuit blob alone (build() without the witness)."""
        return self._layout().blob

    def cells_of(self, target):
        """[(row, col)] of the target's copy class, in row order (KeyError: the class lies in no gate row)."""
        return self._layout().cells[self.find(target)]

    def build(self, witness_values):
        """witness_values: {target: value}.  Returns (blob, wires) for CircuitData(blob).prove(wires)."""
        lay = self._layout()
        # witness: the generators, in creation order, until nothing changes
        val = {self.find(t): c for c, t in lay.constants}
        for t, v in witness_values.items():
            rt = self.find(t)
            v %= P
            if rt in val and val[rt] != v:
                raise ValueError("witness value contradicts the circuit")
            val[rt] = v
        pending, find, bodies = list(self.events), self.find, {name: kind.body for name, kind in GENERATORS.items()}
        while pending:
            rest = []
            for ev in pending:
                vs = list(map(val.get, map(find, ev.ins)))
                if None in vs:
                    rest.append(ev)
                    continue
                for t, v in zip(ev.outs, bodies[ev.kind](ev, vs)):
                    if val.setdefault(find(t), v) != v:
                        raise ValueError("unsatisfiable: a generator contradicts an assigned value")
            if len(rest) == len(pending):
                raise ValueError("witness generation is stuck: some inputs were not assigned")
            pending = rest
        W = self.num_wires
        wires = np.zeros((W, lay.n), dtype=np.uint64)
        for rt, cl in lay.cells.items():
            v = val.get(rt)
            if v is None:
                # the dummy addend of a product-only op whose operand is otherwise unconstrained
                raise ValueError("a wire has no value")
            for (r, c) in cl:
                wires[c, r] = v
        for g in lay.rows:                          # the gate-internal wires: every operation's generator, the unused ones' too
            fill = ROW_KINDS[g["kind"]].fill
            if fill is not None:
                fill(wires, g)
        wires[4:, lay.pi_row] = self._random_pi_wires()
        self.public_input_values = [val[self.find(t)] for t in self.public_inputs]
        self.values = val
        return lay.blob, wires

    # -- the witness on the GPU: what the caller still has to supply ------------------------------------
    def _seed_classes(self):
        """(cells, roots) of the seeds that carry a value of the program: one cell per copy class that holds no constant and
        no generator's output -- the targets `pw.set_target` is called on -- in the order of the classes' first targets."""
        cells = self._layout().cells
        derived = {self.find(t) for t in self.const_of}
        # the operands of a div-rem generator are the program's when nothing created before it derives them: `div_rem_biguint`
        # connects a to div * b + rem afterwards, which compares (biguint.rs:254-256) and does not make `a` an output; the
        # nonnative gadgets connect their operands the same way.  (A seed names the first cell of its class: an operand that
        # enters the circuit nowhere before div_rem_biguint has that result column as its only cell, and the row op then shares
        # the cell's writer bit with the seed -- DESIGN.md 11.6.)
        given = set()
        for ev in self.events:
            if GENERATORS[ev.kind].given:
                given.update(self.find(t) for t in ev.ins if self.find(t) not in derived)
            assert ev.span == 1, "a split over several BaseSum rows spans rows: not a gate-local generator"
            derived.update(self.find(t) for t in ev.derives)
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
        return [given[rt] for rt in roots] + [int(x) for x in self._random_pi_wires()]

    def _random_pi_wires(self):
        """circuit_builder.rs randomize_unused_pi_wires: every wire of the PublicInputGate row after the hash, routed (one draw)
        or not (a second), gets a random value (so no wire column of a real witness is zero in every row)"""
        return np.concatenate([self.rng.integers(0, P, size=NUM_ROUTED - 4, dtype=np.uint64),
                               self.rng.integers(0, P, size=self.num_wires - NUM_ROUTED, dtype=np.uint64)])

    def generators(self):
        """The generators that are no gate's own, for CircuitData.witness_plan(..., generators=): ("equality", (cell_x, cell_y,
        cell_equal, cell_inv)), ("biguint_divrem", (a_cells, b_cells, div_cells, rem_cells)) and, for the four nonnative
        generators, ("nonnative_add" | "_sub" | "_mul" | "_inv", (a_cells, b_cells, first target's cells, second target's cells),
        field name), and ("glv_decompose", (k_cells, (), k1's then k2's cells, (k1_neg cell, k2_neg cell))), in creation order; a
        target's cell -- a limb's too -- is the first cell of its copy class."""
        cells = self._layout().cells

        def first_cells(group, missing):
            if isinstance(group, tuple):
                return tuple(first_cells(t, missing) for t in group)
            if self.find(group) not in cells:
                raise ValueError("%s lies in no gate row" % missing)
            return cells[self.find(group)][0]

        out = []
        for ev in self.events:
            kind = GENERATORS[ev.kind]
            if kind.plan is not None:
                out.append((kind.plan, first_cells(ev.groups, kind.missing)) + ((ev.field,) if ev.field is not None else ()))
        return out

    # -- a WitnessReport (CircuitData.check_witness) in the builder's own words ----------------------------
    def row_of(self, row):
        """(what the circuit's row `row` is to the builder, its creating row dict or None): a row of self.rows by its kind, the
        PublicInputGate row, a ConstantGate row, padding."""
        lay = self._layout()
        if row < len(lay.rows):
            return lay.rows[row]["kind"], lay.rows[row]
        if row == lay.pi_row:
            return "pi", None
        in_extra_wires = min(len(lay.constants), sum(g["extra"] for g in lay.rows if g["kind"] == "ra"))
        const_rows = (len(lay.constants) - in_extra_wires + 1) // 2
        return ("const" if row <= lay.pi_row + const_rows else "noop"), None

    def _class_name(self, cell):
        """A routed cell by its copy class: the class's first target, its size and its first cell (cells_of)."""
        for rt, cl in self._layout().cells.items():
            if cell in cl:
                const = next((c for t, c in self.const_of.items() if self.find(t) == rt), None)
                return "target %d%s (class of %d cells from %s)" % (rt, "" if const is None else " = constant %d" % const, len(cl), cl[0])
        return "no target"

    def explain(self, report):
        """A short string: the report's first failing row as the builder made it -- the creating row's kind, the operation inside
        it where the row holds several, the targets routed there -- and its first broken copy as the copy classes (cells_of) of
        the two cells."""
        parts = []
        if report.first_gate is not None:
            row, _, _, constraint, value = report.first_gate
            kind, g = self.row_of(row)
            text = "row %d is a %s row: constraint %d = 0x%x" % (row, kind, constraint, value)
            if g is not None and kind in ROW_OPS:
                per_op, ops_of = ROW_OPS[kind]
                k, ops = constraint // per_op(g), ops_of(g)
                text += ", operation %d" % k + (" on targets %s" % (tuple(ops[k]),) if k < len(ops) else " (unused)")
            elif g is not None:
                text += ", targets %s" % (tuple(t for t, _ in ROW_KINDS[kind].cells(g)),)
            parts.append(text)
        if report.first_copy is not None:
            (r0, c0), (r1, c1), (v0, v1) = report.first_copy
            parts.append("copy: cell (%d, %d) = 0x%x of %s differs from cell (%d, %d) = 0x%x of %s"
                         % (r0, c0, v0, self._class_name((r0, c0)), r1, c1, v1, self._class_name((r1, c1))))
        if report.first_noncanonical is not None:
            parts.append("cell (%d, %d) holds no canonical field element" % report.first_noncanonical)
        return "; ".join(parts) if parts else "the witness satisfies the circuit"

    def value_of(self, t):
        return self.values[self.find(t)]
