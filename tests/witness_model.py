"""An independent model of the device witness path (test infrastructure): pure Python over big ints, nothing of the
package in it.  Five parts:
  the op registry     which ops a gate row holds and which columns each reads and sets (`row_ops`; the listed generators' shapes);
  the bodies          one function per op code, "to_canonical_u64, then integer arithmetic", restated from the upstream generators
                      (plonky2_ecdsa/biguint/gates/{arithmetic_u32,add_many_u32,subtraction_u32,range_check_u32,comparison}.rs,
                      biguint/biguint.rs, and the stock plonky2 ones); where upstream would panic they name the rejected column;
  evaluate            a plan-free fixed point over the whole matrix: the oracle for the matrix, it knows nothing about levels;
  predict, check_plan what makes a circuit refused and a plan valid, stated as properties of the exported arrays;
  interpret           an exported plan run op by op with the walk's accessor rules: the oracle for the cell a failing witness names.
A circuit is a `Circuit` below: the form it was generated in (gates, row -> gate, constants, copy pairs, generator list); sigma is
never read."""
import json
import os

P = 0xFFFFFFFF00000001
UNSET, WRITER = 0xFFFFFFFF, 0x80000000
G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC, G_BASE_SUM, G_RANDOM_ACCESS, G_POSEIDON = 0, 1, 2, 3, 4, 5, 6
G_U32_ARITHMETIC, G_U32_ADD_MANY, G_U32_SUBTRACTION, G_U32_RANGE_CHECK, G_COMPARISON = 7, 8, 9, 10, 11
(OP_SEED, OP_CONSTANT, OP_ARITHMETIC, OP_BASE_SPLIT, OP_BASE_JOIN, OP_RA_COPY, OP_RA_CONSTS, OP_POSEIDON, OP_U32_ARITHMETIC, OP_U32_ADD_MANY,
 OP_U32_SUBTRACTION, OP_U32_RANGE_CHECK, OP_COMPARISON, OP_EQUALITY, OP_BIGUINT_DIVREM) = range(15)
GEN_CODE = {"equality": OP_EQUALITY, "biguint_divrem": OP_BIGUINT_DIVREM}
GEN_KIND = {"equality": 0, "biguint_divrem": 1}

with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "poseidon.json")) as _f:
    POSEIDON_RC = [int(x) for x in json.load(_f)["round_constants"]]
# plonky2 poseidon_goldilocks.rs MDS_MATRIX_CIRC / MDS_MATRIX_DIAG (width 12)
MDS_CIRC = [17, 15, 41, 16, 2, 28, 13, 13, 39, 18, 34, 20]
MDS_DIAG = [8, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]


def inv(a):
    return pow(a, P - 2, P)


class Circuit:
    """gates: [(kind, params, degree, num_constants)]; row_gate [n]; consts [k][n] (gate constants per row); copies [(row, col, row,
    col)] over routed cells; gens: [(kind name, (a cells, b cells, div cells, rem cells))] -- an equality generator has one cell each."""

    def __init__(self, d, W, R, gates, row_gate, consts, copies, gens=()):
        self.d, self.n, self.W, self.R = d, 1 << d, W, R
        self.gates = [(k, tuple(p), deg, nk) for k, p, deg, nk in gates]
        self.row_gate = list(row_gate) + [0] * (self.n - len(row_gate))
        self.consts = [list(c) for c in consts]
        self.copies = [tuple(int(x) for x in c) for c in copies]
        self.gens = [(k, tuple(tuple((int(r), int(c)) for r, c in grp) for grp in groups)) for k, groups in gens]

    @classmethod
    def from_kw(cls, kw, gens=()):
        """from the keywords of pkg.build_blob"""
        rc = [[int(x) for x in col] for col in kw["row_constants"]]
        return cls(kw["degree_bits"], kw.get("num_wires", 234), kw.get("num_routed_wires", 80), kw["gates"], [int(g) for g in kw["row_gate"]], rc,
                   [tuple(int(x) for x in cp) for cp in kw["copies"]], gens)

    def lc(self, row, i):
        return self.consts[i][row] if i < len(self.consts) else 0

    def gate(self, row):
        return self.gates[self.row_gate[row]]

    def key(self, cell):
        return (cell[1] << self.d) | cell[0]

    def cell(self, key):
        return key & (self.n - 1), key >> self.d

    def kw(self):
        """the keywords of pkg.build_blob / CircuitData.build"""
        import numpy as np
        rc = np.array(self.consts, dtype=np.uint64).reshape(len(self.consts), self.n) if self.consts else np.zeros((0, self.n), dtype=np.uint64)
        return dict(degree_bits=self.d, gates=[(k, p, deg, nk) for k, p, deg, nk in self.gates], row_gate=np.array(self.row_gate, dtype=np.uint32),
                    row_constants=rc, copies=np.array(self.copies, dtype=np.uint32).reshape(-1, 4), num_wires=self.W, num_routed_wires=self.R)

    def generator_list(self):
        """the `generators=` argument of witness_plan (None without any)"""
        return [(k, [list(g) for g in groups]) for k, groups in self.gens] if self.gens else None

    def gen_cells(self, g):
        return [c for grp in self.gens[g][1] for c in grp]

    def gen_shape(self, g):
        return tuple(len(grp) for grp in self.gens[g][1])


# ---- the op registry ----------------------------------------------------------------------------------------------------------
def row_ops(kind, p, c0=1, c1=1):
    """The ops of a row of gate (kind, p) in creation order: [(code, sub, input columns, output columns)].  c0, c1: the row's gate
    constants 0 and 1 -- an ArithmeticGate operation reads its multiplicands only when c0 != 0 and its addend only when c1 != 0."""
    r = lambda a, b: list(range(a, b))  # noqa: E731
    if kind == G_CONSTANT:
        return [(OP_CONSTANT, 0, [], r(0, p[0]))]
    if kind == G_ARITHMETIC:
        return [(OP_ARITHMETIC, i, (r(4 * i, 4 * i + 2) if c0 else []) + ([4 * i + 2] if c1 else []), [4 * i + 3]) for i in range(p[0])]
    if kind == G_BASE_SUM:
        return [(OP_BASE_SPLIT, 0, [0], r(1, 1 + p[1])), (OP_BASE_JOIN, 0, r(1, 1 + p[1]), [0])]
    if kind == G_RANDOM_ACCESS:
        bits, copies, extra = p[0], p[1], p[2]
        vec = 1 << bits
        routed = (2 + vec) * copies + extra
        out = [(OP_RA_COPY, k, [(2 + vec) * k] + r((2 + vec) * k + 2, (2 + vec) * (k + 1)), [(2 + vec) * k + 1] + r(routed + k * bits, routed + (k + 1) * bits))
               for k in range(copies)]
        return out + ([(OP_RA_CONSTS, 0, [], r((2 + vec) * copies, (2 + vec) * copies + extra))] if extra else [])
    if kind == G_POSEIDON:
        return [(OP_POSEIDON, 0, r(0, 12) + [24], r(12, 24) + r(25, 135))]
    if kind == G_U32_ARITHMETIC:
        return [(OP_U32_ARITHMETIC, i, r(6 * i, 6 * i + 3), r(6 * i + 3, 6 * i + 6) + r(6 * p[0] + 32 * i, 6 * p[0] + 32 * i + 32)) for i in range(p[0])]
    if kind == G_U32_ADD_MANY:
        na, nops = p[0], p[1]
        return [(OP_U32_ADD_MANY, i, r((na + 3) * i, (na + 3) * i + na + 1),
                 r((na + 3) * i + na + 1, (na + 3) * i + na + 3) + r((na + 3) * nops + 18 * i, (na + 3) * nops + 18 * i + 18)) for i in range(nops)]
    if kind == G_U32_SUBTRACTION:
        return [(OP_U32_SUBTRACTION, i, r(5 * i, 5 * i + 3), r(5 * i + 3, 5 * i + 5) + r(5 * p[0] + 16 * i, 5 * p[0] + 16 * i + 16)) for i in range(p[0])]
    if kind == G_U32_RANGE_CHECK:
        return [(OP_U32_RANGE_CHECK, 0, r(0, p[0]), r(p[0], 17 * p[0]))]
    if kind == G_COMPARISON:
        nc, cb = p[1], -(-p[0] // p[1])
        return [(OP_COMPARISON, 0, [0, 1], r(2, 4 + 5 * nc + cb + 1))]
    return []


def gen_op(shape):
    """a listed generator over its cell positions: reads a's and b's, sets div's and rem's ({1, 1, 1, 1}: x, y -> equal, inv)"""
    la, lb, ld, lr = shape
    return list(range(la + lb)), list(range(la + lb, la + lb + ld + lr))


def gate_wires_used(kind, p):
    cols = [c for _, _, i, o in row_ops(kind, p) for c in i + o]
    return max(cols) + 1 if cols else 0


# ---- the bodies: f(p, sub, get, lc) -> ([(column, value)], [rejected columns]) ---------------------------------------------------
def body_constant(p, sub, get, lc):
    return [(i, lc(i)) for i in range(p[0])], []


def body_arithmetic(p, i, get, lc):
    return [(4 * i + 3, (get(4 * i) * get(4 * i + 1) * lc(0) + get(4 * i + 2) * lc(1)) % P)], []


def body_base_split(p, sub, get, lc):
    """BaseSplitGenerator; upstream asserts that the sum fits the limbs"""
    v, out = get(0), []
    for i in range(p[1]):
        out.append((1 + i, v % p[0]))
        v //= p[0]
    return out, ([0] if v else [])


def body_base_join(p, sub, get, lc):
    """BaseSumGenerator of le_sum (gadgets/split_join.rs): field arithmetic from the top limb down"""
    s, rej = 0, []
    for i in reversed(range(p[1])):
        limb = get(1 + i)
        if limb >= p[0]:
            rej.append(1 + i)
        s = (s * p[0] + limb) % P
    return [(0, s)], rej


def body_ra_copy(p, k, get, lc):
    """RandomAccessGenerator: the index is taken modulo the vector size (upstream debug-asserts that it is smaller)"""
    bits, copies, extra = p[0], p[1], p[2]
    vec = 1 << bits
    base, routed = (2 + vec) * k, (2 + vec) * copies + extra
    idx = get(base)
    return [(base + 1, get(base + 2 + idx % vec))] + [(routed + k * bits + j, (idx >> j) & 1) for j in range(bits)], []


def body_ra_consts(p, sub, get, lc):
    vec = 1 << p[0]
    return [((2 + vec) * p[1] + i, lc(i)) for i in range(p[2])], []


def _mds(st):
    return [(sum(st[(i + r) % 12] * MDS_CIRC[i] for i in range(12)) + st[r] * MDS_DIAG[r]) % P for r in range(12)]


def poseidon_permute(st):
    return [v for c, v in body_poseidon((), 0, lambda c: (list(st) + [0] * 13)[c], None)[0] if 12 <= c < 24]


def body_poseidon(p, sub, get, lc):
    """PoseidonGenerator: swap, then 4 full, 22 partial, 4 full rounds; the S-box inputs of every round but the first are wires"""
    out, swap, st = [], get(24), [0] * 12
    for i in range(4):
        lo, hi = get(i), get(i + 4)
        delta = swap * (hi - lo) % P
        out.append((25 + i, delta))
        st[i], st[i + 4] = (lo + delta) % P, (hi - delta) % P
    for i in range(8, 12):
        st[i] = get(i)
    for r in range(30):
        st = [(v + POSEIDON_RC[12 * r + i]) % P for i, v in enumerate(st)]
        if r < 4 or r >= 26:
            if r:
                base = 29 + 12 * (r - 1) if r < 4 else 87 + 12 * (r - 26)
                out += [(base + i, st[i]) for i in range(12)]
            st = [pow(v, 7, P) for v in st]
        else:
            out.append((65 + r - 4, st[0]))
            st[0] = pow(st[0], 7, P)
        st = _mds(st)
    return out + [(12 + i, st[i]) for i in range(12)], []


def body_u32_arithmetic(p, i, get, lc):
    o = (get(6 * i) * get(6 * i + 1) + get(6 * i + 2)) % P
    hi, lo = o >> 32, o & 0xFFFFFFFF
    diff = 0xFFFFFFFF - hi
    return [(6 * i + 3, lo), (6 * i + 4, hi), (6 * i + 5, inv(diff) if diff else 0)] + [(6 * p[0] + 32 * i + j, (o >> (2 * j)) & 3) for j in range(32)], []


def body_u32_add_many(p, i, get, lc):
    na, nops = p[0], p[1]
    b = (na + 3) * i
    s = sum(get(b + j) for j in range(na + 1)) % P
    res, carry = s & 0xFFFFFFFF, s >> 32
    aux = (na + 3) * nops + 18 * i
    return ([(b + na + 1, res), (b + na + 2, carry)] + [(aux + j, (res >> (2 * j)) & 3) for j in range(16)]
            + [(aux + 16 + j, (carry >> (2 * j)) & 3) for j in range(2)]), []


def body_u32_subtraction(p, i, get, lc):
    init = (get(5 * i) - get(5 * i + 1) - get(5 * i + 2)) % P
    borrow = 1 if init > 1 << 32 else 0            # (subtraction_u32.rs:312: strictly greater)
    res = (init + (borrow << 32)) % P
    return [(5 * i + 3, res), (5 * i + 4, borrow)] + [(5 * p[0] + 16 * i + j, (res >> (2 * j)) & 3) for j in range(16)], []


def body_u32_range_check(p, sub, get, lc):
    out = []
    for i in range(p[0]):
        v = get(i) & 0xFFFFFFFF                     # (range_check_u32.rs:203: `as u32`)
        out += [(p[0] + 16 * i + j, (v >> (2 * j)) & 3) for j in range(16)]
    return out, []


def body_comparison(p, sub, get, lc):
    nc, cb = p[1], -(-p[0] // p[1])
    a, b, cs = get(0), get(1), 1 << cb
    fc = [(a // cs ** i) % cs for i in range(nc)]
    sc = [(b // cs ** i) % cs for i in range(nc)]
    out, msd = [(2, 1 if a <= b else 0)], 0
    for i, (f, s) in enumerate(zip(fc, sc)):
        out += [(4 + i, f), (4 + nc + i, s), (4 + 2 * nc + i, 1 if f == s else inv((s - f) % P)), (4 + 3 * nc + i, 1 if f == s else 0)]
        if f != s:
            msd = (s - f) % P
            out.append((4 + 4 * nc + i, 0))
        else:
            out.append((4 + 4 * nc + i, msd))
    t = (cs + msd) % P
    return out + [(3, msd)] + [(4 + 5 * nc + i, (t >> i) & 1) for i in range(cb + 1)], []


def body_equality(shape, sub, get, lc):
    diff = (get(0) - get(1)) % P
    return [(2, 1 if diff == 0 else 0), (3, inv(diff) if diff else 0)], []


def body_biguint_divrem(shape, sub, get, lc):
    """get_biguint_target folds the canonical limb values (a limb >= 2^32 carries), BigUint::div_rem, set_biguint_target asserts that
    the digits fit.  Rejected (generators.hpp): b = 0 on b's first cell and nothing is set; too many quotient digits on div's top
    limb (a's first cell where div has none), too many remainder digits on rem's top limb."""
    la, lb, ld, lr = shape
    a = sum(get(i) << (32 * i) for i in range(la))
    b = sum(get(la + i) << (32 * i) for i in range(lb))
    if b == 0:
        return [], [la]
    q, r = divmod(a, b)
    out = [(la + lb + i, (q >> (32 * i)) & 0xFFFFFFFF) for i in range(ld)] + [(la + lb + ld + i, (r >> (32 * i)) & 0xFFFFFFFF) for i in range(lr)]
    rej = ([la + lb + ld - 1 if ld else 0] if q >> (32 * ld) else []) + ([la + lb + ld + lr - 1] if r >> (32 * lr) else [])
    return out, rej


BODY = {OP_CONSTANT: body_constant, OP_ARITHMETIC: body_arithmetic, OP_BASE_SPLIT: body_base_split, OP_BASE_JOIN: body_base_join,
        OP_RA_COPY: body_ra_copy, OP_RA_CONSTS: body_ra_consts, OP_POSEIDON: body_poseidon, OP_U32_ARITHMETIC: body_u32_arithmetic,
        OP_U32_ADD_MANY: body_u32_add_many, OP_U32_SUBTRACTION: body_u32_subtraction, OP_U32_RANGE_CHECK: body_u32_range_check,
        OP_COMPARISON: body_comparison, OP_EQUALITY: body_equality, OP_BIGUINT_DIVREM: body_biguint_divrem}


def run_body(code, p, sub, get, lc):
    """BODY[code] looked up at call time (a test replaces one body by a wrong one)"""
    return BODY[code](p, sub, get, lc)


# ---- the circuit's structure: classes, ops, which cells carry a slot ----------------------------------------------------------------
class _Ops:
    """Every op of the circuit in creation order -- seeds, listed generators, rows -- over routed cells: (code, index, sub, input cells,
    output cells, p).  Columns >= R are gate-internal and left out; a row op none of whose cells has a slot is left out (`active`)."""

    def __init__(self, c, seeds):
        self.c, self.seeds = c, [tuple(s) for s in seeds]
        parent = {}

        def find(v):
            while parent.setdefault(v, v) != v:
                parent[v] = parent[parent[v]]
                v = parent[v]
            return v
        for ra, ca, rb, cb in c.copies:
            if (ra, ca) != (rb, cb):
                a, b = find(c.key((ra, ca))), find(c.key((rb, cb)))
                parent[max(a, b)] = min(a, b)
        self.find = find
        self.in_class = set(parent)
        # cells with a slot before the rows: classes, routed seeds, what the generators name
        slotted = set(parent) | {c.key(s) for s in self.seeds if s[1] < c.R} | {c.key(cell) for g in range(len(c.gens)) for cell in c.gen_cells(g)}
        self.ops = [(OP_SEED, i, 0, [], [s] if s[1] < c.R else [], None) for i, s in enumerate(self.seeds)]
        for g, (kind, _) in enumerate(c.gens):
            cells, (ins, outs) = c.gen_cells(g), gen_op(c.gen_shape(g))
            self.ops.append((GEN_CODE[kind], g, 0, [cells[i] for i in ins], [cells[i] for i in outs], c.gen_shape(g)))
        self.base_sum_rows = {}
        for row in range(c.n):
            kind, p = c.gate(row)[:2]
            cand = [(code, row, sub, [(row, col) for col in i if col < c.R], [(row, col) for col in o if col < c.R], p)
                    for code, sub, i, o in row_ops(kind, p, c.lc(row, 0), c.lc(row, 1))]
            kept = [op for op in cand if any(c.key(cell) in slotted for cell in op[3] + op[4])]
            if kind == G_BASE_SUM and kept:
                kept = cand
                self.base_sum_rows[row] = (len(self.ops), len(self.ops) + 1)
            slotted |= {c.key(cell) for op in kept for cell in op[4]}
            self.ops += kept
        self.slotted = slotted
        # an op's inputs are the input cells that have a slot in the end; every other one reads as zero
        self.ops = [(code, idx, sub, [cell for cell in i if c.key(cell) in slotted], o, p) for code, idx, sub, i, o, p in self.ops]

    def root(self, cell):
        k = self.c.key(cell)
        return self.find(k) if k in self.in_class else k

    def slots(self):
        """{cell key: slot} in planhost.hpp's order: classes by their smallest key, then seeds, generator cells, rows"""
        c, slot_of_root, out = self.c, {}, {}
        for k in sorted(self.in_class):
            out[k] = slot_of_root.setdefault(self.find(k), len(slot_of_root))
        nxt = len(slot_of_root)
        for code, idx, sub, i, o, p in self.ops:
            named = (c.gen_cells(idx) if code in (OP_EQUALITY, OP_BIGUINT_DIVREM) else
                     [(idx, col) for col in range(min(c.gate(idx)[1][1] + 1, c.R))] if code in (OP_BASE_SPLIT, OP_BASE_JOIN) else o)
            for cell in named:
                if c.key(cell) not in out:
                    out[c.key(cell)] = nxt
                    nxt += 1
        return out, nxt


def predict(c, seeds):
    """("plan",) or ("refused", kind, (row, col)): kind "a seed is missing" or "dependency cycle" (planhost.hpp, "what the schedule did
    not reach": the smallest key among the unreached cells that no op produces, else that only limbs -> sum directions produce;
    otherwise the smallest unreached key of all is a cycle's)."""
    S = _Ops(c, seeds)
    reached, fired, progress = set(), [False] * len(S.ops), True
    twin = {a: b for a, b in S.base_sum_rows.values()}
    twin.update({b: a for a, b in twin.items()})
    while progress:
        progress = False
        for k, (code, idx, sub, i, o, p) in enumerate(S.ops):
            if not fired[k] and not (k in twin and fired[twin[k]]) and all(S.root(cell) in reached for cell in i):
                fired[k] = progress = True
                reached |= {S.root(cell) for cell in o}
    producer = {}
    for code, idx, sub, i, o, p in S.ops:
        for cell in o:
            r = S.root(cell)
            producer[r] = (producer.get(r) or 2) if code == OP_BASE_JOIN else 1
    unreached = sorted(k for k in S.slotted if S.root(c.cell(k)) not in reached)
    if not unreached:
        return ("plan",)
    for want in (None, 2):
        for k in unreached:
            if producer.get(S.root(c.cell(k))) == want:
                return "refused", "a seed is missing", c.cell(k)
    return "refused", "dependency cycle", c.cell(unreached[0])


def schedule(c, seeds):
    """The level rule restated as a plain loop, for the corpus's coverage counts alone (check_plan does not use it): {"level": {op
    index in creation order: level}, "waited": ops that were ready in a level that had written one of their outputs, "joins": BaseSum
    rows that run limbs -> sum, "widest": ops in the widest level, "ops": the ops}."""
    S = _Ops(c, seeds)
    twin = {a: b for a, b in S.base_sum_rows.values()}
    twin.update({b: a for a, b in twin.items()})
    written, level, waited, dead, lvl = {}, {}, set(), set(), 0
    left = set(range(len(S.ops)))
    while left:
        cur = sorted(k for k in left if k not in dead and all(written.get(S.root(cell), lvl) < lvl for cell in S.ops[k][3]))
        if not cur:
            break
        for k in cur:
            roots = [S.root(cell) for cell in S.ops[k][4]]
            if any(written.get(r) == lvl for r in roots):
                waited.add(k)
                continue
            level[k] = lvl
            left.discard(k)
            if k in twin:
                dead.add(twin[k])
                left.discard(twin[k])
            for r in roots:
                written.setdefault(r, lvl)
        lvl += 1
    width = {}
    for k, v in level.items():
        width[v] = width.get(v, 0) + 1
    return dict(level=level, waited=waited, joins=[S.ops[k][1] for k in level if S.ops[k][0] == OP_BASE_JOIN], widest=max(width.values(), default=0),
                ops=S.ops, S=S)


# ---- evaluate: the matrix, plan-free -------------------------------------------------------------------------------------------------
def fill(c, m):
    """fill_witness: every row's generator on the final row, straight on the matrix m[col][row]; BaseSum runs sum -> limbs"""
    for row in range(c.n):
        kind, p = c.gate(row)[:2]
        for code, sub, _, _ in row_ops(kind, p):
            if code == OP_BASE_JOIN:
                continue
            for col, v in run_body(code, p, sub, lambda col: m[col][row], lambda i: c.lc(row, i))[0]:
                m[col][row] = v
    return m


def _finish(c, seeds, values, routed_value):
    m = [[0] * c.n for _ in range(c.W)]
    for col in range(c.R):
        for row in range(c.n):
            m[col][row] = routed_value((row, col))
    for (row, col), v in zip(seeds, values):
        if col >= c.R:
            m[col][row] = v
    return fill(c, m)


def evaluate(c, seeds, values, trace=None):
    """("ok", matrix [W][n]) | ("contradiction", sort) | ("stuck", None).  Seeds set their cells, a copy class shares one value, an op
    fires once all of its inputs that anything can set are known, a cell that nothing sets reads as zero; sort: "noncanonical" (a seed
    >= p), "compare" (two sources disagree on a class), "reject" (a generator's inputs admit no output).  trace: a list that receives (op code, the values the body read) per op."""
    S = _Ops(c, seeds)
    val = {}
    if any(v >= P for v in values):
        return "contradiction", "noncanonical"
    for (row, col), v in zip(seeds, values):
        if col < c.R and val.setdefault(S.root((row, col)), v) != v:
            return "contradiction", "compare"
    settable = set(val) | {S.root(cell) for op in S.ops for cell in op[4]}
    todo, progress = [op for op in S.ops if op[0] != OP_SEED], True
    while progress and todo:
        progress, later = False, []
        for op in todo:
            code, idx, sub, i, o, p = op
            if any(S.root(cell) in settable and S.root(cell) not in val for cell in i):
                later.append(op)
                continue
            progress, read = True, []

            def seen(v):
                read.append(v)
                return v
            if code in (OP_EQUALITY, OP_BIGUINT_DIVREM):
                cells = c.gen_cells(idx)
                sets, rej = run_body(code, p, sub, lambda k: seen(val.get(S.root(cells[k]), 0)), None)
                sets = [(cells[k], v) for k, v in sets]
            else:
                sets, rej = run_body(code, p, sub, lambda col: seen(val.get(S.root((idx, col)), 0) if col < c.R else 0), lambda k: c.lc(idx, k))
                sets = [((idx, col), v) for col, v in sets if col < c.R]
            if trace is not None:
                trace.append((code, read))
            if rej:
                return "contradiction", "reject"
            for cell, v in sets:
                if val.setdefault(S.root(cell), v) != v:
                    return "contradiction", "compare"
        todo = later
    if todo:
        return "stuck", None
    return "ok", _finish(c, seeds, values, lambda cell: val.get(S.root(cell), 0))


# ---- plans ---------------------------------------------------------------------------------------------------------------------------
class Plan:
    """an exported plan: cell_slot [R][n], ops [ops] (index | (code | sub << 8) << 32), level_off [levels + 1], gen_off [generators + 1],
    gen_table (flat, one word per cell a generator names); counts: (ops, levels, widest, slots, seeds) as the library reports them"""

    def __init__(self, cell_slot, ops, level_off, gen_off=None, gen_table=None, counts=None):
        self.cell_slot = [[int(x) for x in col] for col in cell_slot]
        self.ops = [int(x) for x in ops]
        self.level_off = [int(x) for x in level_off]
        self.gen_table = [int(x) for x in gen_table.reshape(-1)] if gen_table is not None else []
        self.gen_off = [int(x) for x in gen_off] if gen_off is not None else None
        self.counts = tuple(int(x) for x in counts) if counts is not None else None

    def copy(self):
        q = Plan.__new__(Plan)
        q.cell_slot, q.ops, q.level_off = [list(col) for col in self.cell_slot], list(self.ops), list(self.level_off)
        q.gen_table, q.gen_off, q.counts = list(self.gen_table), None if self.gen_off is None else list(self.gen_off), self.counts
        return q

    def decoded(self):
        return [(o & 0xFFFFFFFF, (o >> 32) & 0xFF, o >> 40) for o in self.ops]


class PlanError(AssertionError):
    pass


def _need(cond, *what):
    if not cond:
        raise PlanError(" ".join(str(w) for w in what))


def check_plan(c, seeds, plan):
    """Raises PlanError unless `plan` is a valid plan of circuit c for `seeds` (the circuit's own generator list).  Nothing here follows
    the compilers' way of finding a schedule: the slots are those of the stated order, and the levels are checked as properties."""
    S = _Ops(c, seeds)
    ngen = len(c.gens)
    # -- slots: one per class and per lone cell that a seed, a generator or an active op names, in the stated order
    want, n_slots = S.slots()
    _need(len(plan.cell_slot) == c.R and all(len(col) == c.n for col in plan.cell_slot), "cell_slot is not [R][n]")
    for col in range(c.R):
        for row in range(c.n):
            w = plan.cell_slot[col][row]
            exp = want.get(c.key((row, col)))
            _need((w == UNSET) if exp is None else (w != UNSET and w & ~WRITER == exp), "slot of cell", (row, col), "is", hex(w), "expected", exp)
    # -- the generator table: the cells in list order
    off = plan.gen_off if plan.gen_off is not None else [4 * g for g in range(ngen + 1)]
    _need(off == [sum(sum(c.gen_shape(g)) for g in range(k)) for k in range(ngen + 1)], "gen_off", off)
    _need(len(plan.gen_table) == off[-1], "gen_table has", len(plan.gen_table), "words")
    for g in range(ngen):
        _need([w & ~WRITER for w in plan.gen_table[off[g]:off[g + 1]]] == [c.key(cell) for cell in c.gen_cells(g)], "table words of generator", g)
    # -- the ops: every seed, every generator, every active row op, one direction per BaseSum row; sorted by (level, creation order)
    creation = {(idx, code, sub): k for k, (code, idx, sub, _, _, _) in enumerate(S.ops)}
    recs = plan.decoded()
    _need(len(set(recs)) == len(recs), "an op is scheduled twice")
    _need(all(r in creation for r in recs), "an op that the circuit does not hold:", [r for r in recs if r not in creation][:3])
    lo = plan.level_off
    _need(lo[0] == 0 and lo[-1] == len(recs) and all(a <= b for a, b in zip(lo, lo[1:])), "level_off", lo[:8])
    level = {}
    for lvl in range(len(lo) - 1):
        ks = [creation[r] for r in recs[lo[lvl]:lo[lvl + 1]]]
        _need(ks == sorted(ks), "level", lvl, "is not in creation order")
        level.update({k: lvl for k in ks})
    dropped = {}
    for row, (a, b) in S.base_sum_rows.items():
        _need((a in level) != (b in level), "BaseSum row", row, "needs exactly one of its two directions")
        dropped[b if a in level else a] = a if a in level else b
    _need(set(level) | set(dropped) == set(range(len(S.ops))), "ops missing from the schedule:", sorted(set(range(len(S.ops))) - set(level) - set(dropped))[:4])
    # -- writer bits.  A listed generator's are its table words'.  Everything else shares cell_slot's bit of the cell: where a seed
    #    and a row op have one cell as their output the bit is the seed's, and the row op compares there
    seed_cell = {c.key(s) for s in S.seeds}

    def has_bit(k, pos):
        code, idx, sub, i, o, p = S.ops[k]
        if code in (OP_EQUALITY, OP_BIGUINT_DIVREM):
            return bool(plan.gen_table[off[idx] + len(gen_op(p)[0]) + pos] & WRITER)
        key = c.key(o[pos])
        if code != OP_SEED and key in seed_cell:
            return False
        return bool(plan.cell_slot[o[pos][1]][o[pos][0]] & WRITER)
    derivers = {}
    for k in level:
        for pos, cell in enumerate(S.ops[k][4]):
            derivers.setdefault(want[c.key(cell)], []).append((level[k], k, pos))
    writer = {}
    for s, ds in derivers.items():
        ws = [x for x in ds if has_bit(x[1], x[2])]
        _need(len(ws) == 1, "slot", s, "has", len(ws), "writer bits among", ds[:4])
        _need(ws[0] == min(ds), "slot", s, "is written by", ws[0], "but first derived by", min(ds))
        writer[s] = ws[0]
    # a bit on a cell that is nobody's output
    outs = {c.key(cell) for k in level for cell in S.ops[k][4] if S.ops[k][0] not in (OP_EQUALITY, OP_BIGUINT_DIVREM)}
    for col in range(c.R):
        for row in range(c.n):
            w = plan.cell_slot[col][row]
            _need(w == UNSET or not w & WRITER or c.key((row, col)) in outs, "writer bit on cell", (row, col), "that no scheduled op sets")
    for g in range(ngen):
        n_in = len(gen_op(c.gen_shape(g))[0])
        _need(not any(w & WRITER for w in plan.gen_table[off[g]:off[g] + n_in]), "writer bit on an input of generator", g)
    # -- levels: one above the latest input's writer; while that level already wrote one of the outputs, the next one
    def earliest(k, skip=None):
        code, idx, sub, i, o, p = S.ops[k]
        ins = [want[c.key(cell)] for cell in i]
        for s in ins:
            _need(s in writer, "slot", s, "is read by op", S.ops[k][:3], "but never written")
        if skip is not None and any(writer[s][1] == skip for s in ins):
            return None                                     # (it waits for the very op that was kept)
        lvl = 1 + max((writer[s][0] for s in ins), default=-1)
        taken = {writer[want[c.key(cell)]][0] for cell in o if want[c.key(cell)] in writer and writer[want[c.key(cell)]][1] != k}
        while lvl in taken:
            lvl += 1
        return lvl
    for k, lvl in level.items():
        _need(earliest(k) == lvl, "op", S.ops[k][:3], "sits in level", lvl, "not in", earliest(k))
        for pos, cell in enumerate(S.ops[k][4]):
            w = writer[want[c.key(cell)]]
            _need(w[1:] == (k, pos) or w[0] < lvl, "op", S.ops[k][:3], "compares in the level of its slot's writer")
    for gone, kept in dropped.items():
        e = earliest(gone, skip=kept)
        _need(e is None or (e, gone) > (level[kept], kept), "BaseSum row", S.ops[gone][1], "runs the direction that is reached second")
    # -- counts
    widest = max((b - a for a, b in zip(lo, lo[1:])), default=0)
    if plan.counts is not None:
        _need(plan.counts == (len(recs), len(lo) - 1, widest, n_slots, len(S.seeds)), "counts", plan.counts, (len(recs), len(lo) - 1, widest, n_slots, len(S.seeds)))
    return dict(levels=len(lo) - 1, widest=widest, slots=n_slots, level=level, ops=S.ops, writer=writer, want=want, dropped=dropped)


def interpret(c, seeds, plan, values):
    """The plan run op by op in `ops` order over a slot array, with the walk's accessor rules: a column >= R reads 0 and is not set, a
    cell without a slot reads 0, a writer stores and everyone else compares, a seed >= p rejects.  Then the scatter, the seeds on
    columns >= R and fill.  Returns (matrix, None) or (matrix, (row, col)): the cell of the smallest contradiction word, for a listed
    generator the cell its table names."""
    off = plan.gen_off if plan.gen_off is not None else [4 * g for g in range(len(c.gens) + 1)]
    slot = lambda row, col: plan.cell_slot[col][row]  # noqa: E731
    seed_cell = {tuple(s) for s in seeds}
    val, err = {}, []
    for pos, (idx, code, sub) in enumerate(plan.decoded()):
        def reject(col):
            err.append((pos, col))
        if code in (OP_EQUALITY, OP_BIGUINT_DIVREM):
            words = plan.gen_table[off[idx]:off[idx + 1]]
            cells = [c.cell(w & ~WRITER) for w in words]
            sets, rej = run_body(code, c.gen_shape(idx), sub, lambda k: val.get(slot(*cells[k]) & ~WRITER, 0), None)
            for k, v in sets:
                s = slot(*cells[k]) & ~WRITER
                if words[k] & WRITER:
                    val[s] = v
                elif val.get(s, 0) != v:
                    reject(k)
            for k in rej:
                reject(k)
            continue
        row = seeds[idx][0] if code == OP_SEED else idx

        def get(col):
            return 0 if col >= c.R or slot(row, col) == UNSET else val.get(slot(row, col) & ~WRITER, 0)
        if code == OP_SEED:
            sets, rej = ([], [seeds[idx][1]]) if values[idx] >= P else ([(seeds[idx][1], values[idx])], [])
        else:
            sets, rej = run_body(code, c.gate(row)[1], sub, get, lambda k: c.lc(row, k))
        for col, v in sets:
            if col >= c.R or slot(row, col) == UNSET:
                continue
            s = slot(row, col)
            if s & WRITER and (code == OP_SEED or (row, col) not in seed_cell):   # (a seeded cell's bit is the seed's)
                val[s & ~WRITER] = v
            elif val.get(s & ~WRITER, 0) != v:
                reject(col)
        for col in rej:
            reject(col)
    m = _finish(c, seeds, values, lambda cell: 0 if slot(*cell) == UNSET else val.get(slot(*cell) & ~WRITER, 0))
    if not err:
        return m, None
    pos, col = min(err)
    idx, code, sub = plan.decoded()[pos]
    if code in (OP_EQUALITY, OP_BIGUINT_DIVREM):
        return m, c.cell(plan.gen_table[off[idx] + col] & ~WRITER)
    return m, ((seeds[idx][0] if code == OP_SEED else idx), col)
