"""A seeded corpus of random circuits for the witness plan and the level walk (test infrastructure; the model is witness_model.py).
Every circuit is built forward: a row is placed, each input of each of its ops is fed either a fresh seed, a copy from a cell whose
value is already known, or nothing (it reads as zero), and the values are kept as the builder goes -- so a circuit is solvable and
acyclic unless a step below breaks it on purpose.  `corpus(seed)` is deterministic: the same list on every machine.
A `Case` holds the circuit, its seed cells, a satisfying value set, failing value sets (one perturbed seed each), and for a refused
circuit nothing but the cells; what a case is expected to do is the model's to say (witness_model.predict / evaluate)."""
import random

import witness_model as wm
from witness_model import (G_ARITHMETIC, G_BASE_SUM, G_COMPARISON, G_CONSTANT, G_NOOP, G_POSEIDON, G_RANDOM_ACCESS, G_U32_ADD_MANY, G_U32_ARITHMETIC,
                           G_U32_RANGE_CHECK, G_U32_SUBTRACTION, P)

EDGE_WORDS = [0, 1, 2, 3, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1, 2**63, P - 2**32, P - 2**32 + 1, P - 2, P - 1]
KINDS = [G_CONSTANT, G_ARITHMETIC, G_BASE_SUM, G_RANDOM_ACCESS, G_POSEIDON, G_U32_ARITHMETIC, G_U32_ADD_MANY, G_U32_SUBTRACTION, G_U32_RANGE_CHECK,
         G_COMPARISON]
SHAPES = [(234, 80), (135, 80)]
DIVREM_SHAPES = [(1, 1, 1, 1), (3, 2, 2, 2), (2, 4, 0, 4), (2, 1, 2, 1)]


def gate_degree(kind, p):
    """the degree a gate declares: its constraints' own, capped at what one selector group takes (8) -- `honest` says whether it is"""
    deg = {G_NOOP: 0, G_CONSTANT: 1, G_ARITHMETIC: 3, G_POSEIDON: 7}.get(kind)
    if kind == G_BASE_SUM:
        deg = p[0]
    elif kind == G_RANDOM_ACCESS:
        deg = p[0] + 1
    elif kind == G_COMPARISON:
        deg = max(1 << -(-p[0] // p[1]), 3)
    elif deg is None:
        deg = 4
    return min(deg, 8), deg <= 8


def gate_constants(kind, p):
    return {G_CONSTANT: p[0] if kind == G_CONSTANT else 0, G_ARITHMETIC: 2, G_RANDOM_ACCESS: p[2] if kind == G_RANDOM_ACCESS else 0}.get(kind, 0)


class Case:
    def __init__(self, name, circuit, seeds, values, bad=(), tags=(), provable=False):
        self.name, self.circuit, self.seeds, self.values = name, circuit, [tuple(s) for s in seeds], list(values) if values is not None else None
        self.bad, self.tags, self.provable = [list(b) for b in bad], set(tags), provable

    def __repr__(self):
        return "Case(%s)" % self.name


class Expected:
    """what the model expects of a case, computed once and shared by the tests: the prediction, the good set's matrix, the failing
    sets' outcomes, the values every op read (`trace`) and the restated schedule"""

    def __init__(self, case):
        self.case = case
        self.predict = wm.predict(case.circuit, case.seeds)
        self.trace = []
        if case.values is not None:
            self.good = wm.evaluate(case.circuit, case.seeds, case.values, self.trace)
            self.bad = [wm.evaluate(case.circuit, case.seeds, v, self.trace) for v in case.bad]
            self.schedule = wm.schedule(case.circuit, case.seeds)


class Builder:
    def __init__(self, rng, d, W=234, R=80, pool="mixed"):
        self.rng, self.d, self.n, self.W, self.R, self.pool = rng, d, 1 << d, W, R, pool
        self.rows, self.consts, self.copies, self.gens = [], {}, [], []
        self.seeds, self.known, self.derived, self.fed = {}, {}, [], set()
        self.tags, self.honest = set(), True

    # ---- values
    def word(self, pool=None):
        pool = pool or self.pool
        r = self.rng.random()
        if pool == "u32" or (pool == "mixed" and r < 0.4):
            return self.rng.randrange(1 << 32)
        if pool == "edge" or (pool == "mixed" and r < 0.7):
            return self.rng.choice(EDGE_WORDS)
        return self.rng.randrange(P)

    # ---- rows
    def free_rows(self):
        return self.n - 1 - len(self.rows)            # (the last row stays a NoopGate row: the listed generators' own cells live there)

    def add_row(self, kind, p, consts=()):
        assert self.free_rows() > 0 and wm.gate_wires_used(kind, p) <= self.W, (kind, p)
        self.rows.append((kind, tuple(p)))
        self.consts[len(self.rows) - 1] = list(consts)
        self.honest &= gate_degree(kind, p)[1]
        return len(self.rows) - 1

    def seed(self, cell, value):
        assert cell not in self.seeds
        self.seeds[cell] = value
        if cell[1] < self.R:
            self.known[cell] = value
            self.fed.add(cell)

    def copy(self, src, dst):
        assert src[1] < self.R and dst[1] < self.R and src != dst
        self.copies.append((src[0], src[1], dst[0], dst[1]))
        self.known[dst] = self.known[src]
        self.fed.add(dst)

    def pick(self, ok=lambda v: True, among=None):
        cells = [c for c in (among if among is not None else list(self.known)) if ok(self.known[c])]
        return self.rng.choice(cells) if cells else None

    def feed(self, cell, ok=lambda v: True, draw=None, how=None):
        """give an input cell its value: "seed", "copy" (from a known cell whose value passes `ok`) or "none" (it reads as zero)"""
        if cell[1] >= self.R:
            return 0
        how = how or self.rng.choices(["seed", "copy", "none"], [5, 4, 1 if ok(0) else 0])[0]
        if how == "copy":
            src = self.pick(ok)
            if src is not None and src != cell:
                self.copy(src, cell)
                return self.known[cell]
            how = "seed"
        if how == "seed":
            for _ in range(200):
                v = draw() if draw else self.word()
                if ok(v):
                    break
            else:
                raise AssertionError("no value passes")
            self.seed(cell, v)
            return v
        self.tags.add("slotless_input")
        return 0

    def run(self, row):
        """the row's ops on the known values: its outputs become known, derived cells"""
        kind, p = self.rows[row]
        lc = lambda i: self.consts[row][i] if i < len(self.consts[row]) else 0  # noqa: E731
        for code, sub, ins, outs in wm.row_ops(kind, p, lc(0), lc(1)):
            if code == wm.OP_BASE_JOIN:
                continue
            sets, rej = wm.BODY[code](p, sub, lambda col: self.known.get((row, col), 0) if col < self.R else 0, lc)
            assert not rej, (kind, p, rej)
            for col, v in sets:
                if col < self.R and (row, col) not in self.known:
                    self.known[(row, col)] = v
                    self.derived.append((row, col))

    # ---- a row of every kind, with its inputs fed
    def place(self, kind, p=None, how=None, draw=None):
        rng = self.rng
        p = p or self.params(kind)
        consts = []
        if kind == G_CONSTANT:
            consts = [self.word() for _ in range(p[0])]
        elif kind == G_ARITHMETIC:
            consts = [rng.choice([0, 1, 1, self.word()]), rng.choice([0, 1, 1, self.word()])]
        elif kind == G_RANDOM_ACCESS:
            consts = [self.word() for _ in range(p[2])]
        row = self.add_row(kind, p, consts)
        cap = (1 << 32) if self.pool == "u32" else P            # (a u32 circuit stays satisfiable: its gates see 32-bit words only)
        f = lambda col, ok=lambda v: v < cap, dr=draw: self.feed((row, col), ok, dr, how)  # noqa: E731
        if kind == G_BASE_SUM:                                  # (every cell of an active BaseSum row has a slot: none may stay unfed)
            B, L = p
            top = min(B ** L, cap)
            how = how or rng.choice(["seed", "copy"])
            if rng.random() < 0.4 and B ** L < 2 ** 63:          # limbs first: the sum is theirs
                for i in range(L):
                    self.feed((row, 1 + i), lambda v: v < B, lambda: rng.randrange(B), rng.choice(["seed", "copy"]))
                self.known[(row, 0)] = wm.body_base_join(p, 0, lambda col: self.known.get((row, col), 0), None)[0][0][1]
                self.derived.append((row, 0))
            else:
                f(0, lambda v: v < top, lambda: self.word() % top)
        elif kind == G_POSEIDON:
            for col in range(12):
                f(col)
            self.feed((row, 24), lambda v: v < 2, lambda: rng.randrange(2), "seed")
        elif kind == G_ARITHMETIC:
            for i in range(p[0]):
                if consts[0]:
                    f(4 * i), f(4 * i + 1)
                if consts[1]:
                    f(4 * i + 2)
        else:
            for code, sub, ins, outs in wm.row_ops(kind, p):
                for col in ins:
                    f(col)
        self.run(row)
        return row

    def params(self, kind):
        rng, W = self.rng, self.W
        if kind == G_CONSTANT:
            return (rng.randint(1, 4),)
        if kind == G_ARITHMETIC:
            return (rng.choice([1, 2, 3, 5, 20]),)
        if kind == G_BASE_SUM:
            return (rng.randint(2, 8), rng.choice([1, 2, 3, 7, 8, 13, 21, 32, 63, 64]))
        if kind == G_RANDOM_ACCESS:
            bits = rng.randint(1, 6)
            extra = rng.randint(0, 2)
            most = (W - extra) // (2 + (1 << bits) + bits)
            return (bits, rng.randint(1, min(most, 3)), extra)
        if kind == G_POSEIDON:
            return ()
        if kind == G_U32_ARITHMETIC:
            return (rng.randint(1, W // 38),)
        if kind == G_U32_ADD_MANY:
            na = rng.choice([0, 1, 2, 5, 16])
            return (na, rng.randint(1, min(3, W // (na + 21))))
        if kind == G_U32_SUBTRACTION:
            return (rng.randint(1, min(4, W // 21)),)
        if kind == G_U32_RANGE_CHECK:
            return (rng.randint(1, min(4, W // 17)),)
        if kind == G_COMPARISON:
            cb = rng.randint(1, 4)
            nc = rng.randint(1, min(64 // cb, 14))
            return (cb * nc - rng.randint(0, cb - 1), nc)
        raise AssertionError(kind)

    # ---- deliberate structure
    def twin(self, row):
        """the row placed again, every input a copy of the first one's, every routed output copied back: two ops derive one class, both
        ready in one level"""
        kind, p = self.rows[row]
        new = self.add_row(kind, p, self.consts[row])
        for col in range(min(wm.gate_wires_used(kind, p), self.R)):
            if (row, col) in self.fed:
                self.copy((row, col), (new, col))
        self.run(new)
        outs = [(new, col) for r, col in self.derived if r == new]
        for r, col in self.rng.sample(outs, min(len(outs), 3)):
            self.copies.append((row, col, new, col))
        self.tags.add("two_derive")
        return new

    def seed_derived(self, on_output):
        """a seed on a class that an op derives: on the op's own output cell, or on a fresh cell copied to it"""
        cands = [c for c in self.derived if c not in self.seeds]
        if not cands:
            return None
        cell = self.rng.choice(cands)
        if on_output:
            self.seeds[cell] = self.known[cell]
            self.tags.add("seed_on_output")
        else:
            fresh = self.spare()
            self.copies.append((cell[0], cell[1], fresh[0], fresh[1]))
            self.known[fresh] = self.known[cell]
            self.seeds[fresh] = self.known[cell]
        self.tags.add("seed_derived")
        return cell

    def spare(self):
        """an unused routed cell of the last row"""
        self._spare = getattr(self, "_spare", 0) + 1
        assert self._spare <= self.R
        return (self.n - 1, self.R - self._spare)

    def seed_high_column(self):
        """a seed on a gate-internal column: a NoopGate row keeps it, any other row's generator writes over it"""
        row = self.rng.choice([self.n - 1] + list(range(len(self.rows))))
        cell = (row, self.rng.randrange(self.R, self.W))
        if cell not in self.seeds:
            self.seeds[cell] = self.word()
            self.tags.add("seed_high_column")

    def equality(self, shared_output=False):
        """an equality generator over known cells; `equal` and `inv` are spare cells, or (shared_output) `inv` is also the output of an
        ArithmeticGate operation 0 * .. + 1 * addend whose addend is seeded with the inverse"""
        x = self.pick()
        y = self.pick(lambda v: v == self.known[x]) if self.rng.random() < 0.3 else self.pick()
        if x is None or y is None:
            return
        diff = (self.known[x] - self.known[y]) % P
        eq, iv = self.spare(), self.spare()
        if shared_output and self.free_rows() > 0:
            row = self.add_row(G_ARITHMETIC, (2,), [0, 1])
            self.seed((row, 2), wm.inv(diff) if diff else 0)
            self.seed((row, 6), self.word())
            self.run(row)
            iv = (row, 3)
            self.tags.add("generator_shares_output")
        self.gens.append(("equality", ([x], [y], [eq], [iv])))
        for cell, v in ((eq, 1 if diff == 0 else 0), (iv, wm.inv(diff) if diff else 0)):
            if cell not in self.known:
                self.known[cell] = v
                self.derived.append(cell)

    def divrem(self, shape, pool=None):
        la, lb, ld, lr = shape
        for _ in range(100):
            a_cells = [self.spare() for _ in range(la)]
            b_cells = [self.spare() for _ in range(lb)]
            av, bv = [self.word(pool or "u32") for _ in range(la)], [self.word(pool or "u32") for _ in range(lb)]
            vals = av + bv
            sets, rej = wm.body_biguint_divrem(shape, 0, lambda k: vals[k], None)
            if not rej:
                break
            self._spare -= la + lb
        else:
            raise AssertionError("no dividend fits")
        for cell, v in zip(a_cells + b_cells, vals):
            self.seed(cell, v)
        out_cells = [self.spare() for _ in range(ld + lr)]
        self.gens.append(("biguint_divrem", (a_cells, b_cells, out_cells[:ld], out_cells[ld:])))
        for cell, (k, v) in zip(out_cells, sets):
            self.known[cell] = v
            self.derived.append(cell)

    # ---- the circuit
    def circuit(self):
        decl = sorted({(gate_degree(k, p)[0], k, p) for k, p in self.rows} | {(0, G_NOOP, ())})
        index = {(k, p): i for i, (deg, k, p) in enumerate(decl)}
        gates = [(k, p, deg, gate_constants(k, p)) for deg, k, p in decl]
        nk = max([len(c) for c in self.consts.values()] + [0])
        consts = [[(self.consts[r][i] if r < len(self.rows) and i < len(self.consts[r]) else 0) for r in range(self.n)] for i in range(nk)]
        return wm.Circuit(self.d, self.W, self.R, gates, [index[kp] for kp in self.rows], consts, self.copies, self.gens)

    def case(self, name, provable=False):
        seeds = list(self.seeds)
        return Case(name, self.circuit(), seeds, [self.seeds[s] for s in seeds], tags=self.tags, provable=provable and self.honest and not self.gens)


# ---- failing value sets ----------------------------------------------------------------------------------------------------------
def perturbed(rng, case):
    """Value sets with one seed changed, at most one per sort of failure: another value on a seed of a class that an op derives (a
    compare mismatch), an edge word where a generator rejects it (a sum too large for its limbs, a zero divisor ..), a value >= p.
    Only what the model finds contradictory is kept."""
    c, out, sorts = case.circuit, [], set()
    S = wm.schedule(c, case.seeds)["S"]
    derived = {S.root(cell) for op in S.ops if op[0] != wm.OP_SEED for cell in op[4]}
    on_derived = [k for k, s in enumerate(case.seeds) if s[1] < c.R and S.root(s) in derived]
    tries = [(k, (case.values[k] + 1) % P) for k in rng.sample(on_derived, min(2, len(on_derived)))]
    tries += [(rng.randrange(len(case.seeds)), rng.choice(EDGE_WORDS)) for _ in range(5)]
    tries += [(rng.randrange(len(case.seeds)), rng.choice([P, P + 1, 2**64 - 1]))]
    for k, val in tries:
        v = list(case.values)
        v[k] = val
        got = wm.evaluate(c, case.seeds, v) if v != case.values else ("ok",)
        if got[0] == "contradiction" and got[1] not in sorts:
            sorts.add(got[1])
            out.append(v)
    return out


# ---- the circuits ----------------------------------------------------------------------------------------------------------------
def mixed(rng, name, d, W, R, pool, kinds=None, structure=True, gens=True):
    b = Builder(rng, d, W, R, pool)
    b.place(G_CONSTANT)
    kinds = kinds or KINDS
    while b.free_rows() > (3 if structure else 0):
        kind = rng.choice(kinds)
        if kind == G_POSEIDON and rng.random() < 0.6:
            continue
        row = b.place(kind)
        if structure and b.free_rows() > 3 and rng.random() < 0.3:
            b.twin(row)
    if structure:
        for on_output in (True, False):
            if rng.random() < 0.6:
                b.seed_derived(on_output)
        if rng.random() < 0.6:
            b.seed_high_column()
        if gens and pool != "u32":
            for _ in range(rng.randint(0, 2)):
                b.equality(shared_output=rng.random() < 0.5)
            if rng.random() < 0.5:
                b.divrem(rng.choice(DIVREM_SHAPES))
    return b


def edge_circuit(rng, kind, d=5):
    """every edge word as the first input of an op of `kind`, the other inputs from the pools; a word that the op rejects goes to a
    failing value set instead (the good set keeps a value that passes)"""
    b = Builder(rng, d, 234, 80, "mixed")
    swaps = []
    for w in EDGE_WORDS:
        if b.free_rows() < 1:
            break
        p = b.params(kind)
        if kind == G_BASE_SUM:
            p = (2, 64) if w >= 2 ** 32 else (rng.randint(2, 8), rng.choice([3, 8, 21]))
        if kind == G_POSEIDON and len([r for r in b.rows if r[0] == G_POSEIDON]) >= 4:
            break
        row = b.add_row(kind, p, [1, 1] if kind == G_ARITHMETIC else [b.word() for _ in range(gate_constants(kind, p))])
        ins = [col for code, sub, i, o in wm.row_ops(kind, p) for col in i if code != wm.OP_BASE_JOIN]
        for j, col in enumerate(ins):
            if col < b.R:
                fits = (lambda v: v < p[0] ** p[1]) if kind == G_BASE_SUM else (lambda v: True)
                if j == 0 and fits(w):
                    b.seed((row, col), w)
                elif j == 0:
                    b.feed((row, col), fits, how="seed")
                    swaps.append(((row, col), w))
                elif kind == G_POSEIDON and col == 24:
                    b.seed((row, col), len(b.rows) & 1)
                elif kind == G_POSEIDON:
                    b.seed((row, col), EDGE_WORDS[(12 * len(b.rows) + j) % len(EDGE_WORDS)])
                else:
                    b.feed((row, col), fits, how=rng.choice(["seed", "seed", "copy"]))
        b.run(row)
    return b, swaps


def edge_join(rng):
    """limbs -> sum rows whose first limb is an edge word: below the base it is the good set's, at or above it a failing set's"""
    b = Builder(rng, 5, 234, 80, "mixed")
    swaps = []
    for w in EDGE_WORDS:
        B, L = rng.randint(2, 8), rng.choice([1, 2, 5, 16])
        row = b.add_row(G_BASE_SUM, (B, L))
        for i in range(L):
            b.seed((row, 1 + i), w if i == 0 and w < B else rng.randrange(B))
        if w >= B:
            swaps.append(((row, 1), w))
        b.known[(row, 0)] = wm.body_base_join((B, L), 0, lambda col: b.known.get((row, col), 0), None)[0][0][1]
        b.derived.append((row, 0))
    return b, swaps


def edge_generators(rng, which):
    """the listed generators on edge words: x of an equality generator; the one-limb dividend ("divrem_a") or divisor ("divrem_b") of
    a div-rem generator -- a word the division rejects (a zero divisor, a quotient or remainder of more than 32 bits) goes to a
    failing set and the good set keeps a 32-bit word"""
    b = Builder(rng, 5, 234, 80, "mixed")
    b.place(G_CONSTANT)
    swaps = []
    for k, w in enumerate(EDGE_WORDS):
        cells = [b.spare() for _ in range(4)]
        if which == "equality":
            vals = [w, w if k % 4 == 0 else b.word()]
            diff = (vals[0] - vals[1]) % P
            sets = [(2, 1 if diff == 0 else 0), (3, wm.inv(diff) if diff else 0)]
            b.gens.append(("equality", tuple([c] for c in cells)))
        else:
            side = 0 if which == "divrem_a" else 1
            for attempt in range(60):
                vals = [rng.randrange(1, 1 << 32), rng.choice([rng.randrange(1, 1 << 32), rng.randrange(1 << 31, 1 << 32), 2**32, 2**32 + 1, 2**63])]
                if attempt == 59:
                    swaps.append((cells[side], w))            # (the last draw is 32-bit words on both sides: it passes)
                    vals[1] = rng.randrange(1, 1 << 32)
                else:
                    vals[side] = w
                sets, rej = wm.body_biguint_divrem((1, 1, 1, 1), 0, lambda i: vals[i], None)
                if not rej:
                    break
            assert not rej
            b.gens.append(("biguint_divrem", tuple([c] for c in cells)))
        for cell, v in zip(cells[:2], vals):
            b.seed(cell, v)
        for cell, (pos, v) in zip(cells[2:], sets):
            b.known[cell] = v
            b.derived.append(cell)
    return b, swaps


def wide_level(rng):
    """one seeded cell copied to the first multiplicand of 40 x 20 ArithmeticGate operations at d = 6: a level of 800 ops"""
    b = Builder(rng, 6, 234, 80, "mixed")
    hub = b.place(G_CONSTANT, (2,))
    b.seed((b.n - 1, 0), b.word())
    for r in range(40):
        row = b.add_row(G_ARITHMETIC, (20,), [rng.choice([1, 3, P - 1]), rng.choice([0, 1])])
        for i in range(20):
            b.copy((b.n - 1, 0), (row, 4 * i))
            b.copy((hub, i & 1), (row, 4 * i + 1))
            if b.consts[row][1] and i % 3 == 0:
                b.seed((row, 4 * i + 2), b.word())
        b.run(row)
    b.seed_derived(True)
    b.seed_derived(False)
    b.tags.add("wide_level")
    return b


# ---- named cases: the smallest circuit that showed a disagreement between the model and the product, or that a check needs ----------
def seed_on_own_output(rng):
    """A seed on the very cell that an ArithmeticGate operation sets: the seed writes in level 0 and the operation has to COMPARE.  The
    cell's one writer bit once served both, so the operation wrote over a wrong seed value and nobody noticed."""
    b = Builder(rng, 2, 234, 80, "u32")
    row = b.add_row(G_ARITHMETIC, (2,), [1, 1])
    for col in (0, 1, 2, 4, 5, 6):
        b.seed((row, col), b.word())
    b.run(row)
    b.seeds[(row, 3)] = b.known[(row, 3)]
    row2 = b.add_row(G_BASE_SUM, (2, 4))
    b.seed((row2, 0), 11)
    b.run(row2)
    b.seeds[(row2, 2)] = b.known[(row2, 2)]
    case = b.case("seed_on_own_output")
    for cell in ((row, 3), (row2, 2)):
        v = list(case.values)
        v[case.seeds.index(cell)] ^= 1
        case.bad.append(v)
    return case


def borrow_boundary(rng):
    """U32SubtractionGate operations whose x - y - borrow is exactly 2^32, one below and one above: the borrow is set strictly above"""
    b = Builder(rng, 2, 234, 80, "mixed")
    row = b.add_row(G_U32_SUBTRACTION, (4,))
    for i, (x, y, bw) in enumerate([(2**32, 0, 0), (2**32 + 1, 1, 0), (2**32 + 1, 0, 0), (2**32 - 1, 0, 0)]):
        for col, v in zip((5 * i, 5 * i + 1, 5 * i + 2), (x, y, bw)):
            b.seed((row, col), v)
    b.run(row)
    return b.case("borrow_boundary")


def remove_seed(rng, case):
    """the case without one seed that its class needs, or None"""
    order = list(range(len(case.seeds)))
    rng.shuffle(order)
    for k in order[:8]:
        seeds = case.seeds[:k] + case.seeds[k + 1:]
        if wm.predict(case.circuit, seeds)[0] == "refused":
            return Case(case.name + "-seed_removed", case.circuit, seeds, None, tags={"refused"})
    return None


def close_cycle(rng, case):
    """the case with one op's output copied back to one of its own seeded inputs (the seed goes), or None"""
    c = case.circuit
    S = wm.schedule(c, case.seeds)["S"]
    ops = [op for op in S.ops if op[0] not in (wm.OP_SEED, wm.OP_EQUALITY, wm.OP_BIGUINT_DIVREM, wm.OP_BASE_SPLIT, wm.OP_BASE_JOIN) and op[3] and op[4]]
    rng.shuffle(ops)
    for code, idx, sub, ins, outs, p in ops[:8]:
        cell = next((x for x in ins if x in case.seeds), None)
        if cell is None:
            continue
        seeds = [s for s in case.seeds if s != cell]
        c2 = wm.Circuit(c.d, c.W, c.R, c.gates, c.row_gate, c.consts, c.copies + [(outs[0][0], outs[0][1], cell[0], cell[1])], c.gens)
        if wm.predict(c2, seeds)[:2] == ("refused", "dependency cycle"):
            return Case(case.name + "-cycle", c2, seeds, None, tags={"refused"})
    return None


SAFE = [G_CONSTANT, G_ARITHMETIC, G_BASE_SUM, G_POSEIDON, G_U32_ARITHMETIC, G_U32_RANGE_CHECK]   # satisfied by any 32-bit inputs


def _with_swaps(b, swaps, name):
    case = b.case(name)
    for cell, w in swaps:
        v = list(case.values)
        v[case.seeds.index(cell)] = w
        case.bad.append(v)
    return case


def corpus(seed=20240611):
    rng = random.Random(seed)
    cases = []
    # mixed circuits over d, both wire shapes, the pools; a u32 circuit holds gates that 32-bit words satisfy, so it also proves
    plan = [(2, "mixed"), (3, "u32"), (3, "mixed"), (4, "edge"), (4, "u32"), (4, "mixed"), (5, "mixed"), (5, "u32"), (5, "random"), (6, "mixed"),
            (4, "mixed"), (3, "edge"), (5, "edge"), (4, "random"), (5, "mixed"), (4, "u32"), (3, "mixed"), (4, "mixed"), (2, "u32"), (5, "mixed")]
    for k, (d, pool) in enumerate(plan):
        W, R = SHAPES[k % 2]
        b = mixed(rng, "mixed%d" % k, d, W, R, pool, kinds=SAFE if pool == "u32" else None)
        cases.append(b.case("mixed%02d_d%d_%s_%d" % (k, d, pool, W), provable=pool == "u32"))
    # one off-reference routed count (tests/golden/param_circuits.py's R = 40): ops whose columns cross it are gate-internal there
    b = mixed(rng, "routed40", 4, 120, 40, "mixed", kinds=[G_CONSTANT, G_ARITHMETIC, G_BASE_SUM, G_U32_SUBTRACTION, G_U32_RANGE_CHECK, G_COMPARISON])
    cases.append(b.case("routed40_d4_mixed_120"))
    # the edge words into every kind of op
    for kind in KINDS[1:]:
        cases.append(_with_swaps(*edge_circuit(rng, kind), "edge_kind%02d" % kind))
    cases.append(_with_swaps(*edge_join(rng), "edge_join"))
    for which in ("equality", "divrem_a", "divrem_b"):
        cases.append(_with_swaps(*edge_generators(rng, which), "edge_" + which))
    for shape in DIVREM_SHAPES[1:]:
        b = Builder(rng, 3, 234, 80, "u32")
        b.place(G_U32_RANGE_CHECK)
        b.divrem(shape)
        if shape[2]:
            b.divrem(shape, "mixed")
        cases.append(b.case("divrem_%d_%d_%d_%d" % shape))
    cases.append(wide_level(rng).case("wide_level_d6"))
    named = [seed_on_own_output(rng), borrow_boundary(rng)]
    # failing value sets: the model keeps those that contradict
    for case in cases:
        case.bad += perturbed(rng, case)
    # refused circuits: four of either kind
    refused = {"a seed is missing": [], "dependency cycle": []}
    for case in cases:
        for make in (remove_seed, close_cycle):
            r = make(rng, case)
            if r is not None:
                kind = wm.predict(r.circuit, r.seeds)[1]
                if len(refused[kind]) < 4:
                    refused[kind].append(r)
                    break
    return cases + named + refused["a seed is missing"] + refused["dependency cycle"]
