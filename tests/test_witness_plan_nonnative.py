"""The four nonnative generators in the witness plan (csrc/planhost.hpp), without a GPU: the stand-alone printer
(csrc/tests/planhost_print.cpp, g++ only) in its four-argument form on the circuits of tests/nonnative_inputs.py.  The rules are
stated here, not recorded.  Every case runs twice: through the plain build of the printer and through one with
-fsanitize=address,undefined (a host program, run here)."""
import numpy as np
import pytest

import nonnative_inputs as ni
import witness_plan_inputs as wpi
from test_witness_plan_divrem import run_v
from test_witness_plan_generators import printer  # noqa: F401  (the fixture builds the same printer)

W = 0x80000000
OP_SEED = 0


def records(generators):
    """builder.generators() -> (p2gpu_generator_v records [kind | field << 8, shape[4]], flat (row, col) list)."""
    recs, cells = [], []
    for kind, groups, field in generators:
        recs.append([ni.KINDS[kind] | ni.FIELD_IDS[field] << 8] + [len(grp) for grp in groups])
        cells += [c for grp in groups for c in grp]
    return np.array(recs, dtype=np.uint32).reshape(-1, 5), np.array(cells, dtype=np.uint32).reshape(-1, 2)


class Circuit:
    def __init__(self, b):
        self.b, self.blob, self.cells = b, b.blob(), b._layout().cells
        self.d = int(np.frombuffer(bytes(np.ascontiguousarray(self.blob)[:256]), dtype=np.uint32)[2])
        self.seeds = b.seed_cells()
        self.gens = b.generators()
        self.recs, self.flat = records(self.gens)

    def key(self, cell):
        return (int(cell[1]) << self.d) | int(cell[0])


SINGLE = [(kind, field) for kind in ("add", "sub", "mul", "neg", "inv") for field in ni.FIELDS]


@pytest.fixture(scope="module")
def circuits(pkg):
    out = {(kind, field): Circuit(ni.virtual(pkg, kind, field)[0]) for kind, field in SINGLE}
    out["mul44"] = Circuit(ni.virtual(pkg, "mul", ni.BASE, 4, 4)[0])
    out["chain"] = Circuit(ni.chain(pkg, ni.SCALAR)[0])
    for name, c in out.items():
        assert 1 << c.d <= (1 << 9 if name == "chain" else 1 << 7), name
    return out


def writer_levels(c, cell_slot, ops, level_off, table, off):
    """{slot: level of the op that writes it}, from the writer bits of cell_slot (row ops, seeds) and of the table (generators)."""
    lv = wpi.op_levels(ops, level_off)
    gen_level = {idx: l for (idx, code, _), l in lv.items() if code >= 13}
    out = {}
    for g, lvl in gen_level.items():
        for w in table[off[g]:off[g + 1]]:
            if w & W:
                key = int(w) & ~W
                out[int(cell_slot[key >> c.d, key & ((1 << c.d) - 1)]) & ~W] = lvl
    return out, gen_level


@pytest.mark.parametrize("case", SINGLE + ["mul44"], ids=str)
def test_single_operation_plan_follows_the_stated_rules(printer, circuits, tmp_path, case):  # noqa: F811
    c = circuits[case]
    (kind, groups, field), = c.gens
    shape = [len(g) for g in groups]
    want_kind = {"add": "nonnative_add", "sub": "nonnative_sub", "neg": "nonnative_sub", "mul": "nonnative_mul", "inv": "nonnative_inv"}[case[0] if case != "mul44" else "mul"]
    assert kind == want_kind
    if case == "mul44":
        assert shape == [4, 4, 8, 0]
    else:
        assert shape == {"add": [8, 8, 8, 1], "sub": [8, 8, 8, 1], "neg": [0, 8, 8, 1], "mul": [8, 8, 8, 8], "inv": [8, 0, 8, 8]}[case[0]]
    got = run_v(printer, tmp_path, c.blob, c.seeds, c.recs, c.flat)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, off, table = got[2]
    # the op record: list index | (code | field << 8) << 32
    word = ni.OP_CODES[kind] | ni.FIELD_IDS[field] << 8
    (pos,) = np.flatnonzero(((ops >> np.uint64(32)) & np.uint64(0xFF)) >= 13)
    assert int(ops[pos]) == 0 | word << 32
    # the offsets follow the shape; one table word per cell in list order; no writer bit on an input word; every output the
    # generator's to write (nothing else derives them before it: the operands are seeds)
    ins = shape[0] + shape[1]
    assert list(off) == [0, sum(shape)]
    assert [int(w) & ~W for w in table] == [c.key(cell) for grp in groups for cell in grp]
    assert not (table[:ins] & W).any() and (table[ins:] & W).all()
    assert all(cell_slot[col, row] != 0xFFFFFFFF for grp in groups for row, col in grp)
    # creation order: behind the seeds, in front of the rows; the operands are seeds' (level 0): the generator runs in level 1
    lv = wpi.op_levels(ops, level_off)
    g_level = lv[(0, ni.OP_CODES[kind], ni.FIELD_IDS[field])]
    assert g_level == 1
    codes = [int(x) for x in (ops[level_off[1]:level_off[2]] >> np.uint64(32)) & np.uint64(0xFF)]
    assert codes[0] == ni.OP_CODES[kind] and OP_SEED not in codes


def test_chain_levels(printer, circuits, tmp_path):  # noqa: F811
    """x3 = s s - x1 - x2 with s = (y2 - y1) / (x2 - x1): seven generators; every one runs one level above the writer of its
    latest input, and the six on the path v -> inv -> s -> s s -> - x1 -> - x2 lie on strictly rising levels."""
    c = circuits["chain"]
    assert [g[0] for g in c.gens] == ni.CHAIN_KINDS and all(g[2] == ni.SCALAR for g in c.gens)
    got = run_v(printer, tmp_path, c.blob, c.seeds, c.recs, c.flat)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, off, table = got[2]
    gen_ops = [int(o) for o in ops if ((int(o) >> 32) & 0xFF) >= 13]
    assert sorted(gen_ops) == sorted(i | (ni.OP_CODES[g[0]] | 1 << 8) << 32 for i, g in enumerate(c.gens))
    assert list(off) == list(np.cumsum([0] + [sum(len(grp) for grp in g[1]) for g in c.gens]))
    written, gen_level = writer_levels(c, cell_slot, ops, level_off, table, off)
    # the writers of every slot, generators' and row ops' alike
    lv = wpi.op_levels(ops, level_off)
    slot_level = dict(written)
    for (idx, code, sub), lvl in lv.items():
        if code == OP_SEED:
            row, col = c.seeds[idx]
            if col < 80 and cell_slot[col, row] & W:
                slot_level[int(cell_slot[col, row]) & ~W] = lvl
    for g, (kind, groups, _) in enumerate(c.gens):
        ins = len(groups[0]) + len(groups[1])
        assert not (table[off[g]:off[g] + ins] & W).any()
        assert (table[off[g] + ins:off[g + 1]] & W).all()            # (no output of the chain is anyone else's)
    # a generator's level is one above its latest input's writer: an input is a seed's slot (level 0) or an earlier generator's
    for g, (kind, groups, _) in enumerate(c.gens):
        levels = []
        for row, col in list(groups[0]) + list(groups[1]):
            s = int(cell_slot[col, row]) & ~W
            assert s in slot_level, (g, row, col)
            levels.append(slot_level[s])
        assert gen_level[g] == max(levels) + 1, (g, kind)
    path = [1, 2, 3, 4, 5, 6]                                            # v, inv, s, s s, - x1, - x2
    assert all(gen_level[a] < gen_level[b] for a, b in zip(path, path[1:]))
    assert gen_level[0] == gen_level[1] == 1 and gen_level[0] < gen_level[3]


def test_refusals(printer, circuits, tmp_path):  # noqa: F811
    """Every refusal of the kind word and of the shapes, with its words, before anything indexes with a cell."""
    c = circuits[("mul", ni.BASE)]
    flat = [tuple(x) for x in c.flat]

    def refused(rec, cells=None):
        cells = flat if cells is None else cells
        got = run_v(printer, tmp_path, c.blob, c.seeds, np.array([rec], dtype=np.uint32), np.array(cells, dtype=np.uint32).reshape(-1, 2))
        assert got[0] == "refused", got[:2]
        return got[1]

    def accepted(rec, cells):
        """the kind and shape checks pass (cells taken from anywhere may still leave an input unreached)"""
        got = run_v(printer, tmp_path, c.blob, c.seeds, np.array([rec], dtype=np.uint32), np.array(cells, dtype=np.uint32).reshape(-1, 2))
        return got[0] == "plan" or ("has the shape" not in got[1] and "unknown kind" not in got[1] and "cells" not in got[1])

    # the kind word: the field byte on kinds 0 and 1, an unknown field, a bit above 15, kind bytes 6 and up -- the whole word is printed
    for word in (0 | 1 << 8, 1 | 1 << 8, 2 | 2 << 8, 4 | 255 << 8, 4 | 1 << 16, 5 | 1 << 31, 6, 7, 6 | 1 << 8, 255):
        assert refused([word, 8, 8, 8, 8]) == "generator 0 has the unknown kind %d" % word
    # shapes: add / sub {la, lb, 8, 1}, mul {la, lb, 8, la + lb - 8}, inv {lx, 0, lx, lx}
    bad = {2: ([8, 8, 8, 0], [8, 8, 7, 1], [8, 8, 8, 2], [17, 8, 8, 1], [8, 17, 8, 1], [0, 0, 8, 1]),
           3: ([8, 8, 8, 0], [8, 8, 9, 1], [0, 0, 8, 1], [0, 17, 8, 1]),
           4: ([8, 8, 8, 7], [8, 8, 8, 9], [4, 3, 8, 0], [3, 4, 8, 0xFFFFFFFF], [17, 8, 8, 17], [8, 8, 7, 8], [0, 0, 8, 0]),
           5: ([8, 1, 8, 8], [8, 0, 8, 7], [8, 0, 7, 8], [0, 0, 0, 0], [17, 0, 17, 17], [8, 8, 8, 8])}
    for kind, shapes in bad.items():
        for field in (0, 1):
            for shape in shapes:
                word = kind | field << 8
                want = "generator 0 of kind %d has the shape {%d, %d, %d, %d}, which is not a shape of its kind" % (word, *shape)
                assert refused([word] + shape) == want
    # ... and the shapes at the bounds are shapes of their kinds
    cells = flat + flat
    assert accepted([2, 0, 1, 8, 1], cells[:10]) and accepted([3 | 1 << 8, 16, 16, 8, 1], cells[:41]) and accepted([2, 1, 0, 8, 1], cells[:10])
    assert accepted([4, 4, 4, 8, 0], cells[:16]) and accepted([4 | 1 << 8, 16, 16, 8, 24], cells[:64]) and accepted([4, 0, 8, 8, 0], cells[:16])
    assert accepted([5, 1, 0, 1, 1], cells[:3]) and accepted([5 | 1 << 8, 16, 0, 16, 16], cells[:48])
    # the other refusals keep their words
    assert refused([4, 8, 8, 8, 8], flat[:-1]) == "the shapes of the generators up to generator 0 name 32 cells, 31 are given"
    assert refused([4, 8, 8, 8, 8], flat + [(0, 0)]) == "the generators' shapes name 32 cells, 33 are given"
    out = list(flat)
    out[20] = (flat[20][0], 80)
    assert refused([4, 8, 8, 8, 8], out) == "generator 0 names cell (row %d, column 80) outside the %d x 80 routed cells" % (flat[20][0], 1 << c.d)
