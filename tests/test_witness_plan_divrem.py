"""Generators with any number of cells in the witness plan (csrc/planhost.hpp), without a GPU: the stand-alone
printer (csrc/tests/planhost_print.cpp, g++ only) with its four-argument form -- p2gpu_generator_v records and the flat cell
list -- on the reference's div_rem circuit (tests/biguint_inputs.py) and on one over virtual operands.  The rules are stated
here, not recorded.  Every case runs twice: through the plain build of the printer and through one with
-fsanitize=address,undefined (a host program, run here)."""
import subprocess

import numpy as np
import pytest

import biguint_inputs as bi
import memory_ops_inputs as moi
import witness_plan_inputs as wpi
from test_witness_plan_generators import printer, run_printer  # noqa: F401  (the fixture builds the same printer)

W = 0x80000000
OP_SEED, OP_U32_ARITHMETIC, OP_EQUALITY, OP_BIGUINT_DIVREM = 0, 8, 13, 14
KINDS = {"equality": 0, "biguint_divrem": 1}


def records(generators):
    """builder.generators() -> (p2gpu_generator_v records [kind, shape[4]], flat (row, col) list)."""
    recs, cells = [], []
    for kind, g in generators:
        groups = [[c] for c in g] if kind == "equality" else [list(grp) for grp in g]
        recs.append([KINDS.get(kind, kind)] + [len(grp) for grp in groups])
        cells += [c for grp in groups for c in grp]
    return np.array(recs, dtype=np.uint32).reshape(-1, 5), np.array(cells, dtype=np.uint32).reshape(-1, 2)


def run_v(exe, tmp_path, blob, seeds, recs, cells):
    """("plan", counts, (cell_slot, ops, level_off, off, table), raw output) or ("refused", text)"""
    bp, sp, gp, cp = (str(tmp_path / n) for n in ("blob", "seeds", "genv", "cells"))
    np.ascontiguousarray(blob).tofile(bp)
    np.array(list(seeds), dtype=np.uint32).reshape(-1, 2).tofile(sp)
    np.ascontiguousarray(recs, dtype=np.uint32).tofile(gp)
    np.ascontiguousarray(cells, dtype=np.uint32).tofile(cp)
    r = subprocess.run([exe, bp, sp, gp, cp], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr[-2000:]
    line, _, rest = r.stdout.partition(b"\n")
    word, _, tail = line.decode().partition(" ")
    if word == "refused":
        assert rest == b""
        return "refused", tail
    assert word == "plan"
    counts = [int(x) for x in tail.split()]
    h = np.frombuffer(bytes(np.ascontiguousarray(blob)[:256]), dtype=np.uint32)
    tot, n_ops, levels, ng, nc = int(h[4]) << int(h[2]), counts[0], counts[1], len(recs), len(cells)
    assert len(rest) == 4 * tot + 8 * n_ops + 4 * (levels + 1) + 4 * (ng + 1) + 4 * nc
    at = [0, 4 * tot, 4 * tot + 8 * n_ops, 4 * tot + 8 * n_ops + 4 * (levels + 1), 4 * tot + 8 * n_ops + 4 * (levels + 1) + 4 * (ng + 1)]
    cell_slot = np.frombuffer(rest, dtype=np.uint32, count=tot).reshape(int(h[4]), -1)
    ops = np.frombuffer(rest, dtype=np.uint64, count=n_ops, offset=at[1])
    level_off = np.frombuffer(rest, dtype=np.uint32, count=levels + 1, offset=at[2])
    off = np.frombuffer(rest, dtype=np.uint32, count=ng + 1, offset=at[3])
    table = np.frombuffer(rest, dtype=np.uint32, count=nc, offset=at[4])
    return "plan", counts, (cell_slot, ops, level_off, off, table), r.stdout


class Circuit:
    def __init__(self, b):
        self.b, self.blob, self.cells = b, b.blob(), b._layout().cells
        self.d = int(np.frombuffer(bytes(np.ascontiguousarray(self.blob)[:256]), dtype=np.uint32)[2])
        self.seeds = b.seed_cells()
        self.gens = b.generators()
        self.recs, self.flat = records(self.gens)

    def key(self, cell):
        return (int(cell[1]) << self.d) | int(cell[0])


@pytest.fixture(scope="module")
def circuits(pkg):
    return {"reference": Circuit(bi.div_rem_case(pkg)[0]), "virtual": Circuit(bi.div_rem_virtual(pkg, 4, 2)[0])}


@pytest.mark.parametrize("name", ["reference", "virtual"])
def test_div_rem_plan_follows_the_stated_rules(printer, circuits, tmp_path, name):  # noqa: F811
    c = circuits[name]
    (kind, groups), = c.gens
    la, lb, ld, lr = (len(g) for g in groups)
    assert kind == "biguint_divrem" and (la, lb, ld, lr) == ((4, 4, 1, 4) if name == "reference" else (4, 2, 3, 2))
    got = run_v(printer, tmp_path, c.blob, c.seeds, c.recs, c.flat)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, off, table = got[2]
    # creation order: the seeds, then the generator (op code 14, its list index in the low word), then the rows; level 0 is by
    # creation order, so is every level
    codes, idx = (ops >> np.uint64(32)) & np.uint64(0xFF), ops & np.uint64(0xFFFFFFFF)
    assert np.count_nonzero(codes == OP_BIGUINT_DIVREM) == 1 and np.count_nonzero(codes == OP_EQUALITY) == 0
    (pos,) = np.flatnonzero(codes == OP_BIGUINT_DIVREM)
    assert int(idx[pos]) == 0 and int(ops[pos] >> np.uint64(40)) == 0
    lv = wpi.op_levels(ops, level_off)
    g_level = lv[(0, OP_BIGUINT_DIVREM, 0)]
    in_level = [int(codes[k]) for k in range(level_off[g_level], level_off[g_level + 1])]
    at = in_level.index(OP_BIGUINT_DIVREM)
    assert OP_SEED not in in_level[at:] and OP_BIGUINT_DIVREM not in in_level[:at] and all(k != OP_SEED for k in in_level[at + 1:])
    assert all(code == OP_SEED for code in in_level[:at])       # (behind the seeds, in front of the rows)
    # the offsets and the table: one word per cell in list order.  The writer bit is on no input, and on the first naming of a
    # div or rem cell unless a level-0 op already writes its class: the reference's test connects div and rem to constants
    # (the ConstantGate rows lie behind the PublicInputGate row), the virtual circuit leaves them the generator's
    assert list(off) == [0, la + lb + ld + lr]
    assert [int(w) & ~W for w in table] == [c.key(cell) for grp in groups for cell in grp]
    outs = list(groups[2]) + list(groups[3])
    constant = [any(row > c.b.pi_row for row, _ in c.cells[_target_at(c, cell)]) for cell in outs]
    assert all(constant) if name == "reference" else not any(constant)
    assert not (table[:la + lb] & W).any() and [bool(w & W) for w in table[la + lb:]] == [not k for k in constant]
    assert all(cell_slot[col, row] != 0xFFFFFFFF for grp in groups for row, col in grp)
    # levels: every operand limb is a seed's or a ConstantGate's, written in level 0: the generator runs in level 1 ...
    assert g_level == 1
    # ... and below the U32ArithmeticGate operations that consume div (mul_biguint(div, b): div's limbs are multiplicand 0)
    # where it writes div; where a ConstantGate does, in level 0, they wait for that writer only
    consumers = [(row, col) for t_cell in groups[2] for row, col in c.cells[c.b.find(_target_at(c, t_cell))] if row < len(c.b.rows) and c.b.rows[row]["kind"] == "u32arith" and col % 6 == 0]
    assert consumers
    for row, col in consumers:
        assert col % 6 == 0 and lv[(row, OP_U32_ARITHMETIC, col // 6)] > (0 if name == "reference" else g_level)


def _target_at(c, cell):
    """a target whose class holds `cell`"""
    for root, cl in c.cells.items():
        if tuple(cell) in [tuple(x) for x in cl]:
            return root
    raise AssertionError(cell)


def test_a_seeded_rem_limb_is_written_by_the_seed_and_compared_by_the_generator(printer, circuits, tmp_path):  # noqa: F811
    c = circuits["virtual"]
    groups = c.gens[0][1]
    rem0 = groups[3][0]
    got = run_v(printer, tmp_path, c.blob, c.seeds + [rem0], c.recs, c.flat)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, off, table = got[2]
    k = sum(len(g) for g in groups[:3])
    assert cell_slot[rem0[1], rem0[0]] & W and not table[k] & W and (table[k + 1:] & W).all() and (table[4 + 2:k] & W).all()


def test_a_slot_named_twice(printer, circuits, tmp_path):  # noqa: F811
    """The same cell as two input positions is one dependency (the op still runs one level above it); the same cell as two
    output positions: the first naming may write, the second compares."""
    c = circuits["virtual"]
    x = c.gens[0][1][0][0]                       # a's first limb: a seed's cell
    y = ((1 << c.d) - 1, 79)                     # a routed cell of the last row that no class and no row op holds
    assert c.b._layout().cells and all(tuple(y) != tuple(cell) for cl in c.cells.values() for cell in cl)
    recs = np.concatenate([c.recs, np.array([[1, 1, 1, 1, 1]], dtype=np.uint32)])
    flat = np.concatenate([c.flat, np.array([x, x, y, y], dtype=np.uint32)])
    got = run_v(printer, tmp_path, c.blob, c.seeds, recs, flat)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, off, table = got[2]
    lv = wpi.op_levels(ops, level_off)
    assert lv[(1, OP_BIGUINT_DIVREM, 0)] == 1 and list(off) == [0, 11, 15]
    assert not table[-4] & W and not table[-3] & W and table[-2] & W and not table[-1] & W and int(table[-2]) & ~W == int(table[-1]) == c.key(y)
    assert cell_slot[y[1], y[0]] != 0xFFFFFFFF and not cell_slot[y[1], y[0]] & W


def test_refusals(printer, circuits, tmp_path):  # noqa: F811
    """Every refusal of the list, with its words, before anything indexes with a cell."""
    c = circuits["virtual"]
    n, R = 1 << c.d, 80

    def refused(recs, flat):
        got = run_v(printer, tmp_path, c.blob, c.seeds, np.array(recs, dtype=np.uint32).reshape(-1, 5), np.array(flat, dtype=np.uint32).reshape(-1, 2))
        assert got[0] == "refused", got[:2]
        return got[1]

    flat = [tuple(x) for x in c.flat]
    assert refused([[7, 4, 2, 3, 2]], flat) == "generator 0 has the unknown kind 7"
    for shape in ([1, 1, 1, 2], [2, 1, 1, 1]):
        assert refused([[0] + shape], flat) == "generator 0 of kind 0 has the shape {%d, %d, %d, %d}, which is not a shape of its kind" % tuple(shape)
    for shape in ([4, 2, 3, 3], [4, 2, 2, 2], [4, 2, 4, 2], [0, 2, 0, 2], [33, 2, 32, 2], [17, 17, 1, 17], [4, 0, 5, 0], [1, 3, 1, 3], [2, 3, 1, 3]):
        assert "generator 0 of kind 1 has the shape {%d, %d, %d, %d}" % tuple(shape) in refused([[1] + shape], flat)
    assert refused([[1, 4, 2, 3, 2]], flat[:-1]) == "the shapes of the generators up to generator 0 name 11 cells, 10 are given"
    assert refused([[1, 4, 2, 3, 2]], flat + [(0, 0)]) == "the generators' shapes name 11 cells, 12 are given"
    assert refused([[1, 4, 2, 3, 2], [0, 1, 1, 1, 1]], flat + [(0, 0)] * 3) == "the shapes of the generators up to generator 1 name 15 cells, 14 are given"
    # the record form of four cells knows the equality generator only, as before: kind 1 is an unknown kind there
    four = [tuple(x) for x in flat[:4]]
    assert run_printer(printer, tmp_path, c.blob, c.seeds, [(1, four)])[:2] == ("refused", "generator 0 has the unknown kind 1")
    assert run_printer(printer, tmp_path, c.blob, c.seeds, [(0, four[:3] + [(flat[0][0], R)]), (1, four)])[1].startswith("generator 0 names cell")
    bad = list(flat)
    bad[9] = (flat[9][0], R)
    assert refused([[1, 4, 2, 3, 2]], bad) == "generator 0 names cell (row %d, column %d) outside the %d x %d routed cells" % (flat[9][0], R, n, R)
    bad = flat + [(0, 0), (0, 1), (n, 2), (0, 3)]
    assert refused([[1, 4, 2, 3, 2], [0, 1, 1, 1, 1]], bad) == "generator 1 names cell (row %d, column 2) outside the %d x %d routed cells" % (n, n, R)
    # lb > la + 1: div has no limbs -- a shape of the kind
    assert "has the shape" not in str(run_v(printer, tmp_path, c.blob, c.seeds, np.array([[1, 1, 3, 0, 3]], dtype=np.uint32), np.array(flat[:7], dtype=np.uint32))[:2])


def test_an_equality_only_list_gives_the_bytes_of_the_record_form(pkg, printer, tmp_path):  # noqa: F811
    """{1, 1, 1, 1} shapes through the new list: cell_slot, ops, level_off and the table are the three-argument form's bytes,
    with the offsets 0, 4, 8, .. in between."""
    b = moi.translated(pkg, moi.WRITE).builder
    blob, seeds, gens = b.blob(), b.seed_cells(), b.generators()
    assert [k for k, _ in gens] == ["equality"] * 2
    old = run_printer(printer, tmp_path, blob, seeds, [(0, cl) for _, cl in gens])
    new = run_v(printer, tmp_path, blob, seeds, *records(gens))
    assert old[0] == new[0] == "plan" and old[1] == new[1]
    for x, y in zip(old[2][:3], new[2][:3]):
        assert x.tobytes() == y.tobytes()
    assert list(new[2][3]) == [0, 4, 8] and old[2][3].tobytes() == new[2][4].tobytes()
    head = len(old[3]) - 16 * len(gens)
    assert new[3] == old[3][:head] + new[2][3].tobytes() + old[3][head:]
