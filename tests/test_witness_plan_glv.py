"""The GLV decomposition generator in the witness plan (csrc/planhost.hpp), without a GPU: the stand-alone printer
(csrc/tests/planhost_print.cpp, g++ only) in its four-argument form on the decomposition circuit of tests/curve_inputs.py.  The
rules are stated here, not recorded.  Every case runs twice: through the plain build of the printer and through one with
-fsanitize=address,undefined (a host program, run here)."""
import numpy as np
import pytest

import curve_inputs as ci
import witness_plan_inputs as wpi
from test_witness_plan_divrem import run_v
from test_witness_plan_generators import printer  # noqa: F401  (the fixture builds the same printer)

W = 0x80000000


class Circuit:
    def __init__(self, b):
        self.b, self.blob = b, b.blob()
        self.d = int(np.frombuffer(bytes(np.ascontiguousarray(self.blob)[:256]), dtype=np.uint32)[2])
        self.seeds, self.gens = b.seed_cells(), b.generators()
        recs, flat = ci.records(self.gens)
        self.recs, self.flat = np.array(recs, dtype=np.uint32).reshape(-1, 5), flat

    def key(self, cell):
        return (int(cell[1]) << self.d) | int(cell[0])


@pytest.fixture(scope="module")
def circuit(pkg):
    c = Circuit(ci.decomposition(pkg)[0])
    assert 1 << c.d <= 1 << 9
    return c


def run(printer, tmp_path, c, recs, flat):  # noqa: F811
    return run_v(printer, tmp_path, c.blob, c.seeds, np.array(recs, dtype=np.uint32).reshape(-1, 5), np.array(flat, dtype=np.uint32).reshape(-1, 2))


def test_decomposition_circuit_compiles(printer, circuit, tmp_path):  # noqa: F811
    """The generators of `decompose_secp256k1_scalar`, in creation order; the GLV one's record is list index 0 | 19 << 32 with no
    field; its table words are its cells in list order, the eight k limbs without a writer bit, the ten targets with one; it
    runs in level 1, above the seeds, and the nonnative generators that read k1, k2 and the signs run above it."""
    c = circuit
    assert [g[0] for g in c.gens] == ["glv_decompose", "nonnative_sub", "nonnative_add", "nonnative_sub", "nonnative_add", "nonnative_mul", "nonnative_add"]
    kind, groups = c.gens[0]
    assert [len(g) for g in groups] == [8, 0, 8, 2] and list(c.recs[0]) == [ci.KIND, 8, 0, 8, 2]
    got = run(printer, tmp_path, c, c.recs, c.flat)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, off, table = got[2]
    records = [int(o) for o in ops if ((int(o) >> 32) & 0xFF) == ci.OP_CODE]
    assert records == [0 | ci.OP_CODE << 32]
    assert list(off) == list(np.cumsum([0] + [sum(r[1:]) for r in c.recs]))
    assert [int(w) & ~W for w in table[:18]] == [c.key(cell) for grp in groups for cell in grp]
    assert not (table[:8] & W).any() and (table[8:18] & W).all()
    lv = wpi.op_levels(ops, level_off)
    levels = {idx: l for (idx, code, _), l in lv.items() if code >= 13}
    assert levels[0] == 1 and all(levels[g] > 1 for g in range(1, len(c.gens)))


def test_refusals(printer, circuit, tmp_path):  # noqa: F811
    """The kind word takes no field: any bit above bit 7 and the numbers 6, 7 and 9 are unknown kinds, the whole word printed;
    the shape is {lk, 0, 8, 2} with 1 <= lk <= 16; the cell checks keep their words."""
    c = circuit
    flat = c.flat[:18]

    def refused(rec, cells=flat):
        got = run(printer, tmp_path, c, [rec], cells)
        assert got[0] == "refused", got[:2]
        return got[1]

    for word in (8 | 1 << 8, 8 | 1 << 16, 9, 6, 7, 6 | 1 << 8, 8 | 1 << 31, 255):
        assert refused([word, 8, 0, 8, 2]) == "generator 0 has the unknown kind %d" % word
    for shape in ([0, 0, 8, 2], [17, 0, 8, 2], [8, 1, 8, 2], [8, 0, 7, 2], [8, 0, 8, 1], [8, 0, 8, 3], [8, 0, 9, 2]):
        assert refused([ci.KIND] + shape) == "generator 0 of kind 8 has the shape {%d, %d, %d, %d}, which is not a shape of its kind" % tuple(shape)
    out = list(flat)
    out[9] = (flat[9][0], 80)
    assert refused([ci.KIND, 8, 0, 8, 2], out) == "generator 0 names cell (row %d, column 80) outside the %d x 80 routed cells" % (flat[9][0], 1 << c.d)
    out[9] = (1 << c.d, 0)
    assert refused([ci.KIND, 8, 0, 8, 2], out) == "generator 0 names cell (row %d, column 0) outside the %d x 80 routed cells" % (1 << c.d, 1 << c.d)
    assert refused([ci.KIND, 8, 0, 8, 2], flat[:-1]) == "the shapes of the generators up to generator 0 name 18 cells, 17 are given"
    assert refused([ci.KIND, 8, 0, 8, 2], flat + [(0, 0)]) == "the generators' shapes name 18 cells, 19 are given"


@pytest.mark.parametrize("lk", [1, 16])
def test_the_generator_alone_compiles_at_either_bound(pkg, printer, tmp_path, lk):  # noqa: F811
    """lk = 1 and lk = 16 over limbs nothing range-checks: build() gives the model's values for a sixteen-limb scalar of N or
    above and for limbs of 2^32 and above, and the plan runs the generator in level 1 and writes all ten targets."""
    limbs = ([ci.GOLDILOCKS - 1] * 16 if lk == 16 else [7])
    c = ci.generator_only(pkg, lk)
    cc = Circuit(c[0])
    _, wires = c[0].build(ci.scalar_witness(c, limbs))
    (_, groups), = cc.gens
    k1, k2, n1, n2 = ci.decompose(ci.fold(limbs) % ci.N)
    assert [int(wires[col, row]) for row, col in groups[2] + groups[3]] == ci.digits(k1, 4) + ci.digits(k2, 4) + [int(n1), int(n2)]
    got = run(printer, tmp_path, cc, cc.recs, cc.flat)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, off, table = got[2]
    assert list(off) == [0, lk + 10] and not (table[:lk] & W).any() and (table[lk:] & W).all()
    assert {l for (idx, code, _), l in wpi.op_levels(ops, level_off).items() if code == ci.OP_CODE} == {1}


def test_shapes_at_the_bounds_are_accepted(printer, circuit, tmp_path):  # noqa: F811
    """lk = 1 and lk = 16 pass the kind and shape checks (cells taken from anywhere may still leave an input unreached)"""
    c = circuit
    cells = (c.flat + c.flat)[:26]
    for lk in (1, 16):
        got = run(printer, tmp_path, c, [[ci.KIND, lk, 0, 8, 2]], cells[:lk + 10])
        assert got[0] == "plan" or ("has the shape" not in got[1] and "unknown kind" not in got[1] and "cells" not in got[1]), got[:2]
