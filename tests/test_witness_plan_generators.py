"""Generators that are no gate's own in the witness plan (csrc/planhost.hpp), without a GPU: the stand-alone
printer (csrc/tests/planhost_print.cpp, g++ only) with its third argument, the generator list, on the `is_equal` circuit and on
the reference's basic-write circuit (tests/memory_ops_inputs.py).  The rules are stated here, not recorded.  Every case runs
twice: through the plain build of the printer and through one with -fsanitize=address,undefined (a host program, run here)."""
import os
import subprocess

import numpy as np
import pytest

import memory_ops_inputs as moi
import witness_plan_inputs as wpi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "acvm-backend-plonky2_amd", "csrc")
W = 0x80000000
OP_SEED, OP_ARITHMETIC, OP_EQUALITY = 0, 2, 13


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def printer(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("planhost_" + request.param) / "planhost_print")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    r = subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(CSRC, "tests", "planhost_print.cpp")],
                       capture_output=True, timeout=600)
    if r.returncode and request.param == "sanitized" and b"san" in r.stderr:
        pytest.skip("g++ cannot link its sanitizer runtime on this machine: " + r.stderr.decode()[-200:])
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def gen_records(generators):
    """p2gpu_generator records: kind, four (row, col) pairs."""
    return np.array([[kind] + [v for cell in cells for v in cell] for kind, cells in generators], dtype=np.uint32).reshape(-1, 9)


def run_printer(exe, tmp_path, blob, cells, generators=None):
    """("plan", counts, (cell_slot, ops, level_off, table), raw output) or ("refused", text); generators: [(kind number, cells)]."""
    bp, sp, gp = str(tmp_path / "blob"), str(tmp_path / "seeds"), str(tmp_path / "gens")
    np.ascontiguousarray(blob).tofile(bp)
    np.array(list(cells), dtype=np.uint32).reshape(-1, 2).tofile(sp)
    args = [exe, bp, sp]
    if generators is not None:
        gen_records(generators).tofile(gp)
        args.append(gp)
    r = subprocess.run(args, capture_output=True, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr[-2000:]
    line, _, rest = r.stdout.partition(b"\n")
    word, _, tail = line.decode().partition(" ")
    if word == "refused":
        assert rest == b""
        return "refused", tail
    assert word == "plan"
    counts = [int(x) for x in tail.split()]
    h = np.frombuffer(bytes(np.ascontiguousarray(blob)[:256]), dtype=np.uint32)
    tot, n_ops, levels, ng = int(h[4]) << int(h[2]), counts[0], counts[1], len(generators or ())
    assert len(rest) == 4 * tot + 8 * n_ops + 4 * (levels + 1) + 16 * ng
    cell_slot = np.frombuffer(rest, dtype=np.uint32, count=tot).reshape(int(h[4]), -1)
    ops = np.frombuffer(rest, dtype=np.uint64, count=n_ops, offset=4 * tot)
    level_off = np.frombuffer(rest, dtype=np.uint32, count=levels + 1, offset=4 * tot + 8 * n_ops)
    table = np.frombuffer(rest, dtype=np.uint32, count=4 * ng, offset=4 * tot + 8 * n_ops + 4 * (levels + 1)).reshape(-1, 4)
    return "plan", counts, (cell_slot, ops, level_off, table), r.stdout


class Circuit:
    """A builder's blob, seed cells and generator list, with the cells of the targets the rules speak of."""

    def __init__(self, builder):
        self.b = builder
        self.blob = builder.blob()
        self.d = int(np.frombuffer(bytes(np.ascontiguousarray(self.blob)[:256]), dtype=np.uint32)[2])
        self.seeds = builder.seed_cells()
        self.gens = [(0, cl) for kind, cl in builder.generators() if kind == "equality"]
        self.events = [e for e in builder.events if e.kind == "equal"]
        assert len(self.gens) == len(self.events) >= 1

    def key(self, cell):
        return (cell[1] << self.d) | cell[0]

    def class_cells(self, target):
        return self.b.cells_of(target)


@pytest.fixture(scope="module")
def circuits(pkg):
    return {"is_equal": Circuit(moi.is_equal_circuit(pkg)[0]), "basic_write": Circuit(moi.translated(pkg, moi.WRITE).builder)}


@pytest.mark.parametrize("name", ["is_equal", "basic_write"])
def test_plan_with_generators_follows_the_stated_rules(printer, circuits, tmp_path, name):
    c = circuits[name]
    assert len(c.gens) == (1 if name == "is_equal" else 2)      # (a write: one is_equal per position of the padded block)
    got = run_printer(printer, tmp_path, c.blob, c.seeds, c.gens)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, table = got[2]
    lv = wpi.op_levels(ops, level_off)
    assert all(lv[(i, OP_SEED, 0)] == 0 for i in range(len(c.seeds)))
    for g, ((_, cl), ev) in enumerate(zip(c.gens, c.events)):
        # the table names the four cells; x is a seed's and y a seed's or a ConstantGate's: both written in level 0, so the
        # equality op sits in level 1 and writes `equal` and `inv`
        assert [int(w) & ~W for w in table[g]] == [c.key(cell) for cell in cl]
        assert lv[(g, OP_EQUALITY, 0)] == 1
        assert not table[g, 0] & W and not table[g, 1] & W and table[g, 2] & W and table[g, 3] & W
        # its writer bits are not in cell_slot: no cell of `equal`'s class, nor `inv`'s one cell, is a row op's output
        for row, col in c.class_cells(ev.outs[0]) + c.class_cells(ev.outs[1]):
            assert cell_slot[col, row] != 0xFFFFFFFF and not cell_slot[col, row] & W
        # every cell a generator names has a slot
        assert all(cell_slot[col, row] != 0xFFFFFFFF for row, col in cl)
        # the ArithmeticGate operation that reads `inv` (mul(diff, inv)) sits above the generator
        (row, col), = c.class_cells(ev.outs[1])
        assert col % 4 == 1 and lv[(row, OP_ARITHMETIC, col // 4)] > lv[(g, OP_EQUALITY, 0)]


def test_a_seeded_equal_is_written_by_the_seed_and_compared_by_the_generator(printer, circuits, tmp_path):
    """The reference's plonky2_is_equal_test_* assign is_equal.target as well: the seed (level 0) writes, the generator compares."""
    c = circuits["is_equal"]
    ce = c.gens[0][1][2]
    got = run_printer(printer, tmp_path, c.blob, c.seeds + [ce], c.gens)
    assert got[0] == "plan", got
    cell_slot, ops, level_off, table = got[2]
    lv = wpi.op_levels(ops, level_off)
    assert lv[(len(c.seeds), OP_SEED, 0)] == 0 and lv[(0, OP_EQUALITY, 0)] == 1
    assert cell_slot[ce[1], ce[0]] & W and not table[0, 2] & W and table[0, 3] & W


@pytest.mark.parametrize("name", ["is_equal", "basic_write"])
def test_without_the_list_a_seed_is_missing(printer, circuits, tmp_path, name):
    """Nothing derives `equal` then: its class is unreached, and the refusal names its cell of the smallest key (the first
    one `equal`'s classes have, where the circuit has several).  `inv` is one cell outside every class: without its generator
    it has no slot and is nobody's to miss."""
    c = circuits[name]
    equal_cells = [cell for ev in c.events for cell in c.class_cells(ev.outs[0])]
    got = run_printer(printer, tmp_path, c.blob, c.seeds)
    assert got[0] == "refused" and "a seed is missing" in got[1], got
    assert "(row %d, column %d)" % min(equal_cells, key=c.key) in got[1], (got[1], equal_cells)


def test_refused_generator_lists(printer, circuits, tmp_path):
    c = circuits["is_equal"]
    kind, cl = c.gens[0]
    R = c.blob[:256].view(np.uint32)[4] if hasattr(c.blob, "view") else 80
    assert R == 80
    outside = (cl[0], cl[1], (cl[2][0], 80), cl[3])           # col = num_routed_wires
    got = run_printer(printer, tmp_path, c.blob, c.seeds, [(kind, outside)])
    assert got[0] == "refused" and "generator 0 names cell (row %d, column 80)" % cl[2][0] in got[1], got
    n = 1 << c.d
    got = run_printer(printer, tmp_path, c.blob, c.seeds, [(kind, cl), (kind, ((n, 0), cl[1], cl[2], cl[3]))])
    assert got[0] == "refused" and "generator 1 names cell (row %d, column 0)" % n in got[1], got
    got = run_printer(printer, tmp_path, c.blob, c.seeds, [(7, cl)])
    assert got[0] == "refused" and "generator 0" in got[1] and "unknown kind 7" in got[1], got


def test_an_empty_list_changes_nothing(pkg, printer, circuits, tmp_path):
    """A plan without such generators is byte for byte the plan of the two-argument call."""
    import witness_gen_inputs as wgi
    cb = wgi.translated(pkg, wgi.BITWISE)
    blob, cells = cb.blob(), cb.builder.seed_cells()
    two = run_printer(printer, tmp_path, blob, cells)
    three = run_printer(printer, tmp_path, blob, cells, [])
    assert two[0] == three[0] == "plan" and two[3] == three[3]
    c = circuits["is_equal"]
    assert run_printer(printer, tmp_path, c.blob, c.seeds, []) == run_printer(printer, tmp_path, c.blob, c.seeds)
