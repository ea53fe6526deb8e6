"""The host plan compiler (csrc/planhost.hpp: no HIP in it) without a GPU: a stand-alone printer, compiled with g++, runs it on
circuit blobs made on the CPU.  Its arrays and counts equal, byte for byte, the plans recorded from p2gpu_witness_plan_create
on the MI355X before the compiler moved (tests/golden/witness_plans.npz; profiles/witness_refactor.md has the recipe); the
rules the hand-built circuits were made for are stated outright; the refusals carry the library's words.
The compiler under test needs g++ alone.  The INPUTS come through the `pkg` fixture: the circuit blobs are made by the
package's own `build_blob` and translator, as tests/test_gpu_witness_plan.py makes them, which loads the built library (no
device call is made)."""
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden")
sys.path.insert(0, GOLDEN)
sys.path.insert(0, HERE)
import witness_gen_inputs as wgi  # noqa: E402
import witness_plan_inputs as wpi  # noqa: E402
import witness_plan_recorded as wpr  # noqa: E402

CSRC = os.path.join(os.path.dirname(HERE), "acvm-backend-plonky2_amd", "csrc")
NAMES = sorted(wpi.HAND_BUILT) + ["fibonacci", "quadratic", "bitwise", "custom_gate_chain", "basic_if", "basic_div", "sha256_compression"]


@pytest.fixture(scope="module")
def printer(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("planhost") / "planhost_print")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(CSRC, "tests", "planhost_print.cpp")], check=True,
                   timeout=300)
    return exe


@pytest.fixture(scope="module")
def cases(pkg):
    return wpr.cases(pkg)


@pytest.fixture(scope="module")
def recorded():
    return wpr.load(GOLDEN)


def run_printer(exe, tmp_path, blob, cells):
    """("plan", counts, (cell_slot, ops, level_off)) or ("refused", text)."""
    bp, sp = str(tmp_path / "blob"), str(tmp_path / "seeds")
    np.ascontiguousarray(blob).tofile(bp)
    np.array(list(cells), dtype=np.uint32).reshape(-1, 2).tofile(sp)
    r = subprocess.run([exe, bp, sp], capture_output=True, timeout=300)
    assert r.returncode == 0, r.stderr[-500:]
    line, _, rest = r.stdout.partition(b"\n")
    word, _, tail = line.decode().partition(" ")
    if word == "refused":
        assert rest == b""
        return "refused", tail
    assert word == "plan"
    counts = [int(x) for x in tail.split()]
    h = np.frombuffer(bytes(np.ascontiguousarray(blob)[:256]), dtype=np.uint32)
    tot, n_ops, levels = int(h[4]) << int(h[2]), counts[0], counts[1]
    assert len(rest) == 4 * tot + 8 * n_ops + 4 * (levels + 1)
    cell_slot = np.frombuffer(rest, dtype=np.uint32, count=tot).reshape(int(h[4]), -1)
    ops = np.frombuffer(rest, dtype=np.uint64, count=n_ops, offset=4 * tot)
    level_off = np.frombuffer(rest, dtype=np.uint32, count=levels + 1, offset=4 * tot + 8 * n_ops)
    return "plan", counts, (cell_slot, ops, level_off)


def test_every_recorded_input_is_run(cases, recorded):
    assert list(cases) == NAMES and sorted(recorded) == sorted(NAMES)
    for name, rec in recorded.items():
        assert ("cell_slot_sha256" in rec) == (name in wpr.DIGEST_ONLY) and ("cell_slot" in rec) != (name in wpr.DIGEST_ONLY)


@pytest.mark.parametrize("name", NAMES)
def test_plan_is_the_recorded_one(printer, cases, recorded, tmp_path, name):
    blob, cells = cases[name]
    got = run_printer(printer, tmp_path, blob, cells)
    assert got[0] == "plan", got
    wpr.compare(name, recorded[name], got[1], got[2])


def test_stated_levels(printer, cases, tmp_path):
    """The rules the hand-built circuits reach, stated here and not taken from a recording."""
    blob, cells = cases["waiting_op_claims_nothing"]
    _, _, (cell_slot, ops, level_off) = run_printer(printer, tmp_path, blob, cells)
    lv = wpi.op_levels(ops, level_off)
    # i takes level 1, j waits for level 2 and claims nothing, so k takes level 1
    assert lv[(0, wpi.OP_ARITHMETIC, 0)] == 1 and lv[(1, wpi.OP_U32_ARITHMETIC, 0)] == 2 and lv[(2, wpi.OP_ARITHMETIC, 0)] == 1, lv
    assert all(lv[(i, wpi.OP_SEED, 0)] == 0 for i in range(len(cells)))
    # the writers: i its output, k its output; j neither of the two words it shares, but its own inverse and limbs
    W = 0x80000000
    assert cell_slot[3, 0] & W and cell_slot[3, 2] & W and not cell_slot[3, 1] & W and not cell_slot[4, 1] & W and cell_slot[5, 1] & W
    blob, cells = cases["base_sum_twins"]
    lv = wpi.op_levels(*run_printer(printer, tmp_path, blob, cells)[2][1:])
    assert lv[(0, wpi.OP_BASE_SPLIT, 0)] == 1 and (0, wpi.OP_BASE_JOIN, 0) not in lv
    assert lv[(1, wpi.OP_BASE_JOIN, 0)] == 1 and (1, wpi.OP_BASE_SPLIT, 0) not in lv
    blob, cells = cases["same_level_contenders"]
    lv = wpi.op_levels(*run_printer(printer, tmp_path, blob, cells)[2][1:])
    assert [lv[(r, wpi.OP_ARITHMETIC, 0)] for r in range(3)] == [1, 2, 2]


def test_refusals(pkg, printer, tmp_path):
    """The words tests/test_gpu_witness_plan.py::test_errors asserts of the library, through the printer."""
    def refused(blob, cells, *words):
        got = run_printer(printer, tmp_path, blob, cells)
        assert got[0] == "refused", got[:2]
        for w in words:
            assert w in got[1], got[1]
        return got[1]

    prog = wgi.BITWISE
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cells = cb.builder.seed_cells()
    n = wires.shape[1]
    refused(blob, cells + [(n, 0)], f"row {n}, column 0")
    refused(blob, cells + [cells[1]], "row %d, column %d" % cells[1], "twice")
    msg = refused(blob, cells[:2] + cells[3:], "seed is missing")
    stuck_cells = cb.builder.cells_of(cb.witness_target_map[2])
    assert any("(row %d, column %d)" % rc in msg for rc in stuck_cells), (msg, stuck_cells)
    kw, seeds = wgi.arithmetic_cycle()
    refused(pkg.build_blob(**kw), seeds, "dependency cycle", "row 0")
    # two tampered cells, the smaller key (column 1) is the one reported
    bad = wpi.tamper_sigma(wpi.tamper_sigma(blob, 1, 3, 11), 2, 1, 5)
    refused(bad, cells, "sigma of cell (row 2, column 1) names no routed cell")
