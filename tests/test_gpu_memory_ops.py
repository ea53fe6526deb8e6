"""The memory opcodes and the equality generator on the MI355X: every circuit of tests/test_reference_memory_tests.py proved
through the C ABI to the oracle's bytes, and their witnesses generated on the device by plans that carry the generators that
are no gate's own (p2gpu_witness_plan_create_gen / _build_gen; csrc/planhost.hpp, genplan.hip, genwit.hip).  Expected matrices
come from translate.py's build() event loop, expected bytes from the oracle, never from the code under test.  Blocks of
length 1, 2, 3 and 5, one write, two reads; every circuit has at most 2^6 rows.  No test provokes a device fault: every
negative is a value the walk compares."""
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, P

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_build_inputs as dbi  # noqa: E402
import memory_ops_inputs as moi  # noqa: E402

E_UNSATISFIED = -5
W = 0x80000000
with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "acvm-backend-plonky2_amd", "csrc", "genwit.hip")) as _f:
    GROUP = int(re.search(r"constexpr uint32_t WALK_GROUP = (\d+);", _f.read()).group(1))   # witnesses per workgroup of the walk
CELL = re.compile(r"\(row (\d+), column (\d+)\)")


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


def _matrix(t):
    return t.cpu().numpy().view(np.uint64)


def _seeds(builder, wires, extra=()):
    cells = builder.seed_cells() + list(extra)
    return cells, [int(wires[c, r]) for r, c in cells]


def _is_equal_case(pkg, x, y):
    b, tx, ty, te = moi.is_equal_circuit(pkg)
    blob, wires = b.build({tx: x, ty: y})
    return b, blob, wires, []


def _program_case(pkg, prog, witness):
    cb = moi.translated(pkg, prog)
    blob, wires = cb.build(witness)
    return cb.builder, blob, wires, cb.public_inputs()


@pytest.fixture(scope="module")
def cases(pkg):
    """name -> (builder, blob, wires, public inputs): the reference's tests and the ones beyond them, built once."""
    out = {name: _program_case(pkg, prog, witness) for name, prog, witness, _ in moi.CASES}
    out["plonky2_is_equal_test_positive"] = _is_equal_case(pkg, 0, 0)
    out["plonky2_is_equal_test_negative"] = _is_equal_case(pkg, 1, 0)
    for name, (b, blob, wires, pis) in out.items():
        assert wires.shape[1] <= 1 << 6, name
    return out


NAMES = [c[0] for c in moi.CASES] + ["plonky2_is_equal_test_positive", "plonky2_is_equal_test_negative"]


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_prove_bytes_and_device_witness(pkg, orc, gpu, cases, name):
    """prove: the oracle's bytes, accepted, from a blob-made and from a p2gpu_circuit_build-made handle.  The device witness:
    for either compiler the plan's matrix is build()'s word for word, p2gpu_prove_seeds gives the bytes of prove(wires), and
    the host and the device plan are equal byte for byte in all four arrays."""
    b, blob, wires, pis = cases[name]
    oc = orc.OracleCircuit(blob)
    want, _ = oc.prove(wires, public_inputs=pis)
    assert oc.verify(want)
    oc.close()
    cd = pkg.CircuitData(blob)
    got = cd.prove(wires, public_inputs=pis).to_bytes()
    assert got == want
    cd.verify(got)
    built = pkg.CircuitData.build(**dbi.decompose(pkg, blob))
    assert built.prove(wires, public_inputs=pis).to_bytes() == want
    built.close()
    cells, values = _seeds(b, wires)
    gens = b.generators()
    assert bool(gens) == (name in ("basic_memory_write", "write_then_read_written_and_other") or name.startswith("plonky2")), name
    exported = {}
    for compile in ("host", "device"):
        plan = cd.witness_plan(cells, compile=compile, generators=gens)
        bad = np.argwhere(_matrix(plan.generate(values)) != wires)
        assert bad.size == 0, (compile, [(int(c), int(r)) for c, r in bad[:8]])
        assert plan.prove(values, public_inputs=pis).to_bytes() == want
        exported[compile] = plan.export() + (plan.export_generators(),)
        plan.close()
    for h, dv in zip(exported["host"], exported["device"]):
        assert h.dtype == dv.dtype and h.shape == dv.shape and h.tobytes() == dv.tobytes()
    table = exported["host"][3]
    assert table.shape == (len(gens), 4) and ((table[:, 2:] & W) != 0).all() and ((table[:, :2] & W) == 0).all()
    if gens:        # without the list nothing derives `equal`
        with pytest.raises(pkg.P2GpuError, match="a seed is missing"):
            cd.witness_plan(cells)
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("bound", range(9))
def test_less_or_equal_check(pkg, orc, gpu, bound):
    """test_memory_operations.rs:123-179 cut to the bounds 0 .. 8: every value <= bound proves to the oracle's bytes; every
    value above it, up to 8, is a contradiction the device walk names."""
    b, t = moi.less_or_equal_circuit(pkg, bound)
    blob = b.blob()
    cd, oc = pkg.CircuitData(blob), orc.OracleCircuit(blob)
    plan = None
    for value in range(9):
        bb, tt = moi.less_or_equal_circuit(pkg, bound)
        if value <= bound:
            _, wires = bb.build({tt: value})
            want, _ = oc.prove(wires, public_inputs=[value])
            assert cd.prove(wires, public_inputs=[value]).to_bytes() == want
            continue
        cells = bb.seed_cells()
        if plan is None:
            plan = cd.witness_plan(cells, generators=bb.generators())
        with pytest.raises(pkg.P2GpuError) as e:
            plan.generate(bb.seed_values({tt: value}))
        assert e.value.code == E_UNSATISFIED, e.value
    if plan is not None:
        plan.close()
    cd.close()
    oc.close()


EDGES = [(0, 0), (P - 1, P - 1), (0, P - 1), (P - 1, 0), (1, 0), (1 << 32, (1 << 32) - 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_edge_operands_of_the_equality_body(pkg, gpu, compile):
    """(x, y) as seeds of the `is_equal` circuit: the matrix is the host event loop's (equal = (x == y), inv = 0 or 1 / (x - y))."""
    b0 = moi.is_equal_circuit(pkg)[0]
    cd = pkg.CircuitData(b0.blob())
    plan = cd.witness_plan(b0.seed_cells(), compile=compile, generators=b0.generators())
    for x, y in EDGES:
        b, blob, wires, _ = _is_equal_case(pkg, x, y)
        cells, values = _seeds(b, wires)
        assert cells == b0.seed_cells()
        (_, (cx, cy, ce, ci)), = b.generators()
        assert int(wires[ce[1], ce[0]]) == (1 if x == y else 0)
        assert int(wires[ci[1], ci[0]]) * ((x - y) % P) % P == (0 if x == y else 1)
        bad = np.argwhere(_matrix(plan.generate(values)) != wires)
        assert bad.size == 0, ((x, y), [(int(c), int(r)) for c, r in bad[:8]])
    plan.close()
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_a_wrongly_seeded_equal_is_named(pkg, gpu, compile):
    """`equal` seeded as the reference's plonky2_is_equal_test_* do: the right value is compared and accepted, the wrong one is
    P2GPU_E_UNSATISFIED whose text names generator 0 and the cell."""
    b, blob, wires, _ = _is_equal_case(pkg, 1, 0)
    (_, gcells), = b.generators()
    ce = gcells[2]
    cells, values = _seeds(b, wires, extra=[ce])
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells, compile=compile, generators=b.generators())
    assert not plan.export_generators()[0, 2] & W and plan.export_generators()[0, 3] & W     # the seed writes, the generator compares
    assert np.array_equal(_matrix(plan.generate(values)), wires)
    with pytest.raises(pkg.P2GpuError) as e:
        plan.generate(values[:-1] + [1])
    assert e.value.code == E_UNSATISFIED and "generator 0" in str(e.value), e.value
    assert tuple(int(v) for v in CELL.search(str(e.value)).groups()) == tuple(ce), e.value
    plan.close()
    cd.close()


# x[i] = v; x[j]; assert(x[k] == e): the write circuit with its second read checked against a value the prover claims
WRITE_READ_CHECKED = dict(ops=moi.WRITE_READ["ops"] + [moi.az([(1, 8), (P - 1, 9)], 0)], public=moi.WRITE_READ["public"] + [9])


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_batch_of_the_write_circuit(pkg, gpu, compile):
    """WALK_GROUP + 1 witnesses of the write circuit (two workgroups, the second one lane wide), indices and values differing;
    member 4 has an out-of-range index, member 8 claims a wrong read value.  Status and first bad cell per member are the lone
    calls', every good matrix its lone call's and build()'s."""
    B = GROUP + 1
    assert B == 9
    prog = WRITE_READ_CHECKED
    cb0 = moi.translated(pkg, prog)
    blob = cb0.blob()
    cells = cb0.builder.seed_cells()
    assert blob[:256].view(np.uint32)[2] <= 6

    def cell_of(w):
        return cb0.builder.cells_of(cb0.witness_target_map[w])[0]

    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells, compile=compile, generators=cb0.witness_generators())
    values, want = [], []
    for m in range(B):
        block = [20 + m, 30 + 2 * m, 40 + 3 * m]
        i, v, j, k = m % 3, 99 + m, (m + 1) % 3, (2 * m) % 3
        after = block[:i] + [v] + block[i + 1:]
        witness = {0: block[0], 1: block[1], 2: block[2], 3: i, 4: v, 5: j, 7: k, 9: after[k]}
        cb = moi.translated(pkg, prog)
        blob_m, wires = cb.build(witness)
        assert np.array_equal(blob_m, blob) and cb.witness_value(6) == after[j]
        vals = [int(wires[c, r]) for r, c in cells]
        if m == 4:
            vals[cells.index(cell_of(3))] = 3                       # position 3 of a block of length 3
        if m == 8:
            vals[cells.index(cell_of(9))] = (after[k] + 1) % P      # the read gives after[k]
        values.append(vals)
        want.append(wires)
    assert len({tuple(v) for v in values}) == B
    got, status, bad = plan.generate_batch(values)
    assert [s != 0 for s in status] == [m in (4, 8) for m in range(B)], status
    for m in range(B):
        if m in (4, 8):
            with pytest.raises(pkg.P2GpuError) as e:
                plan.generate(values[m])
            assert e.value.code == E_UNSATISFIED == status[m]
            assert tuple(int(x) for x in CELL.search(str(e.value)).groups()) == bad[m], (m, e.value, bad[m])
        else:
            assert bad[m] is None
            assert np.array_equal(_matrix(got[m]), want[m]), m
            assert np.array_equal(_matrix(plan.generate(values[m])), want[m]), m
    plan.close()
    cd.close()
