"""The nonnative gadgets and their four generators on the MI355X: the circuits of tests/test_reference_nonnative_tests.py and the
chain of tests/nonnative_inputs.py proved through the C ABI to the oracle's bytes, and their witnesses generated on the device by
plans that carry the generators (p2gpu_witness_plan_create_genv / _build_genv; csrc/planhost.hpp, genplan.hip, genwit.hip,
nonnative.hpp).  Expected matrices come from translate.py's build() event loop, expected bytes from the oracle, expected sums,
products and inverses from Python integers, never from the code under test.  Every single-operation circuit has at most 2^7
rows, the chain at most 2^9.  No test provokes a device fault: every negative is a value the walk compares or rejects."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_build_inputs as dbi  # noqa: E402
import nonnative_inputs as ni  # noqa: E402

E_UNSATISFIED, E_ARG = -5, -7
W = 0x80000000
with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "acvm-backend-plonky2_amd", "csrc", "genwit.hip")) as _f:
    GROUP = int(re.search(r"constexpr uint32_t WALK_GROUP = (\d+);", _f.read()).group(1))   # witnesses per workgroup of the walk
CELL = re.compile(r"\(row (\d+), column (\d+)\)")
CHAIN_POINTS = (ni.X256, ni.Y256, ni.Z256, ni.V256)


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


NAMES = ["%s_%s" % (name, f) for f in ni.FIELDS for name, _ in ni.REFERENCE_CASES] + ["chain"]


@pytest.fixture(scope="module")
def cases(pkg):
    """name -> (builder, blob, wires): the reference's five tests over both fields and the chain, built once."""
    out = {}
    for f in ni.FIELDS:
        for name, make in ni.REFERENCE_CASES:
            b, w = make(pkg, f)
            blob, wires = b.build(w)
            assert wires.shape[1] <= 1 << 7, name
            out["%s_%s" % (name, f)] = (b, blob, wires)
    c = ni.chain(pkg, ni.BASE)
    blob, wires = c[0].build(ni.chain_operands(c, *CHAIN_POINTS))
    assert wires.shape[1] <= 1 << 9
    assert [c[0].value_of(t) for t in c[2]] == ni.digits(ni.chain_x3(ni.BASE, *CHAIN_POINTS), ni.L)
    out["chain"] = (c[0], blob, wires)
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("name", NAMES)
def test_prove_bytes_and_device_witness(pkg, orc, gpu, cases, name):
    """prove: the oracle's bytes, accepted, from a blob-made and from a p2gpu_circuit_build-made handle.  The device witness:
    for either compiler the plan's matrix is build()'s word for word, p2gpu_prove_seeds gives the bytes of prove(wires), and
    the host and the device plan are equal byte for byte in cell_slot, ops, level_off, the offsets and the table."""
    b, blob, wires = cases[name]
    oc = orc.OracleCircuit(blob)
    want, _ = oc.prove(wires, public_inputs=[])
    assert oc.verify(want)
    oc.close()
    cd = pkg.CircuitData(blob)
    got = cd.prove(wires).to_bytes()
    assert got == want
    cd.verify(got)
    built = pkg.CircuitData.build(**dbi.decompose(pkg, blob))
    assert built.prove(wires).to_bytes() == want
    built.close()
    cells, values = _seeds(b, wires)
    gens = b.generators()
    assert [g[0] for g in gens] == (ni.CHAIN_KINDS if name == "chain" else [{"add": "nonnative_add", "sub": "nonnative_sub", "neg": "nonnative_sub",
                                                                             "mul": "nonnative_mul", "inv": "nonnative_inv"}[name.split("_")[0]]])
    exported = {}
    for compile in ("host", "device"):
        plan = cd.witness_plan(cells, compile=compile, generators=gens)
        bad = np.argwhere(_matrix(plan.generate(values)) != wires)
        assert bad.size == 0, (compile, [(int(c), int(r)) for c, r in bad[:8]])
        assert plan.prove(values).to_bytes() == want
        exported[compile] = plan.export() + plan.export_generators_v()
        plan.close()
    for h, dv in zip(exported["host"], exported["device"]):
        assert h.dtype == dv.dtype and h.shape == dv.shape and h.tobytes() == dv.tobytes()
    cell_slot, ops, level_off, off, table = exported["host"]
    records = sorted(int(o) for o in ops if ((int(o) >> 32) & 0xFF) >= 13)
    assert records == sorted(i | (ni.OP_CODES[g[0]] | ni.FIELD_IDS[g[2]] << 8) << 32 for i, g in enumerate(gens))
    assert list(off) == list(np.cumsum([0] + [sum(len(grp) for grp in g[1]) for g in gens]))
    for i, g in enumerate(gens):
        ins = len(g[1][0]) + len(g[1][1])
        assert not (table[off[i]:off[i] + ins] & W).any()
        if name == "chain":                                   # (the reference's tests connect the result to ConstantGate cells)
            assert (table[off[i] + ins:off[i + 1]] & W).all()
    cd.close()


def _shapes():
    by_shape = {}
    for name, kind, la, lb, fa, fb in ni.EDGES:
        by_shape.setdefault((kind, la, lb), []).append((name, fa, fb))
    return by_shape


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_edge_operands_on_the_device(pkg, gpu, compile):
    """One plan per (kind, field, shape), the operands as seeds: every matrix is build()'s, and the two targets read from the
    device's matrix at the generator's cells are Python's values -- A + B = M gives sum = M and overflow 0."""
    seen = set()
    for (kind, la, lb), members in _shapes().items():
        for field in ni.FIELDS:
            c0 = ni.virtual(pkg, kind, field, la, lb)
            blob = c0[0].blob()
            (_, groups, _), = c0[0].generators()
            cd = pkg.CircuitData(blob)
            assert cd.degree <= 1 << 7
            plan = cd.witness_plan(c0[0].seed_cells(), compile=compile, generators=c0[0].generators())
            for name, fa, fb in members:
                c = ni.virtual(pkg, kind, field, la, lb)
                _, wires = c[0].build(ni.operands(c, fa(field), fb(field)))
                cells, values = _seeds(c[0], wires)
                got = _matrix(plan.generate(values))
                bad = np.argwhere(got != wires)
                assert bad.size == 0, (name, field, [(int(x), int(y)) for x, y in bad[:8]])
                first, second = ni.expected(kind, field, fa(field), fb(field))
                assert [int(got[col, row]) for row, col in groups[2]] == ni.digits(first, len(groups[2])), (name, field)
                assert [int(got[col, row]) for row, col in groups[3]] == ni.digits(second, len(groups[3])), (name, field)
                if name == "add_equals_m":
                    assert first == ni.ORDER[field] and second == 0
                seen.add(name)
            plan.close()
            cd.close()
    assert seen == {e[0] for e in ni.EDGES}


def _refused(pkg, plan, values, generator):
    with pytest.raises(pkg.P2GpuError) as e:
        plan.generate(values)
    assert e.value.code == E_UNSATISFIED and ("generator %d" % generator) in str(e.value), e.value
    return tuple(int(v) for v in CELL.search(str(e.value)).groups())


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_contradictions_are_named(pkg, gpu, compile):
    """X = 0: P2GPU_E_UNSATISFIED naming the generator and x's first cell -- in the chain that is x1 = x2.  An inverse of eight
    digits for a target of four limbs: inv's top limb.  An extra seed on a prod limb: the right value is compared and accepted, a
    wrong one is named at that cell, and the table shows that the seed holds the writer bit."""
    c = ni.virtual(pkg, "inv", ni.SCALAR)
    (_, (cx, _, cinv, cdiv), _), = c[0].generators()
    cd = pkg.CircuitData(c[0].blob())
    plan = cd.witness_plan(c[0].seed_cells(), compile=compile, generators=c[0].generators())
    assert _refused(pkg, plan, c[0].seed_values(ni.operands(c, 0)), 0) == tuple(cx[0])
    c2 = ni.virtual(pkg, "inv", ni.SCALAR)
    assert _refused(pkg, plan, c2[0].seed_values(ni.operands(c2, ni.ORDER[ni.SCALAR])), 0) == tuple(cx[0])      # (M reduces to zero)
    plan.close()
    cd.close()

    c = ni.chain(pkg, ni.BASE)
    gens = c[0].generators()
    cd = pkg.CircuitData(c[0].blob())
    plan = cd.witness_plan(c[0].seed_cells(), compile=compile, generators=gens)
    assert gens[2][0] == "nonnative_inv"
    assert _refused(pkg, plan, c[0].seed_values(ni.chain_operands(c, ni.X256, ni.Y256, ni.X256, ni.V256)), 2) == tuple(gens[2][1][0][0])
    plan.close()
    cd.close()

    c = ni.virtual(pkg, "inv", ni.BASE, la=4)
    (_, (cx, _, cinv, cdiv), _), = c[0].generators()
    assert len(cinv) == 4 and pow(3, -1, ni.ORDER[ni.BASE]) >> 128
    cd = pkg.CircuitData(c[0].blob())
    plan = cd.witness_plan(c[0].seed_cells(), compile=compile, generators=c[0].generators())
    assert _refused(pkg, plan, c[0].seed_values(ni.operands(c, 3)), 0) == tuple(cinv[-1])
    plan.close()
    cd.close()

    c = ni.virtual(pkg, "mul", ni.BASE)
    gens = c[0].generators()
    (_, (ca, cb, cprod, cover), _), = gens
    cd = pkg.CircuitData(c[0].blob())
    c2 = ni.virtual(pkg, "mul", ni.BASE)
    _, wires = c2[0].build(ni.operands(c2, ni.X256, ni.Y256))
    cells, values = _seeds(c2[0], wires, extra=[cprod[1]])
    assert values[-1] == (ni.X256 * ni.Y256 % ni.ORDER[ni.BASE]) >> 32 & ni.M
    plan = cd.witness_plan(cells, compile=compile, generators=gens)
    off, table = plan.export_generators_v()
    k = 8 + 8 + 1
    assert not table[k] & W and table[k - 1] & W and table[k + 1] & W          # the seed writes, the generator compares
    assert np.array_equal(_matrix(plan.generate(values)), wires)
    assert _refused(pkg, plan, values[:-1] + [(values[-1] + 1) & ni.M], 0) == tuple(cprod[1])
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_an_operand_of_the_order_or_above_is_unsatisfiable(pkg, gpu):
    """The virtual add circuit with a = M + 5: the generator reduces, the constraint does not.  P2GPU_E_UNSATISFIED, and both
    compilers, the lone and the batched call name the same cell (which one is the schedule's business)."""
    named = []
    for compile in ("host", "device"):
        c = ni.virtual(pkg, "add", ni.BASE)
        cd = pkg.CircuitData(c[0].blob())
        plan = cd.witness_plan(c[0].seed_cells(), compile=compile, generators=c[0].generators())
        values = c[0].seed_values(ni.operands(c, ni.ORDER[ni.BASE] + 5, ni.Y256))
        with pytest.raises(pkg.P2GpuError) as e:
            plan.generate(values)
        assert e.value.code == E_UNSATISFIED, e.value
        named.append(tuple(int(v) for v in CELL.search(str(e.value)).groups()))
        c2 = ni.virtual(pkg, "add", ni.BASE)
        _, wires = c2[0].build(ni.operands(c2, ni.X256, ni.Y256))
        good = [int(wires[col, row]) for row, col in c2[0].seed_cells()]
        got, status, bad = plan.generate_batch([good, values])
        assert status == [0, E_UNSATISFIED] and bad[0] is None and np.array_equal(_matrix(got[0]), wires)
        named.append(bad[1])
        plan.close()
        cd.close()
    assert len(set(named)) == 1, named


@pytest.mark.gpu
def test_refused_lists_from_both_compilers(pkg, gpu):
    """Every refusal of a list with the new kinds comes back as P2GPU_E_ARG with the same words from
    p2gpu_witness_plan_create_genv and from p2gpu_witness_plan_build_genv."""
    c = ni.virtual(pkg, "mul", ni.BASE)
    b = c[0]
    (_, groups, _), = b.generators()
    cd = pkg.CircuitData(b.blob())
    n, R = cd.degree, cd.num_routed_wires
    outside = (groups[0], groups[1], groups[2][:2] + ((groups[2][2][0], R),) + groups[2][3:], groups[3])
    lists = [
        ([(7, groups)], "generator 0 has the unknown kind 7"),
        ([(6, groups, 0)], "generator 0 has the unknown kind 6"),
        ([("nonnative_mul", groups, 2)], "generator 0 has the unknown kind %d" % (4 | 2 << 8)),
        ([("equality", groups, 1)], "generator 0 has the unknown kind 256"),
        ([("biguint_divrem", groups, "secp256k1_scalar")], "generator 0 has the unknown kind 257"),
        ([(4 | 1 << 16, groups)], "generator 0 has the unknown kind 65540"),
        ([("nonnative_mul", (groups[0], groups[1], groups[2], groups[3][:7]), "secp256k1_base")],
         "generator 0 of kind 4 has the shape {8, 8, 8, 7}, which is not a shape of its kind"),
        ([("nonnative_mul", (groups[0][:3], groups[1][:4], groups[2], ()), "secp256k1_scalar")],
         "generator 0 of kind 260 has the shape {3, 4, 8, 0}, which is not a shape of its kind"),
        ([("nonnative_add", (groups[0], groups[1], groups[2], groups[3][:2]), "secp256k1_base")],
         "generator 0 of kind 2 has the shape {8, 8, 8, 2}, which is not a shape of its kind"),
        ([("nonnative_sub", ((), (), groups[2], groups[3][:1]), "secp256k1_base")],
         "generator 0 of kind 3 has the shape {0, 0, 8, 1}, which is not a shape of its kind"),
        ([("nonnative_inv", (groups[0], groups[1][:1], groups[2], groups[3]), "secp256k1_base")],
         "generator 0 of kind 5 has the shape {8, 1, 8, 8}, which is not a shape of its kind"),
        ([("nonnative_mul", outside, "secp256k1_base")], "generator 0 names cell (row %d, column %d) outside the %d x %d routed cells" % (groups[2][2][0], R, n, R)),
    ]
    for compile in ("host", "device"):
        for gens, words in lists:
            with pytest.raises(pkg.P2GpuError) as e:
                cd.witness_plan(b.seed_cells(), compile=compile, generators=gens)
            assert e.value.code == E_ARG and words in str(e.value), (compile, e.value)
    seeds = np.array(b.seed_cells(), dtype=np.uint32)
    recs = np.array([[4, 8, 8, 8, 8]], dtype=np.uint32)
    flat = np.array([cell for g in groups for cell in g], dtype=np.uint32)
    lib = cd._lib
    lib.p2gpu_last_error.restype = ctypes.c_char_p
    for make in (lib.p2gpu_witness_plan_create_genv, lib.p2gpu_witness_plan_build_genv):
        h = ctypes.c_void_p()
        assert make(cd._h, seeds.ctypes.data, len(seeds), recs.ctypes.data, 1, flat.ctypes.data, 31, ctypes.byref(h)) == E_ARG and not h.value
        assert lib.p2gpu_last_error().decode() == "the shapes of the generators up to generator 0 name 32 cells, 31 are given"
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_batch_of_the_chain(pkg, gpu, compile):
    """WALK_GROUP + 1 witnesses of the chain (two workgroups, the second one lane wide), the points differing per member;
    member 6 has x1 = x2.  Status and first bad cell per member are the lone calls', every good matrix its lone call's and
    build()'s."""
    B = GROUP + 1
    assert B == 9
    c0 = ni.chain(pkg, ni.BASE)
    cells, gens = c0[0].seed_cells(), c0[0].generators()
    cd = pkg.CircuitData(c0[0].blob())
    plan = cd.witness_plan(cells, compile=compile, generators=gens)
    m = ni.ORDER[ni.BASE]
    values, want = [], []
    for k in range(B):
        pts = [(v * (2 * k + 3) + k) % m for v in CHAIN_POINTS]
        if k == 6:
            pts[2] = pts[0]
        c = ni.chain(pkg, ni.BASE)
        if k != 6:
            _, wires = c[0].build(ni.chain_operands(c, *pts))
            assert [c[0].value_of(t) for t in c[2]] == ni.digits(ni.chain_x3(ni.BASE, *pts), ni.L)
            values.append([int(wires[col, row]) for row, col in cells])
            want.append(wires)
        else:
            values.append(c[0].seed_values(ni.chain_operands(c, *pts)))
            want.append(None)
    assert len({tuple(v) for v in values}) == B
    got, status, bad = plan.generate_batch(values)
    assert [s != 0 for s in status] == [k == 6 for k in range(B)], status
    for k in range(B):
        if k == 6:
            assert status[k] == E_UNSATISFIED and bad[k] == tuple(gens[2][1][0][0])
            assert _refused(pkg, plan, values[k], 2) == bad[k]
        else:
            assert bad[k] is None
            assert np.array_equal(_matrix(got[k]), want[k]), k
            assert np.array_equal(_matrix(plan.generate(values[k])), want[k]), k
    plan.close()
    cd.close()
