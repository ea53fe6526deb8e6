"""The u32 / biguint gadgets and the div-rem generator on the MI355X: the circuits of tests/test_reference_biguint_tests.py and
a 16-by-8-limb div_rem (a 512-bit product reduced modulo the secp256k1 base-field prime, the shape `nonnative` reduces with)
proved through the C ABI to the oracle's bytes, and their witnesses generated on the device by plans that carry the generator
(p2gpu_witness_plan_create_genv / _build_genv; csrc/planhost.hpp, genplan.hip, genwit.hip, bigdiv.hpp).  Expected matrices
come from translate.py's build() event loop, expected bytes from the oracle, expected quotients from Python integers, never
from the code under test.  Every circuit has at most 2^7 rows.  No test provokes a device fault: every negative is a value the
walk compares or rejects."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import biguint_inputs as bi  # noqa: E402
import device_build_inputs as dbi  # noqa: E402

E_UNSATISFIED, E_ARG = -5, -7
W = 0x80000000
with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "acvm-backend-plonky2_amd", "csrc", "genwit.hip")) as _f:
    GROUP = int(re.search(r"constexpr uint32_t WALK_GROUP = (\d+);", _f.read()).group(1))   # witnesses per workgroup of the walk
CELL = re.compile(r"\(row (\d+), column (\d+)\)")
# the 512-bit product of two field elements, and what it reduces to
PRODUCT = (0xC6EF372F_E94F82BE_3B9AC9FF_54A0B1D7_9E3779B9_7F4A7C15_F39CC060_5CEDC834 * 0xA54FF53A_5F1D36F1_510E527F_ADE682D1_9B05688C_2B3E6C1F_1F83D9AB_FB41BD6B)
assert PRODUCT >> 480 and PRODUCT < bi.SECP256K1_P ** 2


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


def _wide_case(pkg):
    c = bi.div_rem_virtual(pkg, 16, 8)
    return c[0], bi.operands(c, PRODUCT, bi.SECP256K1_P)


@pytest.fixture(scope="module")
def cases(pkg):
    """name -> (builder, blob, wires): the reference's five tests and the 16-by-8 div_rem, built once."""
    out = {}
    for name, make in bi.REFERENCE_CASES + [("div_rem_16_by_8", None)]:
        b, w = make(pkg) if make else _wide_case(pkg)
        blob, wires = b.build(w)
        assert wires.shape[1] <= 1 << 7, name
        out[name] = (b, blob, wires)
    return out


NAMES = [c[0] for c in bi.REFERENCE_CASES] + ["div_rem_16_by_8"]


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
    assert [g[0] for g in gens] == (["biguint_divrem"] if name.startswith("div_rem") else [])
    if name == "div_rem_16_by_8":
        (_, groups), = gens
        assert [len(g) for g in groups] == [16, 8, 9, 8]
        q, r = divmod(PRODUCT, bi.SECP256K1_P)
        assert [int(wires[c, row]) for grp in groups[2:] for row, c in grp] == bi.digits(q, 9) + bi.digits(r, 8)
    exported = {}
    for compile in ("host", "device"):
        plan = cd.witness_plan(cells, compile=compile, generators=gens)
        bad = np.argwhere(_matrix(plan.generate(values)) != wires)
        assert bad.size == 0, (compile, [(int(c), int(r)) for c, r in bad[:8]])
        assert plan.prove(values).to_bytes() == want
        exported[compile] = plan.export() + plan.export_generators_v()
        if gens:
            with pytest.raises(pkg.P2GpuError) as e:      # the four-cell export does not read this plan
                plan.export_generators()
            assert e.value.code == E_ARG
        plan.close()
    for h, dv in zip(exported["host"], exported["device"]):
        assert h.dtype == dv.dtype and h.shape == dv.shape and h.tobytes() == dv.tobytes()
    cell_slot, ops, level_off, off, table = exported["host"]
    codes = (ops >> np.uint64(32)) & np.uint64(0xFF)
    assert np.count_nonzero(codes == 14) == len(gens) and list(off) == [0] + [sum(len(g) for g in groups) for _, groups in gens]
    if gens:
        ins = len(gens[0][1][0]) + len(gens[0][1][1])
        assert not (table[:ins] & W).any()
        # div and rem are the generator's to write unless a ConstantGate holds them (the reference's test connects both)
        assert (table[ins:] & W).all() == (name == "div_rem_16_by_8")
    cd.close()


def _virtual(pkg, la=4, lb=4):
    c = bi.div_rem_virtual(pkg, la, lb)
    return c, c[0].blob()


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_edge_operands_on_the_device(pkg, orc, gpu, compile):
    """One plan per shape, the operands as seeds: every matrix is build()'s (quotients from Python's divmod).  The circuit whose
    div has no limbs holds U32AddManyGate { num_addends: 0 } rows: it is proved to the oracle's bytes as well."""
    by_shape = {}
    for name, la, lb, a, b in bi.DIV_REM_EDGES:
        by_shape.setdefault((la, lb), []).append((name, a, b))
    for (la, lb), members in by_shape.items():
        c0, blob = _virtual(pkg, la, lb)
        cd = pkg.CircuitData(blob)
        plan = cd.witness_plan(c0[0].seed_cells(), compile=compile, generators=c0[0].generators())
        for name, a, b in members:
            c, _ = _virtual(pkg, la, lb)
            _, wires = c[0].build(bi.operands(c, a, b))
            q, r = divmod(a, b)
            assert [c[0].value_of(t) for t in c[3] + c[4]] == bi.digits(q, len(c[3])) + bi.digits(r, lb), name
            cells, values = _seeds(c[0], wires)
            bad = np.argwhere(_matrix(plan.generate(values)) != wires)
            assert bad.size == 0, (name, [(int(x), int(y)) for x, y in bad[:8]])
            if name == "div_without_limbs":
                oc = orc.OracleCircuit(blob)
                want, _ = oc.prove(wires, public_inputs=[])
                assert oc.verify(want) and cd.prove(wires).to_bytes() == want == plan.prove(values).to_bytes()
                oc.close()
        plan.close()
        cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_contradictions_are_named(pkg, gpu, compile):
    """b = 0: P2GPU_E_UNSATISFIED naming the generator and b's first cell.  A quotient with more digits than div has limbs:
    div's top limb.  An extra seed on a rem limb: the right value is compared and accepted, a wrong one is named at that cell."""
    c, blob = _virtual(pkg)
    b = c[0]
    (_, (ca, cb, cdiv, crem)), = b.generators()
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(b.seed_cells(), compile=compile, generators=b.generators())

    def refused(a_value, b_value):
        with pytest.raises(pkg.P2GpuError) as e:
            plan.generate(b.seed_values(bi.operands(c, a_value, b_value)))
        assert e.value.code == E_UNSATISFIED and "generator 0" in str(e.value), e.value
        return tuple(int(v) for v in CELL.search(str(e.value)).groups())

    assert refused(bi.X128, 0) == tuple(cb[0])
    assert divmod(bi.X128, bi.Y128 >> 40)[0] >> 32
    assert refused(bi.X128, bi.Y128 >> 40) == tuple(cdiv[-1])
    plan.close()
    c2, _ = _virtual(pkg)
    _, wires = c2[0].build(bi.operands(c2, bi.X128, bi.Y128))
    cells, values = _seeds(c2[0], wires, extra=[crem[1]])
    plan = cd.witness_plan(cells, compile=compile, generators=b.generators())
    off, table = plan.export_generators_v()
    k = 4 + 4 + 1 + 1
    assert not table[k] & W and table[k - 1] & W and table[k + 1] & W          # the seed writes, the generator compares
    assert np.array_equal(_matrix(plan.generate(values)), wires)
    with pytest.raises(pkg.P2GpuError) as e:
        plan.generate(values[:-1] + [(values[-1] + 1) & bi.M])
    assert e.value.code == E_UNSATISFIED and "generator 0" in str(e.value), e.value
    assert tuple(int(v) for v in CELL.search(str(e.value)).groups()) == tuple(crem[1]), e.value
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_refused_lists_from_both_compilers(pkg, gpu):
    """Every refusal of a generator list comes back as P2GPU_E_ARG with the same words from p2gpu_witness_plan_create_genv and
    from p2gpu_witness_plan_build_genv."""
    c, blob = _virtual(pkg, 4, 2)
    b = c[0]
    (_, groups), = b.generators()
    cd = pkg.CircuitData(blob)
    n, R, lib = cd.degree, cd.num_routed_wires, cd._lib
    outside = (groups[0], groups[1], groups[2][:2] + ((groups[2][2][0], R),), groups[3])
    below = (groups[0], groups[1], groups[2], ((n, 0), groups[3][1]))
    lists = [
        ([(7, groups)], "generator 0 has the unknown kind 7"),
        ([("biguint_divrem", (groups[0], groups[1], groups[2][:2], groups[3]))], "generator 0 of kind 1 has the shape {4, 2, 2, 2}, which is not a shape of its kind"),
        ([("equality", (groups[0][:2], groups[1][:1], groups[2][:1], groups[3][:1]))], "generator 0 of kind 0 has the shape {2, 1, 1, 1}, which is not a shape of its kind"),
        ([("biguint_divrem", outside)], "generator 0 names cell (row %d, column %d) outside the %d x %d routed cells" % (groups[2][2][0], R, n, R)),
        ([("biguint_divrem", groups), ("biguint_divrem", below)], "generator 1 names cell (row %d, column 0) outside the %d x %d routed cells" % (n, n, R)),
    ]
    seeds = np.array(b.seed_cells(), dtype=np.uint32)
    recs = np.array([[1, 4, 2, 3, 2]], dtype=np.uint32)
    flat = np.array([cell for g in groups for cell in g], dtype=np.uint32)
    raw = [
        ((recs.ctypes.data, 1, flat.ctypes.data, 10), "the shapes of the generators up to generator 0 name 11 cells, 10 are given"),
        ((None, 1, flat.ctypes.data, 11), "generators are counted but the list is a null pointer"),
        ((recs.ctypes.data, 1, None, 11), "generator cells are counted but the list is a null pointer"),
    ]
    lib.p2gpu_last_error.restype = ctypes.c_char_p
    for compile in ("host", "device"):
        for gens, words in lists:
            with pytest.raises(pkg.P2GpuError) as e:
                cd.witness_plan(b.seed_cells(), compile=compile, generators=gens)
            assert e.value.code == E_ARG and words in str(e.value), (compile, e.value)
        make = lib.p2gpu_witness_plan_build_genv if compile == "device" else lib.p2gpu_witness_plan_create_genv
        for (g, ng, cl, nc), words in raw:
            h = ctypes.c_void_p()
            assert make(cd._h, seeds.ctypes.data, len(seeds), g, ng, cl, nc, ctypes.byref(h)) == E_ARG and not h.value
            assert lib.p2gpu_last_error().decode() == words, compile
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_batch_of_the_div_rem_circuit(pkg, gpu, compile):
    """WALK_GROUP + 1 witnesses of the 128-bit div_rem circuit (two workgroups, the second one lane wide), the operands
    differing: member 2 divides by one limb, member 5 takes the add-back step, member 6 has b = 0.  Status and first bad cell
    per member are the lone calls', every good matrix its lone call's and build()'s."""
    B = GROUP + 1
    assert B == 9
    c0, blob = _virtual(pkg)
    cells = c0[0].seed_cells()
    (_, (_, cb, _, _)), = c0[0].generators()
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells, compile=compile, generators=c0[0].generators())
    values, want = [], []
    for m in range(B):
        a, b = (bi.X128 >> m) | 1, (bi.Y128 >> (2 * m + 1)) | (1 << 120)
        if m == 2:
            a, b = 0xFFFFFFF0_12345678, 0xFFFFFFF1
        if m == 5:
            a, b = bi.ADD_BACK_A, bi.ADD_BACK_B
        if m == 6:
            b = 0
        c, _ = _virtual(pkg)
        if b:
            _, wires = c[0].build(bi.operands(c, a, b))
            assert [c[0].value_of(t) for t in c[3] + c[4]] == bi.digits(a // b, 1) + bi.digits(a % b, 4)
            values.append([int(wires[col, row]) for row, col in cells])
            want.append(wires)
        else:
            values.append(c[0].seed_values(bi.operands(c, a, b)))
            want.append(None)
    assert len({tuple(v) for v in values}) == B
    got, status, bad = plan.generate_batch(values)
    assert [s != 0 for s in status] == [m == 6 for m in range(B)], status
    for m in range(B):
        if m == 6:
            assert status[m] == E_UNSATISFIED and bad[m] == tuple(cb[0])
            with pytest.raises(pkg.P2GpuError) as e:
                plan.generate(values[m])
            assert e.value.code == E_UNSATISFIED
            assert tuple(int(x) for x in CELL.search(str(e.value)).groups()) == bad[m], (e.value, bad[m])
        else:
            assert bad[m] is None
            assert np.array_equal(_matrix(got[m]), want[m]), m
            assert np.array_equal(_matrix(plan.generate(values[m])), want[m]), m
    plan.close()
    cd.close()
