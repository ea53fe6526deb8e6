"""The curve and GLV gadgets and the GLV decomposition generator on the MI355X: witnesses generated on the device by plans that
carry the generator (p2gpu_witness_plan_create_genv / _build_genv; csrc/planhost.hpp, genplan.hip, genwit.hip, glv.hpp), compared
with translate.py's build() matrix word for word, and proofs from device witnesses compared with the proofs of the host matrix
byte for byte.  Expected decompositions and points come from the integer model of tests/curve_inputs.py, never from the code
under test.  Shapes: the decomposition circuit has a few hundred rows, one curve operation at most 2^10, the one-limb MSM 2^14
(sixteen windows reach every table path), one whole glv_mul 2^16 and the whole opcode 2^17, each of the last three built once per
module -- their cost is the host build, not the GPU.  No test provokes a device fault: every negative is a value the walk
compares or rejects, or a list the plan refuses before anything indexes with it."""
import os
import re
import sys
import time

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve_inputs as ci  # noqa: E402

E_UNSATISFIED, E_ARG = -5, -7
CELL = re.compile(r"\(row (\d+), column (\d+)\)")


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


def _matrix(t):
    return t.cpu().numpy().view(np.uint64)


def _seeds(builder, wires):
    cells = builder.seed_cells()
    return cells, [int(wires[c, r]) for r, c in cells]


def _same_plans(pkg, cd, cells, gens):
    """both compilers' plans of one circuit, equal byte for byte in cell_slot, ops, level_off, the offsets and the table"""
    plans = {compile: cd.witness_plan(cells, compile=compile, generators=gens) for compile in ("host", "device")}
    exported = {k: p.export() + p.export_generators_v() for k, p in plans.items()}
    for h, dv in zip(exported["host"], exported["device"]):
        assert h.dtype == dv.dtype and h.shape == dv.shape and h.tobytes() == dv.tobytes()
    return plans, exported["host"]


def _decomposed(matrix, groups):
    """(k1, k2, k1_neg, k2_neg) read from a wire matrix at the generator's cells"""
    words = [int(matrix[col, row]) for row, col in groups[2]]
    signs = [int(matrix[col, row]) for row, col in groups[3]]
    return ci.fold(words[:4]), ci.fold(words[4:]), bool(signs[0]), bool(signs[1])


# -- 1. the decomposition circuit alone ---------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def decomposition(pkg, gpu):
    c = ci.decomposition(pkg)
    cd = pkg.CircuitData(c[0].blob())
    assert cd.degree <= 1 << 9
    plans, exported = _same_plans(pkg, cd, c[0].seed_cells(), c[0].generators())
    yield c, cd, plans, exported
    for p in plans.values():
        p.close()
    cd.close()


@pytest.mark.gpu
def test_decomposition_of_every_stated_scalar(pkg, gpu, decomposition):
    """From the eight k limbs alone the device's matrix is build()'s, for either compiler's plan, and k1, k2 and the signs in it
    are the model's; the plan's record of the generator carries code 19 and no field."""
    c, cd, plans, (cell_slot, ops, level_off, off, table) = decomposition
    gens = c[0].generators()
    assert gens[0][0] == "glv_decompose" and len(gens[0]) == 2
    assert [int(o) for o in ops if ((int(o) >> 32) & 0xFF) == ci.OP_CODE] == [0 | ci.OP_CODE << 32]
    assert not (table[:8] & 0x80000000).any() and (table[8:18] & 0x80000000).all()
    for k in ci.SCALARS:
        cc = ci.decomposition(pkg)
        _, wires = cc[0].build(ci.scalar_witness(cc, ci.digits(k, ci.L)))
        cells, values = _seeds(cc[0], wires)
        for compile, plan in plans.items():
            got = _matrix(plan.generate(values))
            bad = np.argwhere(got != wires)
            assert bad.size == 0, (hex(k), compile, [(int(x), int(y)) for x, y in bad[:8]])
        assert _decomposed(got, gens[0][1]) == ci.decompose(k), hex(k)


@pytest.mark.gpu
def test_a_batch_of_nine_scalars_goes_through_one_walk(pkg, gpu, decomposition):
    c, cd, plans, _ = decomposition
    scalars = ci.SCALARS[3:12]
    assert len(set(scalars)) == 9
    values, want = [], []
    for k in scalars:
        cc = ci.decomposition(pkg)
        _, wires = cc[0].build(ci.scalar_witness(cc, ci.digits(k, ci.L)))
        values.append(_seeds(cc[0], wires)[1])
        want.append(wires)
    for plan in plans.values():
        got, status, bad = plan.generate_batch(values)
        assert status == [0] * 9 and bad == [None] * 9
        for i in range(9):
            assert np.array_equal(_matrix(got[i]), want[i]), i


@pytest.mark.gpu
def test_a_scalar_of_the_order_or_above_is_reduced_first(pkg, gpu, decomposition):
    """k = N + 12345 as raw limbs: the generator decomposes 12345 (k mod N: from_noncanonical_biguint), which the device's matrix
    shows at the generator's cells; the circuit's own check, which is on the raw limbs, then fails: P2GPU_E_UNSATISFIED for that
    member, as build() refuses it."""
    c, cd, plans, _ = decomposition
    groups = c[0].generators()[0][1]
    good = ci.decomposition(pkg)
    _, wires = good[0].build(ci.scalar_witness(good, ci.digits(12345, ci.L)))
    cells, values = _seeds(good[0], wires)
    raw = ci.decomposition(pkg)
    above = raw[0].seed_values(ci.scalar_witness(raw, ci.digits(ci.N + 12345, ci.L)))
    assert len(above) == len(values) and above[:8] == ci.digits(ci.N + 12345, ci.L)
    above[8:] = values[8:]                                       # (the PublicInputGate row's wires as the good witness has them)
    got, status, bad = plans["host"].generate_batch([values, above])
    assert status == [0, E_UNSATISFIED] and np.array_equal(_matrix(got[0]), wires)
    assert _decomposed(_matrix(got[1]), groups) == ci.decompose(12345) == _decomposed(wires, groups)
    assert bad[0] is None and bad[1] is not None
    with pytest.raises(ValueError):
        raw[0].build(ci.scalar_witness(raw, ci.digits(ci.N + 12345, ci.L)))


@pytest.mark.gpu
def test_sixteen_limbs_fold_and_reduce(pkg, gpu):
    """A sixteen-limb scalar of N or above, and limbs of 2^32 and above, through the generator without the gadget's check around
    it (which holds for reduced scalars only): the device's matrix is build()'s and its ten cells are the model's for
    fold(limbs) mod N."""
    for limbs in (ci.LIMB_LISTS[0], ci.LIMB_LISTS[1], [ci.GOLDILOCKS - 1] * 16, [5]):
        c = ci.generator_only(pkg, len(limbs))
        (_, groups), = c[0].generators()
        assert [len(g) for g in groups] == [len(limbs), 0, 8, 2]
        blob, wires = c[0].build(ci.scalar_witness(c, limbs))
        assert _decomposed(wires, groups) == ci.decompose(ci.fold(limbs) % ci.N), limbs
        cells, values = _seeds(c[0], wires)
        cd = pkg.CircuitData(blob)
        for compile in ("host", "device"):
            plan = cd.witness_plan(cells, compile=compile, generators=c[0].generators())
            assert np.array_equal(_matrix(plan.generate(values)), wires), (limbs, compile)
            plan.close()
        cd.close()


# -- 2. one curve operation ------------------------------------------------------------------------------------------------------
def _device_witness_and_proof(pkg, b, blob, wires, max_rows, compilers=("host", "device")):
    cd = pkg.CircuitData(blob)
    assert cd.degree <= max_rows
    want = cd.prove(wires).to_bytes()
    cd.verify(want)
    cells, values = _seeds(b, wires)
    walk = {}
    for compile in compilers:
        plan = cd.witness_plan(cells, compile=compile, generators=b.generators())
        bad = np.argwhere(_matrix(plan.generate(values)) != wires)
        assert bad.size == 0, (compile, [(int(c), int(r)) for c, r in bad[:8]])
        got = plan.prove(values).to_bytes()
        assert got == want
        cd.verify(got)
        walk[compile] = plan.info()
        plan.close()
    cd.close()
    return walk


OPS = [("add", None), ("double", None), ("conditional_add", 1), ("conditional_add", 0), ("assert_valid", None)]


@pytest.mark.gpu
@pytest.mark.parametrize("op,bit", OPS, ids=["add", "double", "conditional_add_true", "conditional_add_false", "assert_valid"])
def test_curve_operation_on_the_device(pkg, gpu, op, bit):
    c = ci.curve_op(pkg, op)
    points = [ci.MSM_P, ci.MSM_Q][:len(c[1])]
    blob, wires = c[0].build(ci.curve_op_witness(c, points, bit))
    if c[3] is not None:
        want = {"add": lambda: ci.add(*points), "double": lambda: ci.double(points[0]),
                "conditional_add": lambda: ci.add(*points) if bit else points[0]}[op]()
        assert ci.point_of(c[0], c[3]) == want and ci.on_curve(want)
    _device_witness_and_proof(pkg, c[0], blob, wires, 1 << 10)


@pytest.mark.gpu
@pytest.mark.parametrize("index", [0, 5, 15])
def test_random_access_curve_points_on_the_device(pkg, gpu, index):
    c = ci.random_access(pkg)
    blob, wires = c[0].build({c[1]: index})
    assert ci.point_of(c[0], c[2]) == ci.TABLE[index]
    _device_witness_and_proof(pkg, c[0], blob, wires, 1 << 10)


# -- 3. unsatisfiable operands -----------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("compile", ["host", "device"])
def test_curve_add_of_a_point_with_itself_is_named(pkg, gpu, compile):
    """x2 - x1 = 0 has no inverse: P2GPU_E_UNSATISFIED naming the inverse generator (the third of curve_add) and v's first cell"""
    c = ci.curve_op(pkg, "add")
    gens = c[0].generators()
    assert gens[2][0] == "nonnative_inv"
    cd = pkg.CircuitData(c[0].blob())
    plan = cd.witness_plan(c[0].seed_cells(), compile=compile, generators=gens)
    with pytest.raises(pkg.P2GpuError) as e:
        plan.generate(c[0].seed_values(ci.curve_op_witness(c, [ci.MSM_P, ci.MSM_P])))
    assert e.value.code == E_UNSATISFIED and "generator 2" in str(e.value), e.value
    assert tuple(int(v) for v in CELL.search(str(e.value)).groups()) == tuple(gens[2][1][0][0])
    plan.close()
    cd.close()


# -- 4. the window walk with one-limb scalars ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def msm(pkg, gpu):
    c = ci.msm_one_limb(pkg)
    cd = pkg.CircuitData(c[0].blob())
    assert cd.degree == 1 << 14
    plan = cd.witness_plan(c[0].seed_cells(), generators=c[0].generators())
    yield c, cd, plan
    plan.close()
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("n,m", ci.MSM_SCALARS, ids=["%x_%x" % s for s in ci.MSM_SCALARS])
def test_msm_with_one_limb_scalars(pkg, gpu, msm, n, m):
    """Sixteen windows: (0x2D, 0) and (0, 0xC0000001) walk the p and the q column of the table and many zero indices (no add),
    (0xFFFFFFFF, 0x1B) the mixed entries; the device's matrix is build()'s and the result limbs are the model's."""
    c, cd, plan = msm
    _, wires = c[0].build({c[1][0]: n, c[2][0]: m})
    want = ci.msm(ci.MSM_P, ci.MSM_Q, n, m, 1)
    assert ci.point_of(c[0], c[3]) == want
    cells, values = _seeds(c[0], wires)
    got = _matrix(plan.generate(values))
    bad = np.argwhere(got != wires)
    assert bad.size == 0, [(int(x), int(y)) for x, y in bad[:8]]
    cell = lambda t: c[0].cells_of(t)[0]  # noqa: E731
    limbs = [[int(got[cell(t)[1], cell(t)[0]]) for t in coordinate] for coordinate in c[3]]
    assert (ci.fold(limbs[0]), ci.fold(limbs[1])) == want


# -- 5. refusals from both compilers ----------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_refused_lists_from_both_compilers(pkg, gpu, decomposition):
    c, cd, _, _ = decomposition
    b = c[0]
    groups = b.generators()[0][1]
    n, R = cd.degree, cd.num_routed_wires
    k, _, out, signs = groups
    outside = (k, (), out[:3] + ((out[3][0], R),) + out[4:], signs)
    shape = "generator 0 of kind 8 has the shape {%d, %d, %d, %d}, which is not a shape of its kind"
    lists = [([(word, groups)], "generator 0 has the unknown kind %d" % word) for word in (8 | 1 << 8, 8 | 1 << 16, 9, 6, 7)]
    lists += [
        ([("glv_decompose", ((), (), out, signs))], shape % (0, 0, 8, 2)),
        ([("glv_decompose", (k + k + k[:1], (), out, signs))], shape % (17, 0, 8, 2)),
        ([("glv_decompose", (k, k[:1], out, signs))], shape % (8, 1, 8, 2)),
        ([("glv_decompose", (k, (), out[:7], signs))], shape % (8, 0, 7, 2)),
        ([("glv_decompose", (k, (), out, signs[:1]))], shape % (8, 0, 8, 1)),
        ([("glv_decompose", outside)], "generator 0 names cell (row %d, column %d) outside the %d x %d routed cells" % (out[3][0], R, n, R)),
    ]
    for compile in ("host", "device"):
        for gens, words in lists:
            with pytest.raises(pkg.P2GpuError) as e:
                cd.witness_plan(b.seed_cells(), compile=compile, generators=gens)
            assert e.value.code == E_ARG and words in str(e.value), (compile, e.value)


# -- 6. one whole glv_mul ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_glv_mul_of_the_recorded_vector_from_eight_limbs(pkg, gpu):
    """The reference's test_curve_mul circuit (2^16 rows): the witness on the device from the eight scalar limbs, the proof from
    it equal to the proof of build()'s matrix, accepted."""
    b, scalar = ci.glv_mul_case(pkg)
    k, x, y = ci.curve_mul_vector()
    t0 = time.time()
    blob, wires = b.build(dict(zip(scalar, ci.digits(k, ci.L))))
    host = time.time() - t0
    walk = _device_witness_and_proof(pkg, b, blob, wires, 1 << 16, compilers=("host",))
    print("glv_mul: host build %.1f s, plan %s" % (host, walk["host"]))


# -- 7. the whole opcode -------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_the_whole_opcode_from_the_prover_toml_bytes(pkg, orc, gpu):
    """program bytes -> to_translator_opcodes -> translate -> witness_seeds + witness_generators -> plan -> prove -> verify: the
    bytes are the oracle's proof of build()'s matrix.  The one large test (2^17 rows): its time is the host build and the
    oracle's proof, not the GPU."""
    circuit, witness = ci.ecdsa_program()
    circuit = pkg.acir.deserialize_program(pkg.acir.serialize_program([circuit]))["functions"][0]
    tr = pkg.translate.CircuitBuilderFromAcirToPlonky2()
    tr.translate_circuit(pkg.acir.to_translator_opcodes(circuit), circuit["public_parameters"], circuit["private_parameters"])
    t0 = time.time()
    blob, wires = tr.build(dict(witness))
    host = time.time() - t0
    assert tr.witness_value(ci.ECDSA_OUTPUT) == 1 and wires.shape[1] == 1 << 17
    cells = tr.builder.seed_cells()
    values = [int(wires[c, r]) for r, c in cells]
    assert values[:160] == tr.witness_seeds(witness)[1][:160] and cells == tr.witness_seeds(witness)[0]
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells, generators=tr.witness_generators())
    got = plan.prove(values, tr.public_inputs()).to_bytes()
    print("ecdsa opcode: host build %.1f s, plan %s" % (host, plan.info()))
    bad = np.argwhere(_matrix(plan.generate(values)) != wires)
    assert bad.size == 0, [(int(c), int(r)) for c, r in bad[:8]]
    cd.verify(got)
    plan.close()
    cd.close()
    oc = orc.OracleCircuit(blob)
    want, _ = oc.prove(wires, public_inputs=tr.public_inputs())
    assert oc.verify(want)
    oc.close()
    assert got == want
