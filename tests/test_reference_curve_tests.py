"""The reference's curve gadget tests, one to one, with fixed values: plonky2_ecdsa/curve/gadgets/curve.rs:330-545 -- the live
test_curve_mul and the ones the file keeps commented (point validity, double, add, conditional add, scalar_mul against double);
the circuits are restated in tests/curve_inputs.py.  Every reference test is "build circuit -> real prove -> real verify"; so is
every test here: restated gadgets (gadgets_curve.py, gadgets_glv.py) -> p2gpu_build_blob -> prove -> verify on the CPU oracle.
Expected points come from the integer model of curve_inputs.py and from the reference's recorded vector, never from the gadgets.
tests/test_gpu_curve.py runs circuits of the same gadgets on the MI355X."""
import pytest

import curve_inputs as ci


def _prove(orc, blob, wires, max_rows):
    assert wires.shape[1] <= max_rows
    oc = orc.OracleCircuit(blob)
    try:
        proof, _ = oc.prove(wires, public_inputs=[])
        assert oc.verify(proof)
    finally:
        oc.close()


def test_the_model_reproduces_the_recorded_vector():
    """the yardstick first: the window walk and the decomposition on integers give the reference's expected point"""
    k, x, y = ci.curve_mul_vector()
    assert k == ci.N - 5 and ci.on_curve((x, y))
    assert ci.glv(ci.G, k) == (x, y) == ci.mul(k, ci.G) == ci.neg(ci.mul(5, ci.G))
    assert ci.on_curve(ci.RANDO) and ci.on_curve(ci.TO_ADD) and all(ci.on_curve(pt) for pt in ci.TABLE)
    assert ci.msm(ci.MSM_P, ci.MSM_Q, 3 << 100, 7 << 64 | 9, 4) == ci.mul(((3 << 100) * 5 + (7 << 64 | 9) * 11) % ci.N, ci.G)


@pytest.mark.parametrize("make,rows", [(ci.point_is_valid, 1 << 9), (ci.double_case, 1 << 11), (ci.add_case, 1 << 10), (ci.conditional_add_case, 1 << 10)],
                         ids=["point_is_valid", "double", "add", "conditional_add"])
def test_reference_curve_test_on_the_oracle(pkg, orc, make, rows):
    b, w = make(pkg)
    blob, wires = b.build(w)
    _prove(orc, blob, wires, rows)
    assert {g[0] for g in b.generators()} <= {"nonnative_add", "nonnative_sub", "nonnative_mul", "nonnative_inv"}
    assert all(g[2] == ci.BASE for g in b.generators())


def test_a_point_off_the_curve_is_unsatisfiable(pkg):
    """curve.rs:354-380 test_curve_point_is_not_valid: (G.x, G.y + 1)"""
    assert not ci.on_curve((ci.GX, ci.GY + 1))
    b, w = ci.point_is_valid(pkg, bad=True)
    with pytest.raises(ValueError, match="unsatisfiable"):
        b.build(w)


def test_curve_add_has_the_stated_rows(pkg):
    """one curve_add over virtual points: ten nonnative generators in upstream's order, below 2^8 rows"""
    c = ci.curve_op(pkg, "add")
    assert [g[0].split("_")[1] for g in c[0].generators()] == ["sub", "sub", "inv", "mul", "mul", "add", "sub", "sub", "mul", "sub"]
    blob, wires = c[0].build(ci.curve_op_witness(c, [ci.MSM_P, ci.MSM_Q]))
    assert wires.shape[1] == 1 << 8
    assert ci.point_of(c[0], c[3]) == ci.add(ci.MSM_P, ci.MSM_Q) == ci.mul(16, ci.G)
    c = ci.curve_op(pkg, "add")
    with pytest.raises(ValueError, match="inverts zero"):
        c[0].build(ci.curve_op_witness(c, [ci.MSM_P, ci.MSM_P]))


def test_scalar_mul_by_two_is_double(pkg, orc):
    """curve.rs:520-545 test_curve_random: thirty-two double-and-add steps from a point drawn from the builder's seeded generator
    (upstream: the thread's); the drawn point is on the curve and the same for the same seed."""
    b, w = ci.scalar_mul_two_case(pkg)
    blob, wires = b.build(w)
    _prove(orc, blob, wires, 1 << 14)
    b1, b2 = ci.builder(pkg), ci.builder(pkg)
    pt = b1.generate_random_point()
    assert ci.on_curve(pt) and pt == b2.generate_random_point() and pt != b1.generate_random_point()


@pytest.fixture(scope="module")
def glv_mul(pkg):
    b, scalar = ci.glv_mul_case(pkg)
    return b, scalar, b.blob()


def test_glv_mul_of_the_recorded_vector(pkg, orc, glv_mul):
    """curve.rs:482-518 test_curve_mul: glv_mul(G, N - 5) is the recorded point; 2^16 rows"""
    b, scalar, _ = glv_mul
    k, x, y = ci.curve_mul_vector()
    blob, wires = b.build(dict(zip(scalar, ci.digits(k, ci.L))))
    assert wires.shape[1] == 1 << 16
    gens = b.generators()
    assert gens[0][0] == "glv_decompose" and [len(g) for g in gens[0][1]] == [8, 0, 8, 2] and len(gens[0]) == 2
    assert [g[0] for g in gens].count("glv_decompose") == 1 and [g[0] for g in gens].count("equality") == 64
    _prove(orc, blob, wires, 1 << 16)


def test_glv_mul_refuses_another_scalar(pkg, glv_mul):
    """the same circuit (the expected point is a constant of it) with the scalar N - 4"""
    b, scalar, _ = glv_mul
    with pytest.raises(ValueError):
        b.build(dict(zip(scalar, ci.digits(ci.N - 4, ci.L))))
