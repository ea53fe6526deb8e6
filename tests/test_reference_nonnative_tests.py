"""The reference's nonnative gadget tests, one to one, with fixed values in place of FF::rand(): plonky2_ecdsa/biguint/gadgets/
nonnative.rs:739-908 (add, sub, mul, neg, inv), over both fields the reference instantiates, and the chain of
tests/nonnative_inputs.py; the circuits are restated there.  Every reference test is "build circuit -> real prove -> real
verify"; so is every test here: restated gadgets (translate.py) -> p2gpu_build_blob -> prove -> verify on the CPU oracle.
tests/test_gpu_nonnative.py runs the same circuits on the MI355X."""
import pytest

import nonnative_inputs as ni


def _prove(orc, blob, wires, max_rows):
    assert wires.shape[1] <= max_rows
    oc = orc.OracleCircuit(blob)
    try:
        proof, _ = oc.prove(wires, public_inputs=[])
        assert oc.verify(proof)
    finally:
        oc.close()


CASES = [(name, make, f) for f in ni.FIELDS for name, make in ni.REFERENCE_CASES]
IDS = ["%s_%s" % (name, f) for name, _, f in CASES]


@pytest.mark.parametrize("name,make,field", CASES, ids=IDS)
def test_reference_nonnative_test_on_the_oracle(pkg, orc, name, make, field):
    b, w = make(pkg, field)
    blob, wires = b.build(w)
    _prove(orc, blob, wires, 1 << 7)
    kind = {"add": "nonnative_add", "sub": "nonnative_sub", "neg": "nonnative_sub", "mul": "nonnative_mul", "inv": "nonnative_inv"}[name]
    (g,) = b.generators()
    assert g[0] == kind and g[2] == field
    assert [len(x) for x in g[1]] == {"add": [8, 8, 8, 1], "sub": [8, 8, 8, 1], "neg": [0, 8, 8, 1], "mul": [8, 8, 8, 8], "inv": [8, 0, 8, 8]}[name]
    kinds = {r["kind"] for r in b.rows}
    assert kinds >= {"add": {"u32addmany", "cmp", "arith"}, "sub": {"u32range", "u32sub"}, "neg": {"u32range", "u32sub"},
                     "mul": {"u32range", "u32arith", "u32addmany"}, "inv": {"u32arith", "u32addmany"}}[name]


@pytest.mark.parametrize("name,make,field", CASES, ids=IDS)
def test_a_wrong_claimed_constant_is_refused(pkg, name, make, field):
    m = ni.ORDER[field]
    right = {"add": (ni.X256 + ni.Y256) % m, "sub": (ni.X256 - ni.Y256) % m, "mul": ni.X256 * ni.Y256 % m, "neg": m - ni.X256,
             "inv": pow(ni.X256, -1, m)}[name]
    make(pkg, field, claimed=right)[0].build({})
    for wrong in ((right + 1) % m, right ^ (1 << 255)):
        if wrong >= m:
            continue
        b, w = make(pkg, field, claimed=wrong)
        with pytest.raises(ValueError):
            b.build(w)


@pytest.mark.parametrize("field", ni.FIELDS)
def test_chain_on_the_oracle(pkg, orc, field):
    """x3 of curve_add's formula from seven generators; x1 = x2 inverts zero: build() raises as upstream panics."""
    c = ni.chain(pkg, field)
    assert [g[0] for g in c[0].generators()] == ni.CHAIN_KINDS
    blob, wires = c[0].build(ni.chain_operands(c, ni.X256, ni.Y256, ni.Z256, ni.V256))
    assert [c[0].value_of(t) for t in c[2]] == ni.digits(ni.chain_x3(field, ni.X256, ni.Y256, ni.Z256, ni.V256), ni.L)
    _prove(orc, blob, wires, 1 << 9)
    c = ni.chain(pkg, field)
    with pytest.raises(ValueError, match="inverts zero"):
        c[0].build(ni.chain_operands(c, ni.X256, ni.Y256, ni.X256, ni.V256))


@pytest.mark.parametrize("field", ni.FIELDS)
@pytest.mark.parametrize("kind", ["add", "sub", "mul", "inv"])
def test_an_operand_of_the_order_or_above_is_unsatisfiable(pkg, kind, field):
    """The generator reduces its operands first, the constraint does not: raw limbs >= M make the circuit unsatisfiable, as
    upstream.  (The same operand below M builds.)"""
    m = ni.ORDER[field]
    c = ni.virtual(pkg, kind, field)
    y = 0 if kind == "inv" else ni.Y256
    c[0].build(ni.operands(c, m - 5, y))
    c = ni.virtual(pkg, kind, field)
    with pytest.raises(ValueError):
        c[0].build(ni.operands(c, m + 5, y))


@pytest.mark.parametrize("name,kind,la,lb,fa,fb", ni.EDGES, ids=[e[0] for e in ni.EDGES])
def test_edge_operands_build_and_prove(pkg, orc, name, kind, la, lb, fa, fb):
    """Every edge circuit is satisfied by what Python expects (A + B = M: sum = M, overflow 0); one field is proved."""
    for field in ni.FIELDS:
        c = ni.virtual(pkg, kind, field, la, lb)
        blob, wires = c[0].build(ni.operands(c, fa(field), fb(field)))
        first, second = ni.expected(kind, field, fa(field), fb(field))
        assert [c[0].value_of(t) for t in c[3]] == ni.digits(first, len(c[3])) and [c[0].value_of(t) for t in c[4]] == ni.digits(second, len(c[4])), field
        if field == ni.SCALAR:
            _prove(orc, blob, wires, 1 << 7)


def test_what_upstream_panics_on_raises(pkg):
    """The inverse of zero; an inverse that needs eight digits in a target of four limbs; fewer operand limbs than the modulus has."""
    c = ni.virtual(pkg, "inv", ni.BASE)
    with pytest.raises(ValueError, match="inverts zero"):
        c[0].build(ni.operands(c, 0))
    c = ni.virtual(pkg, "inv", ni.BASE, la=4)
    assert pow(3, -1, ni.ORDER[ni.BASE]) >> 128
    with pytest.raises(ValueError, match="more digits"):
        c[0].build(ni.operands(c, 3))
    b = ni.builder(pkg)
    with pytest.raises(ValueError):
        b.mul_nonnative(b.add_virtual_biguint_target(3), b.add_virtual_biguint_target(4), ni.BASE)


def test_the_other_gadgets(pkg, orc):
    """if_nonnative, nonnative_conditional_neg, mul_many_nonnative, reduce, bool_to_nonnative and split_nonnative_to_bits on
    constants, proved: the selected, negated, multiplied and reduced values are Python's."""
    f, m = ni.BASE, ni.ORDER[ni.BASE]
    b = ni.builder(pkg)
    x, y, z = (b.constant_nonnative(v, f) for v in (ni.X256, ni.Y256, ni.Z256))
    t, fl = b.constant_bool(True), b.constant_bool(False)
    b.connect_nonnative(b.if_nonnative(t, x, y, f), x, f)
    b.connect_nonnative(b.if_nonnative(fl, x, y, f), y, f)
    b.connect_nonnative(b.nonnative_conditional_neg(x, t, f), b.constant_nonnative(m - ni.X256, f), f)
    b.connect_nonnative(b.mul_many_nonnative([x, y, z], f), b.constant_nonnative(ni.X256 * ni.Y256 * ni.Z256 % m, f), f)
    b.connect_nonnative(b.reduce(b.constant_biguint(ni.X256 * ni.Y256), f), b.constant_nonnative(ni.X256 * ni.Y256 % m, f), f)
    b.connect_nonnative(b.add_nonnative(x, b.bool_to_nonnative(t, f), f), b.constant_nonnative(ni.X256 + 1, f), f)
    bits = b.split_nonnative_to_bits(b.constant_nonnative(5, f), f)
    assert len(bits) == 32 and b.num_nonnative_limbs(f) == 8 and b.zero_nonnative(f) == []
    for i, bit in enumerate(bits):
        b.connect(bit, b.constant_bool(i in (0, 2)))
    blob, wires = b.build({})
    assert [g[0] for g in b.generators()].count("nonnative_mul") == 2
    _prove(orc, blob, wires, 1 << 10)
