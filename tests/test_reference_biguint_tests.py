"""The reference's biguint and u32 gadget tests, one to one, with fixed values in place of OsRng: plonky2_ecdsa/biguint/
biguint.rs:374-521 (add, sub, mul, cmp, div_rem on 128-bit operands), gadgets/arithmetic_u32.rs:363-394 (test_add_many_u32s),
gadgets/multiple_comparison.rs:93-151 (test_list_le), the circuits restated in tests/biguint_inputs.py.  Every reference test
is "build circuit -> real prove -> real verify"; so is every test here: restated gadgets (translate.py) -> p2gpu_build_blob ->
prove -> verify on the CPU oracle.  tests/test_gpu_biguint.py runs the same circuits on the MI355X."""
import numpy as np
import pytest

import biguint_inputs as bi

MAX_ROWS = 1 << 7


def _prove(orc, blob, wires):
    assert wires.shape[1] <= MAX_ROWS
    oc = orc.OracleCircuit(blob)
    try:
        proof, _ = oc.prove(wires, public_inputs=[])
        assert oc.verify(proof)
    finally:
        oc.close()


def _gate_kinds(blob):
    h = np.ascontiguousarray(blob)[:256].view(np.uint32)
    table = np.ascontiguousarray(blob)[256:256 + 48 * int(h[23])].view(np.uint32).reshape(-1, 12)
    return [int(k) for k in table[:, 0]]


@pytest.mark.parametrize("name,make,num_wires", [c + (135,) for c in bi.REFERENCE_CASES] + [bi.REFERENCE_CASES[-1] + (234,)],
                         ids=[c[0] + "_135" for c in bi.REFERENCE_CASES] + ["div_rem_234"])
def test_reference_biguint_test_on_the_oracle(pkg, orc, name, make, num_wires):
    """The reference runs them at 135 wires (standard_recursion_config); div_rem here also at 234 (what the backend builds
    with), where the U32 rows hold 6 / 11 operations instead of 3 / 6."""
    b, w = make(pkg, num_wires=num_wires)
    blob, wires = b.build(w)
    _prove(orc, blob, wires)
    kinds = {r["kind"] for r in b.rows}
    assert kinds >= {"add": {"u32addmany"}, "sub": {"u32sub"}, "mul": {"u32arith", "u32addmany"}, "cmp": {"cmp", "arith"},
                     "div_rem": {"u32arith", "u32addmany", "cmp", "arith"}}[name]
    assert set(_gate_kinds(blob)) >= {{"u32arith": 7, "u32addmany": 8, "u32sub": 9, "cmp": 11}[k] for k in kinds if k in ("u32arith", "u32addmany", "u32sub", "cmp")}
    assert [g[0] for g in b.generators()] == (["biguint_divrem"] if name == "div_rem" else [])


@pytest.mark.parametrize("name,make", bi.REFERENCE_CASES, ids=[c[0] for c in bi.REFERENCE_CASES])
def test_a_wrong_claimed_output_is_refused(pkg, name, make):
    x, y = max(bi.X128, bi.Y128), min(bi.X128, bi.Y128)
    wrong = {"add": x + y + 1, "sub": x - y - 1, "mul": x * y + (1 << 64), "cmp": not (bi.X128 <= bi.Y128),
             "div_rem": (x // y, x % y + 1)}[name]
    b, w = make(pkg, claimed=wrong)
    with pytest.raises(ValueError):
        b.build(w)


def test_add_many_u32s(pkg, orc):
    """arithmetic_u32.rs:363-394: fifteen addends, one U32AddManyGate { num_addends: 15 } operation."""
    b, w = bi.add_many_case(pkg)
    blob, wires = b.build(w)
    _prove(orc, blob, wires)
    (row,) = [r for r in b.rows if r["kind"] == "u32addmany"]
    assert row["na"] == 15 and row["num_ops"] == 135 // (15 + 3 + 18) and len(row["ops"]) == 1
    with pytest.raises(ValueError):
        b2, w2 = bi.add_many_case(pkg, claimed=1)
        b2.build(w2)


@pytest.mark.parametrize("num_bits", [20, 32, 40, 44])
@pytest.mark.parametrize("size", [1, 3, 6])
def test_list_le(pkg, orc, size, num_bits):
    """multiple_comparison.rs:93-151 test_multiple_comparison: sizes 1, 3, 6 x widths 20, 32, 40, 44; two ComparisonGate rows
    per limb with chunk_bits = 2.  The wrong answer is refused."""
    b, w = bi.list_le_case(pkg, size, num_bits)
    blob, wires = b.build(w)
    _prove(orc, blob, wires)
    cmp_rows = [r for r in b.rows if r["kind"] == "cmp"]
    assert len(cmp_rows) == 2 * size and all(r["bits"] == num_bits and r["chunks"] == (num_bits + 1) // 2 for r in cmp_rows)
    b2, w2 = bi.list_le_case(pkg, size, num_bits, claimed=True)
    with pytest.raises(ValueError):
        b2.build(w2)


def test_gate_shapes_and_ids(pkg):
    """Operations per row and the (degree, id) order, from the gates' own source: arithmetic_u32.rs:39-42, add_many_u32.rs
    :43-48, subtraction_u32.rs:39-43; every distinct num_addends is its own gate; more than MAX_NUM_ADDENDS is refused."""
    for nw, arith, sub, am3, am15 in ((135, 3, 6, 5, 3), (234, 6, 11, 9, 4)):
        b = bi.builder(pkg, nw)
        assert (b.u32_gate_ops("u32arith"), b.u32_gate_ops("u32sub"), b.u32_gate_ops("u32addmany", 3), b.u32_gate_ops("u32addmany", 15)) == \
            (arith, sub, am3, am15)
    b = bi.builder(pkg)
    xs = b.add_virtual_u32_targets(17)
    b.add_many_u32(xs[:3])
    b.add_many_u32(xs[:4])
    b.add_many_u32(xs[4:7])
    assert [(r["kind"], r["na"], len(r["ops"])) for r in b.rows] == [("u32addmany", 3, 2), ("u32addmany", 4, 1)]
    with pytest.raises(ValueError, match="MAX_NUM_ADDENDS"):
        b.add_many_u32(xs)
    # the special cases: no gate for constants, none for 0 or 1 addends, add_u32 for 2
    n = len(b.rows)
    assert b.mul_add_u32(b.constant_u32(0xFFFFFFFF), b.constant_u32(0xFFFFFFFF), b.constant_u32(0xFFFFFFFF)) == \
        (b.constant_u32(0), b.constant_u32(0xFFFFFFFF))
    assert b.add_many_u32([]) == (b.zero(), b.zero()) and b.add_many_u32([xs[0]]) == (xs[0], b.zero()) and len(b.rows) == n
    b.add_many_u32(xs[:2])
    assert b.rows[-1]["kind"] == "u32arith" and b.rows[-1]["ops"][0][:3] == (xs[0], b.one(), xs[1])


@pytest.mark.parametrize("name,la,lb,a,b", bi.DIV_REM_EDGES, ids=[c[0] for c in bi.DIV_REM_EDGES])
def test_div_rem_edge_operands(pkg, orc, name, la, lb, a, b):
    """0; 2^32 - 1 in every limb; a < b; a = b; b one limb; b with a zero top limb; quotient words of 2^32 - 1; an add-back;
    lb > la + 1, where div has no limbs and upstream's mul_biguint places U32AddManyGate operations without addends."""
    c = bi.div_rem_virtual(pkg, la, lb)
    blob, wires = c[0].build(bi.operands(c, a, b))
    _prove(orc, blob, wires)
    q, r = divmod(a, b)
    assert [c[0].value_of(t) for t in c[3]] == bi.digits(q, len(c[3])) and [c[0].value_of(t) for t in c[4]] == bi.digits(r, lb)
    if name == "div_without_limbs":
        assert len(c[3]) == 0 and [r["na"] for r in c[0].rows if r["kind"] == "u32addmany"].count(0) == 1


def test_div_rem_refusals(pkg):
    """b = 0 raises (upstream panics in div_rem); a limb at or above 2^32 carries into the next one, and a quotient with more
    digits than div has limbs raises."""
    c = bi.div_rem_virtual(pkg, 4, 4)
    with pytest.raises(ValueError, match="divides by zero"):
        c[0].build(bi.operands(c, bi.X128, 0))
    T = pkg.translate.CircuitBuilder
    assert T.divrem_values([(1 << 32) + 5, 0], [1], 2, 1) == ([5, 1], [0])
    assert T.divrem_values([5], [0, 0, 7], 0, 3) == ([], [5, 0, 0])
    with pytest.raises(ValueError, match="more digits"):
        T.divrem_values([0, 1 << 32], [1], 2, 1)
    with pytest.raises(ValueError, match="more digits"):
        T.divrem_values([1 << 33], [1 << 32, 1 << 32], 0, 1)


def test_generator_cells_and_seeds(pkg):
    """generators(): the div-rem generator's limbs by the first cell of their copy classes, in creation order beside an
    equality generator; its outputs are derived, so no seed names them; a limb in no gate row is the existing error."""
    c = bi.div_rem_virtual(pkg, 4, 2)
    b = c[0]
    b.is_equal(c[1][0], c[2][0])
    gens = b.generators()
    assert [g[0] for g in gens] == ["biguint_divrem", "equality"]
    assert [len(g) for g in gens[0][1]] == [4, 2, 3, 2]
    for grp, targets in zip(gens[0][1], c[1:]):
        assert list(grp) == [b.cells_of(t)[0] for t in targets]
    seeds = set(b.seed_cells())
    assert all(b.cells_of(t)[0] in seeds for t in c[1] + c[2])
    assert not any(cell in seeds for t in list(c[3]) + list(c[4]) for cell in b.cells_of(t))
    b2 = bi.builder(pkg)
    b2._listed_generator("divrem", (b2.add_virtual_target(),), (b2.one(),), (b2.add_virtual_target(),), (b2.add_virtual_target(),))
    b2.mul(b2.one(), b2.add_virtual_target())
    with pytest.raises(ValueError, match="lies in no gate row"):
        b2.generators()
