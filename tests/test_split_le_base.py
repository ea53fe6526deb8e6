"""`split_le_base` and `add_many` of builder.py, and the split gadgets of split_nonnative.rs above them, on the CPU oracle: one
BaseSumGate<4>{16} row per split, degree 4, whose limbs are the base-4 digits Python computes; a value of 2^32 or more has no
sixteen base-4 limbs."""
import pytest

import curve_inputs as ci

WORDS = [0, 3, 2**32 - 1, 0xAAAAAAAA]


def base4(v, count=16):
    return [(v >> (2 * i)) & 3 for i in range(count)]


def test_sixteen_base_four_limbs_of_edge_words(pkg, orc):
    b = ci.builder(pkg)
    xs = [b.add_virtual_target() for _ in WORDS]
    limbs = [b.split_le_base(x, 16, 4) for x in xs]
    blob, wires = b.build(dict(zip(xs, WORDS)))
    rows = [r for r in b.rows if r["kind"] == "basesum"]
    assert len(rows) == len(WORDS) and all(r["base"] == 4 and r["L"] == 16 for r in rows)
    for word, ls in zip(WORDS, limbs):
        assert [b.value_of(t) for t in ls] == base4(word)
    assert base4(0xAAAAAAAA) == [2] * 16 and base4(2**32 - 1) == [3] * 16
    # the gate: id and degree as the row kind states them, the declaration (G_BASE_SUM, (base, L, 0, 0), base, 0)
    degree, ident, decl = pkg.translate.ROW_KINDS["basesum"].spec(b, 4, 16)
    assert (degree, ident, decl) == (4, "BaseSumGate { num_limbs: 16 } + Base: 4", (pkg.translate.G_BASE_SUM, (4, 16, 0, 0), 4, 0))
    assert pkg.translate.ROW_KINDS["basesum"].spec(b, 2, 63)[:2] == (2, "BaseSumGate { num_limbs: 63 } + Base: 2")
    oc = orc.OracleCircuit(blob)
    proof, _ = oc.prove(wires, public_inputs=[])
    assert oc.verify(proof)
    oc.close()
    # the seeds of the device witness are the four words: the limbs are derived, the row's sum lies in its word's class
    assert len(b.seed_cells()) == len(WORDS) + (pkg.translate.NUM_WIRES - 4)


@pytest.mark.parametrize("value", [2**32, 2**32 + 5, 2**63])
def test_a_value_of_two_to_the_32_or_more_is_unsatisfiable(pkg, value):
    b = ci.builder(pkg)
    x = b.add_virtual_target()
    b.split_le_base(x, 16, 4)
    with pytest.raises(ValueError, match="does not fit"):
        b.build({x: value})


def test_base_two_rows_are_what_they_were(pkg):
    """split_le still places BaseSumGate<2>{63} rows and its bits are the bits"""
    b = ci.builder(pkg)
    x = b.add_virtual_target()
    bits = b.split_le(x, 40)
    b.build({x: 0xA5_DEADBEEF})
    assert [b.value_of(t) for t in bits] == [(0xA5_DEADBEEF >> i) & 1 for i in range(40)]
    assert [(r["base"], r["L"]) for r in b.rows if r["kind"] == "basesum"] == [(2, 63)]


def test_add_many_and_the_split_gadgets(pkg):
    b = ci.builder(pkg)
    xs = [b.add_virtual_target() for _ in range(4)]
    total = b.add_many(xs)
    assert b.add_many([]) == b.zero()
    v = b.constant_nonnative(0x1234_5678_9ABC_DEF0_0FED_CBA9, ci.SCALAR)
    two_bit = b.split_nonnative_to_2_bit_limbs(v, ci.SCALAR)
    four_bit = b.split_nonnative_to_4_bit_limbs(v, ci.SCALAR)
    b.build(dict(zip(xs, (5, ci.GOLDILOCKS - 1, 7, 1 << 40))))
    assert b.value_of(total) == (5 + ci.GOLDILOCKS - 1 + 7 + (1 << 40)) % ci.GOLDILOCKS
    assert len(two_bit) == 16 * 3 and len(four_bit) == 8 * 3
    assert [b.value_of(t) for t in two_bit] == base4(0x1234_5678_9ABC_DEF0_0FED_CBA9, 48)
    assert [b.value_of(t) for t in four_bit] == [(0x1234_5678_9ABC_DEF0_0FED_CBA9 >> (4 * i)) & 15 for i in range(24)]
