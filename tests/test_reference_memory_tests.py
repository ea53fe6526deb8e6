"""The reference's memory-opcode unit tests, one to one: plonky2-backend/src/circuit_translation/tests/
test_memory_operations.rs (six tests, one of them #[ignore]d), the circuits restated as data in tests/memory_ops_inputs.py.
Every reference test is "build circuit -> real prove -> real verify"; so is every test here: restated translator
(translate.py: MemoryOperationsTranslator, is_equal, random_access) -> p2gpu_build_blob -> prove -> verify on the CPU oracle,
public inputs as expected.  tests/test_gpu_memory_ops.py runs the same circuits on the MI355X."""
import pytest

import memory_ops_inputs as moi
from memory_ops_inputs import P


def _pi_tail(pis):
    return b"".join(int(v).to_bytes(8, "little") for v in pis)


def _prove(orc, blob, wires, pis):
    oc = orc.OracleCircuit(blob)
    try:
        proof, _ = oc.prove(wires, public_inputs=pis)
        assert proof.endswith(_pi_tail(pis)) and oc.verify(proof)
    finally:
        oc.close()


@pytest.mark.parametrize("name,prog,witness,expected", moi.CASES, ids=[c[0] for c in moi.CASES])
def test_reference_memory_test_on_the_oracle(pkg, orc, name, prog, witness, expected):
    """:10-36 the read, :39-79 the basic write, :82-117 the block of length 3; beyond the reference: a block of length 1 (no
    RandomAccess row), one of length 5 (bits = 3), a write followed by reads of the written position and of another one."""
    cb = moi.translated(pkg, prog)
    blob, wires = cb.build(witness)
    assert cb.public_inputs() == expected
    kinds = [r["kind"] for r in cb.builder.rows]
    assert ("ra" in kinds) == (name != "block_of_length_1")
    if name == "block_of_length_5":
        assert [r["bits"] for r in cb.builder.rows if r["kind"] == "ra"] == [3]
    if name == "write_then_read_written_and_other":
        assert {w: cb.witness_value(w) for w in moi.WRITE_READ_RESULTS} == moi.WRITE_READ_RESULTS
    _prove(orc, blob, wires, expected)


@pytest.mark.parametrize("x,y,equal", [(0, 0, 1), (1, 0, 0)], ids=["positive", "negative"])
def test_plonky2_is_equal(pkg, orc, x, y, equal):
    """:388-407 plonky2_is_equal_test_positive, :409-429 _negative: is_equal.target is assigned as well."""
    b, tx, ty, te = moi.is_equal_circuit(pkg)
    blob, wires = b.build({tx: x, ty: y, te: equal})
    assert b.value_of(te) == equal
    _prove(orc, blob, wires, [])
    with pytest.raises(ValueError):
        moi.is_equal_circuit(pkg)[0].build({tx: x, ty: y, te: 1 - equal})


def test_is_equal_generator_cells(pkg):
    """generators(): one equality generator, its four cells in ArithmeticGate rows, `inv` in exactly one cell."""
    b, tx, ty, te = moi.is_equal_circuit(pkg)
    (kind, cl), = b.generators()
    assert kind == "equality" and len(cl) == 4
    (ev,) = [e for e in b.events if e.kind == "equal"]
    equal, inv = ev.outs
    assert equal == te and b.cells_of(inv) == [cl[3]] and cl[2] == b.cells_of(te)[0]
    assert all(b.rows[r]["kind"] == "arith" for r, _ in cl)


def test_brute_force_range_checks_up_to_8(pkg, orc):
    """:123-179 test_brute_force_range_checks_up_to_17 (#[ignore]d upstream), cut to the bounds 0 .. 8: every valid pair
    proves and verifies, every invalid pair is refused."""
    for bound in range(9):
        for value in range(9):
            b, t = moi.less_or_equal_circuit(pkg, bound)
            if value <= bound:
                blob, wires = b.build({t: value})
                _prove(orc, blob, wires, [value])
            else:
                with pytest.raises(ValueError):
                    b.build({t: value})


def test_out_of_range_index_is_refused(pkg):
    """Position 3 of a block of length 3 is a padded one: the <= check refuses it."""
    with pytest.raises(ValueError):
        moi.translated(pkg, moi.LENGTH_3).build({0: 5, 1: 10, 2: 11, 3: 3})
    with pytest.raises(ValueError):
        moi.translated(pkg, moi.WRITE_READ).build({0: 20, 1: 21, 2: 22, 3: 3, 4: 99, 5: 2, 7: 1})


def test_wrong_claimed_read_value_is_refused(pkg):
    with pytest.raises(ValueError):
        moi.translated(pkg, moi.WRITE_READ).build({0: 20, 1: 21, 2: 22, 3: 2, 4: 99, 5: 2, 7: 1, 8: 22})
    with pytest.raises(ValueError):
        moi.translated(pkg, moi.READ).build({0: 0, 1: 4, 2: 1, 3: 4})      # x[0] == x[y] fails


def test_refused_memory_operations(pkg):
    """Where the reference would unwrap a None (memory_translator.rs:33, 42)."""
    def tr(op):
        pkg.translate.CircuitBuilderFromAcirToPlonky2().translate_circuit([moi.init(0, [0, 1]), op], public_parameters=[0, 1])
    with pytest.raises(ValueError, match="the operation is not a constant"):
        tr(("memory_op", 0, ([], [(1, 5)], 0), 2, 3))
    with pytest.raises(ValueError, match="the index is not a single witness"):
        tr(("memory_op", 0, 0, ([], [(2, 2)], 0), 3))
    with pytest.raises(ValueError, match="the value is not a single witness"):
        tr(("memory_op", 0, 0, 2, ([], [(1, 3)], 1)))
    with pytest.raises(ValueError, match="unknown memory operation code"):
        tr(("memory_op", 0, 2, 2, 3))
