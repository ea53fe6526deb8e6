"""MemoryInit / MemoryOp from a serialised ACIR program to the translator (acir.to_translator_opcodes(..., memory=True)): the
reference's basic-write program (tests/test_memory_operations.rs:278-361) written as `Program` bytes with the module's own
inverse functions, read back, and translated to the same circuit as its tuple form (tests/memory_ops_inputs.py)."""
import numpy as np
import pytest

import memory_ops_inputs as moi
from memory_ops_inputs import P


def expr(lin=(), q_c=0):
    return {"mul_terms": [], "linear_combinations": [tuple(t) for t in lin], "q_c": q_c % P}


def mem_op(block, operation, index, value, predicate=None):
    return ("MemoryOp", {"block_id": block, "op": {"operation": expr(q_c=operation), "index": expr(lin=[(1, index)]), "value": expr(lin=[(1, value)])},
                         "predicate": predicate})


def write_program():
    ops = [("MemoryInit", {"block_id": 0, "init": [0, 1], "block_type": "Memory"}),
           mem_op(0, 1, 2, 3, predicate=expr(q_c=1)),          # (a predicate is read and dropped, as the reference drops it)
           ("AssertZero", expr(lin=[(P - 1, 4)])),
           mem_op(0, 0, 4, 5),
           ("AssertZero", expr(lin=[(1, 5)], q_c=-1)),
           ("AssertZero", expr(lin=[(P - 1, 6)], q_c=1)),
           mem_op(0, 0, 6, 7),
           ("AssertZero", expr(lin=[(P - 1, 7)], q_c=11))]
    return {"current_witness_index": 7, "opcodes": ops, "public_parameters": [0, 1, 2, 3]}


def test_memory_program_round_trips_to_the_tuple_form(pkg):
    ac = pkg.acir
    prog = ac.deserialize_program(ac.serialize_program([write_program()]))
    circuit = prog["functions"][0]
    assert [k for k, _ in circuit["opcodes"]] == [k for k, _ in write_program()["opcodes"]]
    ops = ac.to_translator_opcodes(circuit, memory=True)
    want = [tuple(list(o) if isinstance(o, list) else o for o in op) for op in moi.WRITE["ops"]]
    assert [(op[0],) + tuple(op[1:]) for op in ops if op[0].startswith("memory")] == [op for op in want if op[0].startswith("memory")]
    cb = pkg.translate.CircuitBuilderFromAcirToPlonky2()
    cb.translate_circuit(ops, public_parameters=circuit["public_parameters"])
    assert np.array_equal(cb.blob(), moi.translated(pkg, moi.WRITE).blob())
    witness = moi.CASES[1][2]
    blob, wires = cb.build(witness)
    blob2, wires2 = moi.translated(pkg, moi.WRITE).build(witness)
    assert np.array_equal(wires, wires2) and cb.public_inputs() == moi.CASES[1][3]


def test_the_default_still_refuses_memory_opcodes(pkg):
    ac = pkg.acir
    circuit = ac.deserialize_program(ac.serialize_program([write_program()]))["functions"][0]
    with pytest.raises(NotImplementedError, match="MemoryInit"):
        ac.to_translator_opcodes(circuit)
    with pytest.raises(NotImplementedError, match="MemoryOp"):
        ac.to_translator_opcodes({"opcodes": circuit["opcodes"][1:]})


def test_operands_that_are_no_witness_reach_the_translator_as_expressions(pkg):
    """An index that is no single witness and an operation that is no constant stay expressions; the translator refuses them."""
    ac = pkg.acir
    bad_index = ("MemoryOp", {"block_id": 0, "op": {"operation": expr(q_c=0), "index": expr(lin=[(2, 2)]), "value": expr(lin=[(1, 3)])}, "predicate": None})
    bad_op = ("MemoryOp", {"block_id": 0, "op": {"operation": expr(lin=[(1, 5)]), "index": expr(lin=[(1, 2)]), "value": expr(lin=[(1, 3)])}, "predicate": None})
    init = ("MemoryInit", {"block_id": 0, "init": [0, 1], "block_type": "Memory"})
    for bad, words in ((bad_index, "the index is not a single witness"), (bad_op, "the operation is not a constant")):
        circuit = ac.deserialize_program(ac.serialize_program([{"opcodes": [init, bad]}]))["functions"][0]
        ops = ac.to_translator_opcodes(circuit, memory=True)
        with pytest.raises(ValueError, match=words):
            pkg.translate.CircuitBuilderFromAcirToPlonky2().translate_circuit(ops)
