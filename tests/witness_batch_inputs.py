"""Inputs of the batched device witness tests (test infrastructure): members of the BITWISE program that differ from each
other, and the custom-gate chain of witness_gen_inputs.py with the comparison's second operand as a parameter."""
import numpy as np

import witness_gen_inputs as wgi
from gate_wires import (P, comparison_wires, u32_add_many_wires, u32_arithmetic_wires, u32_range_check_wires, u32_subtraction_wires)

F = wgi.F
# witnesses 0 and 2 of BITWISE: 8-bit values, 0 and 0xFF among them; 9 and 11 entries, so 99 members differ pairwise
_A = [0x00, 0xFF, 0xB7, 0x5D, 0x01, 0x80, 0x7F, 0xAA, 0x55]
_C = [0x5D, 0x00, 0xFF, 0xB7, 0x80, 0x01, 0xAA, 0x55, 0x7F, 0x33, 0xCC]
_members = {}


def bitwise_program(k):
    """Member k of a BITWISE batch: the program with its inputs and the outputs 3, 4, 5 recomputed here."""
    a, c = _A[k % len(_A)], _C[k % len(_C)]
    return dict(opcodes=wgi.BITWISE["opcodes"], witness={0: a, 1: wgi.BITWISE["witness"][1], 2: c, 5: (a & c) + (a ^ c)},
                outputs={3: a & c, 4: a ^ c})


def bitwise_member(pkg, k):
    """(blob, seed cells, seed values, expected wires) of member k, from a fresh builder's build(); computed once."""
    if k not in _members:
        prog = bitwise_program(k)
        cb = wgi.translated(pkg, prog)
        blob, wires = cb.build(prog["witness"])
        tm = cb.witness_target_map
        for w, v in prog["outputs"].items():               # (the matrix holds the outputs this module computed)
            r, c = cb.builder.cells_of(tm[w])[0]
            assert int(wires[c, r]) == v
        cells, values = wgi.seeds_from_wires(cb, wires)
        assert values[:4] == [prog["witness"][w] for w in (0, 1, 2, 5)]      # the input seeds come first, in witness order
        wires.setflags(write=False)
        _members[k] = (blob, cells, values, wires)
    return _members[k]


def custom_gate_chain(second=0x80000000):
    """witness_gen_inputs.custom_gate_chain() with seed (3, 1), the comparison's second operand, set to `second`: the rows
    from the comparison on are recomputed with the same gate_wires functions.  Returns (seed values, expected wires, the
    comparison's result)."""
    kw, cells, values, want = wgi.custom_gate_chain()
    r2_x = int(want[8, 2])                                 # the subtraction's second result: the comparison's first operand
    r3 = comparison_wires(r2_x, second, 32, 16)
    r4 = u32_range_check_wires([r3[2], int(want[3, 2])])
    idx = r4[18]
    items = [0, 1, F, P - 1]
    r5 = [idx, items[idx]] + items + [idx & 1, idx >> 1]
    out = want.copy()
    for r, row in ((3, r3), (4, r4), (5, r5)):
        out[:, r] = 0
        out[:len(row), r] = np.array([int(v) % P for v in row], dtype=np.uint64)
    vals = list(values)
    vals[cells.index((3, 1))] = second
    if second == 0x80000000:
        assert np.array_equal(out, want)                   # the parameter's default reproduces the helper's matrix
    return vals, out, r3[2]
