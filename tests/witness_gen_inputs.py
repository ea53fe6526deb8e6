"""Inputs of the device witness-generation tests (test infrastructure): the translated programs with their seeds, and a
hand-built chain of the reference's custom gates whose expected rows come from tests/gate_wires.py."""
import numpy as np

from gate_wires import (G_ARITHMETIC, G_COMPARISON, G_RANDOM_ACCESS, G_U32_ADD_MANY, G_U32_ARITHMETIC, G_U32_RANGE_CHECK, G_U32_SUBTRACTION, P,
                        comparison_wires, u32_add_many_wires, u32_arithmetic_wires, u32_range_check_wires, u32_subtraction_wires)

G_NOOP = 0
W, R = 234, 80
F = 0xFFFFFFFF

FIBONACCI = dict(opcodes=[("assert_zero", [], [(1, 0)], -377)], witness={0: 377})
QUADRATIC = dict(opcodes=[("assert_zero", [(1, 0, 1)], [(P - 1, 2)], 0), ("assert_zero", [], [(3, 0), (2, 1)], -17)],
                 witness={0: 3, 1: 4, 2: 12})
A, C = 0xB7, 0x5D
BITWISE = dict(opcodes=[("range", 0, 8), ("range", 1, 33), ("and", 0, 2, 3, 8), ("xor", 0, 2, 4, 32),
                        ("assert_zero", [], [(1, 3), (1, 4), (P - 1, 5)], 0)],
               witness={0: A, 1: (1 << 33) - 1, 2: C, 5: (A & C) + (A ^ C)}, outputs={3: A & C, 4: A ^ C})


def translated(pkg, prog, num_wires=234, **kw):
    cb = pkg.translate.CircuitBuilderFromAcirToPlonky2(num_wires=num_wires)
    cb.translate_circuit(prog["opcodes"], **kw)
    return cb


def seeds_from_wires(cb, wires):
    """(cells, values): the builder's seed cells with the values build()'s matrix holds there -- the input witnesses and the
    PublicInputGate row's wires."""
    cells = cb.builder.seed_cells()
    return cells, [int(wires[c, r]) for r, c in cells]


def custom_gate_chain():
    """U32Arithmetic(3 ops) -> U32AddMany(2, 2) -> U32Subtraction(2) -> Comparison(32 bits, 16 chunks of 2 bits: the widest
    chunk the library takes) -> U32RangeCheck(2) -> RandomAccess(2 bits), one row each at d = 4, linked by copies; in row 0
    the LAST operation's low word feeds the FIRST operation's multiplicand.  Returns (build keywords, seed cells, seed values,
    expected wires): the expected rows are gate_wires' functions applied in the chain's order."""
    d, n = 4, 16
    gates = [(G_NOOP, (), 0, 0), (G_RANDOM_ACCESS, (2, 1, 0), 3, 0), (G_COMPARISON, (32, 16), 4, 0), (G_U32_ADD_MANY, (2, 2), 4, 0),
             (G_U32_ARITHMETIC, (3,), 4, 0), (G_U32_RANGE_CHECK, (2,), 4, 0), (G_U32_SUBTRACTION, (2,), 4, 0)]
    row_gate = np.zeros(n, dtype=np.uint32)
    row_gate[:6] = [4, 3, 6, 2, 5, 1]
    copies = [(0, 15, 0, 0), (0, 9, 0, 1),                  # row 0: op 2's low word -> op 0's m0, op 1's low word -> op 0's m1
              (0, 3, 1, 0), (0, 16, 1, 1),                  # -> AddMany op 0's addends: op 0's low word, op 2's HIGH word
              (1, 3, 1, 5), (1, 4, 1, 7),                   # AddMany op 0's result and carry -> op 1's addend and carry
              (1, 8, 2, 0), (2, 3, 2, 5), (1, 3, 2, 6), (2, 4, 2, 7),   # -> Subtraction: op 0's x; op 1's x, y, borrow
              (2, 8, 3, 0),                                 # -> Comparison's first operand
              (3, 2, 4, 0), (2, 3, 4, 1),                   # -> RangeCheck's limbs: the comparison's result, a subtraction's
              (4, 18, 5, 0)]                                # the lowest 2-bit limb of the second word -> RandomAccess's index
    seeds = {(0, 2): F, (0, 6): 0, (0, 7): 1, (0, 8): 1, (0, 12): F, (0, 13): F, (0, 14): F,    # op 2: the product's high half is 2^32 - 1
             (1, 2): 1, (1, 6): 1, (2, 1): 2, (2, 2): 0, (3, 1): 0x80000000,
             (5, 2): 0, (5, 3): 1, (5, 4): F, (5, 5): P - 1}
    # ---- expected, in the chain's order ----
    first = u32_arithmetic_wires([0, 0, F], [0, 1, F], [0, 1, F])
    lo1, lo2, hi2 = first[9], first[15], first[16]
    assert (lo1, lo2, hi2) == (1, 0, F) and first[17] == 0             # the zero-inverse branch
    r0 = u32_arithmetic_wires([lo2, 0, F], [lo1, 1, F], [F, 1, F])
    add0 = u32_add_many_wires([[r0[3], hi2], [0, 0]], [1, 0])[0]
    r1 = u32_add_many_wires([[r0[3], hi2], [add0[3], 1]], [1, add0[4]])[0]
    sub0 = u32_subtraction_wires([r1[8], 0], [2, 0], [0, 0])
    r2 = u32_subtraction_wires([r1[8], sub0[3]], [2, r1[3]], [0, sub0[4]])
    r3 = comparison_wires(r2[8], 0x80000000, 32, 16)
    r4 = u32_range_check_wires([r3[2], r2[3]])
    idx = r4[18]
    items = [0, 1, F, P - 1]
    r5 = [idx, items[idx]] + items + [idx & 1, idx >> 1]
    want = np.zeros((W, n), dtype=np.uint64)
    for r, row in enumerate((r0, r1, r2, r3, r4, r5)):
        want[:len(row), r] = np.array([int(v) % P for v in row], dtype=np.uint64)
    for (r, c), v in seeds.items():
        assert int(want[c, r]) == v
    kw = dict(degree_bits=d, gates=gates, row_gate=row_gate, row_constants=np.zeros((0, n), dtype=np.uint64),
              copies=np.array(copies, dtype=np.uint32), num_wires=W, num_routed_wires=R)
    cells = sorted(seeds)
    return kw, cells, [seeds[c] for c in cells], want


def arithmetic_cycle():
    """One ArithmeticGate row whose first operation's output is copied to its own multiplicand."""
    n = 4
    rc = np.zeros((2, n), dtype=np.uint64)
    rc[0, 0] = rc[1, 0] = 1
    kw = dict(degree_bits=2, gates=[(G_NOOP, (), 0, 0), (G_ARITHMETIC, (20,), 3, 2)], row_gate=np.array([1, 0, 0, 0], dtype=np.uint32),
              row_constants=rc, copies=np.array([(0, 3, 0, 0)], dtype=np.uint32), num_wires=W, num_routed_wires=R)
    return kw, [(0, 1), (0, 2)]
