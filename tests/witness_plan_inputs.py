"""Hand-built circuits for the witness-plan compilers (test infrastructure; the style of witness_gen_inputs.custom_gate_chain):
each is the smallest shape that reaches one rule of the schedule.  Every function returns (build keywords, seed cells)."""
import numpy as np

from gate_wires import G_ARITHMETIC, G_BASE_SUM, G_CONSTANT, G_U32_ARITHMETIC

G_NOOP = 0
W, R = 234, 80
# op codes of csrc/genops.hpp, as the exported op records carry them
OP_SEED, OP_CONSTANT, OP_ARITHMETIC, OP_BASE_SPLIT, OP_BASE_JOIN, OP_U32_ARITHMETIC = 0, 1, 2, 3, 4, 8

NOOP = (G_NOOP, (), 0, 0)
ARITH = (G_ARITHMETIC, (20,), 3, 2)


def _kw(d, gates, row_gate, row_constants, copies):
    n = 1 << d
    rg = np.zeros(n, dtype=np.uint32)
    rg[:len(row_gate)] = row_gate
    return dict(degree_bits=d, gates=gates, row_gate=rg, row_constants=row_constants,
                copies=np.array(copies, dtype=np.uint32).reshape(-1, 4), num_wires=W, num_routed_wires=R)


def _ones(n, rows):
    rc = np.zeros((2, n), dtype=np.uint64)
    rc[:, list(rows)] = 1
    return rc


def same_level_contenders():
    """Rows 0 and 1: ArithmeticGate operation 0 with every input seeded, the outputs copied together -- both are ready at level
    1, row 0 writes, row 1 compares at level 2.  Row 2's operation reads the class (its first multiplicand) and derives it
    again: ready at level 2, it compares there without waiting."""
    copies = [(0, 3, 1, 3), (0, 3, 2, 3), (0, 3, 2, 0)]
    seeds = [(0, 0), (0, 1), (0, 2), (1, 0), (1, 1), (1, 2), (2, 1), (2, 2)]
    return _kw(2, [NOOP, ARITH], [1, 1, 1], _ones(4, range(3)), copies), seeds


def waiting_op_claims_nothing():
    """Three ops in creation order, all ready at level 1: i = row 0 ArithmeticGate op 0, j = row 1 U32ArithmeticGate op 0,
    k = row 2 ArithmeticGate op 0; i's output is j's output_low, j's output_high is k's output.  i takes, j waits -- and claims
    nothing -- so k takes: levels 1, 2, 1.  "The smallest contender of a slot wins, the others wait" in ONE round would make k
    wait behind j."""
    copies = [(0, 3, 1, 3), (1, 4, 2, 3)]
    seeds = [(r, c) for r in range(3) for c in range(3)]
    return _kw(2, [NOOP, ARITH, (G_U32_ARITHMETIC, (3,), 4, 0)], [1, 2, 1], _ones(4, (0, 2)), copies), seeds


def base_sum_twins():
    """Row 0: the sum and every limb seeded -- both directions are ready at level 1, the split (created first) runs and the
    join is dropped.  Row 1: the limbs seeded, the sum not -- the join runs, the split is dropped when the sum arrives."""
    limbs = 8
    seeds = [(0, c) for c in range(limbs + 1)] + [(1, c) for c in range(1, limbs + 1)]
    return _kw(2, [NOOP, (G_BASE_SUM, (2, limbs), 2, 0)], [1, 1], np.zeros((0, 4), dtype=np.uint64), []), seeds


def hub(per_row=16):
    """One ConstantGate cell copied to the first multiplicand of 63 x 16 = 1008 ArithmeticGate operations at d = 6: one class
    of 1009 cells (the other inputs have no slot and read as zero)."""
    d, n = 6, 64
    rc = _ones(n, range(1, n))
    rc[0, 0], rc[1, 0] = 5, 7
    copies = [(0, 0, r, 4 * i) for r in range(1, n) for i in range(per_row)]
    return _kw(d, [NOOP, (G_CONSTANT, (2,), 1, 2), ARITH], [1] + [2] * (n - 1), rc, copies), [(1, 1)]


HAND_BUILT = dict(same_level_contenders=same_level_contenders, waiting_op_claims_nothing=waiting_op_claims_nothing,
                  base_sum_twins=base_sum_twins, hub=hub)


def op_levels(ops, level_off):
    """{(row or seed index, code, sub): level} of an exported plan."""
    pos = np.arange(len(ops))
    lvl = np.searchsorted(level_off, pos, side="right") - 1
    return {(int(o & 0xFFFFFFFF), int(o >> 32) & 0xFF, int(o >> 40)): int(l) for o, l in zip(ops, lvl)}


def tamper_sigma(blob, row, col, value):
    """A copy of `blob` whose sigma value of cell (row, col) is `value` (the layout device_build_inputs.decompose reads)."""
    b = np.array(blob, dtype=np.uint8, copy=True)
    h = b[:256].view(np.uint32)
    d, Rr, NC, ng = int(h[2]), int(h[4]), int(h[5]), int(h[23])
    n = 1 << d
    off = 256 + 48 * ng + 8 * Rr + 8 * NC * n
    b[off:off + 8 * Rr * n].view(np.uint64)[col * n + row] = value
    return b
