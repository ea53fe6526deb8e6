"""The witness check's model (tests/check_model.py) against the oracle alone, without a device: matrices that satisfy their circuits
are clean, the single-wire corruptions of the reference's gate tests are reported at their rows, and `CircuitBuilder.explain`
names the builder's row for a finding."""
import numpy as np
import pytest

import check_model as cm
import witness_gen_inputs as wgi
from gate_wires import (G_COMPARISON, G_U32_ADD_MANY, G_U32_ARITHMETIC, G_U32_RANGE_CHECK, G_U32_SUBTRACTION, P, comparison_wires,
                        u32_add_many_wires, u32_arithmetic_wires, u32_range_check_wires, u32_subtraction_wires)

W = 234


def _u32s(rng, n):
    return [int(x) for x in rng.integers(0, 1 << 32, size=n, dtype=np.uint64)]


def one_gate_kw(kind, params, degree, rows, d=3):
    """The build keywords and matrix of 2^d rows: `rows` under the gate, NoopGate below (the circuits of the gate-vector tests)."""
    n = 1 << d
    kw = dict(degree_bits=d, gates=[(0, (), 0, 0), (kind, tuple(params), degree, 0)], row_gate=[1] * len(rows) + [0] * (n - len(rows)),
              row_constants=np.zeros((0, n), dtype=np.uint64), copies=np.zeros((0, 4), dtype=np.uint32), num_wires=W, num_routed_wires=80)
    wires = np.zeros((W, n), dtype=np.uint64)
    for r, w in enumerate(rows):
        wires[:len(w), r] = np.array([int(v) % P for v in w], dtype=np.uint64)
    return kw, wires


def gate_vector_negatives():
    """(name, kind, params, rows, failing row): the negatives of tests/test_gpu_gate_vectors.py, restated."""
    out = []
    rng = np.random.default_rng(2)
    good = u32_arithmetic_wires(_u32s(rng, 3), _u32s(rng, 3), _u32s(rng, 3))
    bad = u32_arithmetic_wires([0] * 3, [0] * 3, [0xFFFFFFFF00000001] * 3)
    out.append(("u32arith canonicity", G_U32_ARITHMETIC, [3], [good, bad, good], 1))
    for idx in (18, 3):                                  # a wrong limb, a wrong product
        w = list(good)
        w[idx] = (w[idx] + 1) % P
        out.append(("u32arith wire %d" % idx, G_U32_ARITHMETIC, [3], [good, w], 1))
    for na, ops in ((10, 3), (3, 9), (16, 4), (2, 5)):
        rng = np.random.default_rng(na)
        rows = []
        for _ in range(2):
            addends = [_u32s(rng, na) for _ in range(ops)]
            rows.append(u32_add_many_wires(addends, _u32s(rng, ops) if na < 16 else [0] * ops)[0])
        bad = list(rows[0])
        bad[na + 1] = (bad[na + 1] + 1) % P              # wrong result
        out.append(("u32addmany %d x %d" % (na, ops), G_U32_ADD_MANY, [na, ops], [rows[1], bad], 1))
    for ops in (3, 11):
        rng = np.random.default_rng(3)
        rows = [u32_subtraction_wires(_u32s(rng, ops), _u32s(rng, ops), [int(b) for b in rng.integers(0, 2, size=ops)]) for _ in range(2)]
        bad = list(rows[0])
        bad[4] = 2                                       # output borrow must be a bit
        out.append(("u32sub %d" % ops, G_U32_SUBTRACTION, [ops], [rows[1], bad], 1))
    rng = np.random.default_rng(4)
    rows = [u32_range_check_wires(_u32s(rng, 8)) for _ in range(2)]
    out.append(("u32range 2^32", G_U32_RANGE_CHECK, [8], [rows[0], u32_range_check_wires([1 << 32] + [0] * 7)], 1))
    w = list(rows[1])
    w[8], w[9] = (w[8] + 4) % P, (w[9] - 1) % P          # a limb outside {0..3} whose recomposition still matches
    out.append(("u32range limb", G_U32_RANGE_CHECK, [8], [w], 0))
    a, b = 0x12345678, 0x23456789
    bad = comparison_wires(a, b, 32, 16)
    bad[2] ^= 1                                          # wrong result bool
    out.append(("comparison", G_COMPARISON, [32, 16], [comparison_wires(a, b, 32, 16), bad], 1))
    return out


def test_custom_gate_chain_is_clean(orc):
    kw, _, _, want = wgi.custom_gate_chain()
    m = cm.Model(orc, kw, want)
    assert m.ok and m.gate_rows_failed == 0 and not m.nonconstant and m.first_gate is None
    assert len(m.classes) >= 10                          # (the chain's copies form classes the model really checks)


@pytest.mark.parametrize("name", ["FIBONACCI", "QUADRATIC", "BITWISE"])
def test_translated_programs_are_clean(pkg, orc, name):
    prog = getattr(wgi, name)
    with cm.recorded_build(pkg) as seen:
        cb = wgi.translated(pkg, prog)
        _, wires = cb.build(prog["witness"])
    assert len(seen) == 1
    m = cm.Model(orc, seen[0], wires)
    assert m.ok, (m.first_gate, m.nonconstant)
    assert any(m.classes)


@pytest.mark.parametrize("case", gate_vector_negatives(), ids=lambda c: c[0])
def test_gate_vector_negatives_are_reported_at_their_row(orc, case):
    _, kind, params, rows, bad_row = case
    kw, wires = one_gate_kw(kind, params, 4, rows)
    m = cm.Model(orc, kw, wires)
    assert m.gate_rows_failed == 1 and m.first_gate[0] == bad_row and m.first_gate[2] == kind
    assert [r for r in range(8) if m.row_status[r] != cm.NONE] == [bad_row]
    # the same rows without the corruption are clean: the finding is the corruption's
    kw, wires = one_gate_kw(kind, params, 4, [rows[0]] if bad_row else [])
    assert cm.Model(orc, kw, wires).ok


def _report_from_model(pkg, m):
    """A WitnessReport with the model's first gate finding (what the device would have filled in)."""
    raw = pkg.prover._WitnessReport()
    raw.gate_rows_failed = m.gate_rows_failed
    raw.gate_row, raw.gate_index, raw.gate_kind, raw.constraint, raw.constraint_value = m.first_gate
    return pkg.WitnessReport(raw)


def test_explain_names_the_builder_row_of_a_corrupted_product(pkg, orc):
    prog = wgi.QUADRATIC
    with cm.recorded_build(pkg) as seen:
        cb = wgi.translated(pkg, prog)
        _, wires = cb.build(prog["witness"])
    b = cb.builder
    t0, t1 = (b.find(cb.witness_target_map[w]) for w in (0, 1))
    found = [(g["row"], k, op) for g in b.rows if g["kind"] == "arith" and g["c"][0] for k, op in enumerate(g["ops"])
             if {b.find(op[0]), b.find(op[1])} == {t0, t1}]
    assert len(found) == 1                               # the product w0 * w1
    row, k, op = found[0]
    m = cm.Model(orc, seen[0], cm.corrupt(wires, row, 4 * k + 3))
    assert m.gate_rows_failed == 1 and m.first_gate[:4] == (row, m.first_gate[1], 3, k)
    text = b.explain(_report_from_model(pkg, m))
    assert "row %d is a arith row" % row in text and "operation %d on targets %s" % (k, tuple(op)) in text
    assert "ACIR opcode 0" in cb.explain(_report_from_model(pkg, m))
    # a clean report
    assert b.explain(pkg.WitnessReport(pkg.prover._WitnessReport())) == "the witness satisfies the circuit"
    # a copy finding is worded through the cells' classes
    raw = pkg.prover._WitnessReport()
    cells = b.cells_of(op[3])
    raw.copy_cells_failed = 1
    raw.copy_cell[0], raw.copy_cell[1] = cells[0]
    raw.copy_partner[0], raw.copy_partner[1] = cells[-1]
    text = b.explain(pkg.WitnessReport(raw))
    assert "class of %d cells from %s" % (len(cells), cells[0]) in text and "copy: cell (%d, %d)" % cells[0] in text
