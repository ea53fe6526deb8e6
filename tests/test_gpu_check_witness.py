"""The witness check on the MI355X (p2gpu_check_witness / _dev / p2gpu_check_seeds through CircuitData.check_witness,
WitnessPlan.check / check_batch) against tests/check_model.py: the expected report from the build keywords and the oracle's gate
evaluator.  Gates, `row_status` and canonicity are compared exactly, copies by the model's order-free promises (a)-(e).  Where a
circuit has no build keywords (the synthetic blobs) the verdict is compared with the prover's own."""
import ctypes

import numpy as np
import pytest

import check_model as cm
import witness_batch_inputs as wbi
import witness_gen_inputs as wgi

pytestmark = pytest.mark.gpu
P = cm.P
E_UNSATISFIED = -5
G_PUBLIC_INPUT, G_BASE_SUM, G_POSEIDON, G_U32_SUBTRACTION = 2, 4, 6, 9


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


@pytest.fixture(scope="module")
def chain(pkg, gpu):
    """(build keywords, the satisfying matrix, the handle) of the custom-gate chain, d = 4: all five custom gates and RandomAccess."""
    kw, _, _, want = wgi.custom_gate_chain()
    cd = pkg.CircuitData(pkg.build_blob(**kw))
    yield kw, want, cd
    cd.close()


def _checked(orc, cd, kw, wires, public_inputs=()):
    """The device's report of `wires`, already compared with the model's; (report, model, flagged cells)."""
    rep = cd.check_witness(wires, public_inputs, details=True)
    m = cm.Model(orc, kw, wires, public_inputs)
    flagged = m.assert_report(rep)
    assert (rep.message == "") == rep.ok
    return rep, m, flagged


# ---- the custom-gate chain ---------------------------------------------------------------------------------------------
def test_chain_clean(orc, chain):
    kw, want, cd = chain
    rep, m, flagged = _checked(orc, cd, kw, want)
    assert rep.ok and m.ok and not flagged and rep.gate_rows_failed == rep.copy_cells_failed == rep.noncanonical_cells == 0
    assert (rep.row_status == cm.NONE).all() and not rep.cell_flags.any()
    assert cd.check_witness(want).row_status is None        # (details are brought back only when asked for)


# per row of the chain: an input wire, a limb (an index bit of the RandomAccess row), an output
CHAIN_CELLS = {0: (2, 18, 3), 1: (2, 10, 3), 2: (1, 10, 3), 3: (1, 4, 2), 4: (0, 2, 3), 5: (0, 6, 1)}


@pytest.mark.parametrize("row", sorted(CHAIN_CELLS))
def test_chain_one_corruption_per_row(pkg, orc, chain, row):
    kw, want, cd = chain
    for col in CHAIN_CELLS[row]:
        rep, m, _ = _checked(orc, cd, kw, cm.corrupt(want, row, col))
        assert not rep.ok and rep.gate_rows_failed == 1 and rep.first_gate[0] == row, (row, col, rep)
        assert rep.first_gate[2] == kw["gates"][int(kw["row_gate"][row])][0]
        assert "row %d (%s, gate " % (row, pkg.prover.GATE_KIND_NAMES[rep.first_gate[2]]) in rep.message


def test_chain_u32_arithmetic_canonicity_case(orc, chain):
    """arithmetic_u32.rs:584: the addend 0xFFFFFFFF00000001 -- output_high = 2^32 - 1 with a non-zero output_low -- in the
    chain's U32ArithmeticGate row: its first constraint is the one that rejects the encoding."""
    from gate_wires import u32_arithmetic_wires

    kw, want, cd = chain
    w = np.array(want, copy=True)
    bad = u32_arithmetic_wires([0] * 3, [0] * 3, [0xFFFFFFFF00000001] * 3)
    w[:, 0] = 0
    w[:len(bad), 0] = np.array([int(v) % P for v in bad], dtype=np.uint64)
    rep, m, _ = _checked(orc, cd, kw, w)
    assert rep.first_gate[0] == 0 and rep.first_gate[3] == 0 and rep.first_gate[4] == P - 1     # (hi_not_max * lo = -1 * 1)


def test_chain_one_broken_copy_per_pair(orc, chain):
    kw, want, cd = chain
    for ra, ca, rb, cb in [tuple(int(x) for x in c) for c in kw["copies"]]:
        rep, m, flagged = _checked(orc, cd, kw, cm.corrupt(want, rb, cb, delta=5))
        cl = m.classes[m.class_of[(rb, cb)]]
        assert (ra, ca) in cl and m.nonconstant == [m.class_of[(rb, cb)]]
        assert len(flagged) == 2 and (rb, cb) in flagged          # (e): the corrupted cell and the cell sigma maps onto it
        if len(cl) == 2:
            assert sorted(flagged) == cl                          # (d)
        assert "copy (" in rep.message or rep.gate_rows_failed    # (gates are worded before copies)


def test_chain_noncanonical_words(orc, chain):
    """p and 2^64 - 1 in a routed and in a non-routed column: counted, the lowest key named, and the gate and copy verdicts
    are those of the matrix reduced once -- p in a cell that holds 0 changes neither."""
    kw, want, cd = chain
    assert int(want[2, 2]) == 0 and int(want[200, 7]) == 0
    w = np.array(want, copy=True)
    w[2, 2] = P                                   # routed, row 2 (a subtraction's borrow in): reduced, the matrix is `want`
    w[200, 7] = P                                 # not routed, a NoopGate row
    rep, m, flagged = _checked(orc, cd, kw, w)
    assert rep.noncanonical_cells == 2 and rep.first_noncanonical == (2, 2) and rep.gate_rows_failed == 0 and not flagged
    assert not rep.ok and "(2, 2)" in rep.message and "canonical" in rep.message
    w[100, 0] = (1 << 64) - 1                     # not routed: a limb of row 0, reduced 2^32 - 2: the limb's range check fails
    w[9, 0] = (1 << 64) - 1                       # routed and copied to (0, 1): reduced it differs from its class
    rep, m, flagged = _checked(orc, cd, kw, w)
    assert rep.noncanonical_cells == 4 and rep.first_noncanonical == (2, 2)
    assert rep.first_gate[0] == 0 and flagged and m.nonconstant


# ---- far fewer rows than a wave ----------------------------------------------------------------------------------------
def test_arithmetic_cycle(pkg, orc, gpu):
    kw, _ = wgi.arithmetic_cycle()
    cd = pkg.CircuitData(pkg.build_blob(**kw))
    try:
        w = np.zeros((wgi.W, 4), dtype=np.uint64)
        w[0, 0], w[1, 0], w[2, 0], w[3, 0] = 5, 1, 0, 5          # out = m0 * m1 + addend, copied back to m0
        rep, _, _ = _checked(orc, cd, kw, w)
        assert rep.ok
        rep, m, flagged = _checked(orc, cd, kw, cm.corrupt(w, 0, 3))
        assert rep.first_gate[:4] == (0, 1, 3, 0) and sorted(flagged) == [(0, 0), (0, 3)]
        rep, _, _ = _checked(orc, cd, kw, cm.corrupt(w, 0, 4 * 19 + 3))      # the last operation of the row
        assert rep.first_gate[:4] == (0, 1, 3, 19) and rep.copy_cells_failed == 0
    finally:
        cd.close()


# ---- a translated program with public inputs: a PoseidonGate row and a PublicInputGate row -------------------------------
def _basic_div():
    x, y, inv, q, ret = range(5)
    half = pow(2, P - 2, P)
    return dict(opcodes=[("assert_zero", [(1, x, inv)], [], P - 1), ("assert_zero", [(1, y, inv)], [(P - 1, q)], 0),
                         ("assert_zero", [], [(1, q), (P - 1, ret)], 0)],
                public=(y,), private=(x,), witness={x: 2, y: 1, inv: half, q: half, ret: half})


@pytest.mark.parametrize("num_wires", [234, 135])
def test_translated_program_with_public_inputs(pkg, orc, gpu, num_wires):
    prog = _basic_div()
    with cm.recorded_build(pkg) as seen:
        cb = wgi.translated(pkg, prog, num_wires=num_wires, public_parameters=prog["public"], private_parameters=prog["private"])
        blob, wires = cb.build(prog["witness"])
    kw, pis = seen[0], cb.public_inputs()
    kinds = [kw["gates"][int(g)][0] for g in kw["row_gate"]]
    pose_row, pi_row = kinds.index(G_POSEIDON), kinds.index(G_PUBLIC_INPUT)
    assert pis == [1] and pi_row == cb.builder.pi_row
    cd = pkg.CircuitData(blob)
    try:
        rep, _, _ = _checked(orc, cd, kw, wires, pis)
        assert rep.ok
        cd.verify(cd.prove(wires, pis).to_bytes())
        rep, _, _ = _checked(orc, cd, kw, wires, [2])                  # a wrong public input value: the hash differs
        assert rep.gate_rows_failed == 1 and rep.first_gate[:4] == (pi_row, rep.first_gate[1], G_PUBLIC_INPUT, 0) and rep.copy_cells_failed == 0
        assert "PublicInputGate" in rep.message
        rep, _, _ = _checked(orc, cd, kw, cm.corrupt(wires, pose_row, 29 + 14), pis)      # an S-box input of the second full round
        assert rep.gate_rows_failed == 1 and rep.first_gate[0] == pose_row and rep.first_gate[2] == G_POSEIDON and rep.copy_cells_failed == 0
        assert "PoseidonGate" in rep.message and "row %d " % pose_row in cb.explain(rep) and "poseidon" in cb.explain(rep)
        with pytest.raises(pkg.P2GpuError) as e:                          # the public inputs' count is checked first
            cd.check_witness(wires, [])
        assert e.value.code == -7
    finally:
        cd.close()


# ---- every gate kind the workload generator emits, two blocks of rows: the checker's verdict is the prover's --------------
@pytest.mark.parametrize("mix,npi", [("ecdsa", 0), ("sha", 4)])
def test_verdict_equals_the_provers(pkg, gpu, mix, npi):
    out = pkg.make_circuit(9, mix, seed=3, num_public_inputs=npi)
    blob, wires, pis = out[0], out[1], ([int(x) for x in out[2]] if npi else [])
    cd = pkg.CircuitData(blob)
    try:
        assert cd.check_witness(wires, pis).ok
        cd.verify(cd.prove(wires, pis).to_bytes())
        rng = np.random.default_rng(20 + npi)
        verdicts = []
        for _ in range(16):
            col, row = int(rng.integers(0, wires.shape[0])), int(rng.integers(0, wires.shape[1]))
            w = cm.corrupt(wires, row, col, delta=int(rng.integers(1, P, dtype=np.uint64)))
            rep = cd.check_witness(w, pis)
            try:
                proof, code = cd.prove(w, pis).to_bytes(), 0
            except pkg.P2GpuError as e:
                proof, code = None, e.code
            assert code in (0, E_UNSATISFIED), code
            if rep.ok:
                assert code == 0, (col, row)
                cd.verify(proof)
            else:
                assert code == E_UNSATISFIED, (col, row, rep)
            verdicts.append(rep.ok)
        print("verdicts:", verdicts)
    finally:
        cd.close()


# ---- the witness plan's output, lone and batched ----------------------------------------------------------------------------
def test_plan_check_on_bitwise(pkg, gpu):
    blob, cells, values, wires = wbi.bitwise_member(pkg, 0)
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    try:
        rep = plan.check(values, details=True)
        assert rep.ok and (rep.row_status == cm.NONE).all() and not rep.cell_flags.any()
        v = list(values)
        v[0] = 256                                       # not 8 bits: the level walk itself refuses, as generate() does
        with pytest.raises(pkg.P2GpuError) as e:
            plan.check(v)
        assert e.value.code == E_UNSATISFIED
    finally:
        plan.close()
        cd.close()


def test_check_batch_isolation(pkg, gpu):
    """Three value sets, the middle one with an input of 256 under an 8-bit range check.  The walk refuses that member at a limb of
    the BaseSum row (the ninth bit, which the circuit ties to the constant zero) and its matrix then holds what the row's own
    generator derives: a BaseSum row that adds up, with a limb that differs from the zero it is copied from.  The report names that
    row through the broken copy; the other members are clean and their matrices the lone call's."""
    members = [wbi.bitwise_member(pkg, k) for k in range(3)]
    blob, cells = members[0][0], members[0][1]
    values = [list(m[2]) for m in members]
    values[1][0] = 256
    cb = wgi.translated(pkg, wbi.bitwise_program(0))
    cb.blob()
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    try:
        _, _, bad = plan.generate_batch(values)
        reports, got, status = plan.check_batch(values, details=True)
        assert status == [0, E_UNSATISFIED, 0] and bad[0] is None and bad[2] is None
        assert reports[0].ok and reports[2].ok and not reports[1].ok
        print("middle member:", reports[1], "the walk's contradiction:", bad[1])
        row, col = bad[1]
        assert cb.builder.row_of(row)[0] == "basesum"
        assert reports[1].cell_flags[col, row] == 1 and reports[1].copy_cells_failed == int(reports[1].cell_flags.sum()) >= 2
        cell, partner, vals = reports[1].first_copy
        assert (row, col) in (cell, partner) and vals[0] != vals[1]
        assert reports[1].message.startswith("witness 1 of the batch: ") and "(%d, %d)" % (row, col) in reports[1].message
        assert "constant 0" in cb.builder.explain(reports[1])
        for b in (0, 2):
            assert np.array_equal(got[b].cpu().numpy().view(np.uint64), members[b][3])
            assert np.array_equal(plan.generate(values[b]).cpu().numpy().view(np.uint64), members[b][3])
    finally:
        plan.close()
        cd.close()


# ---- the C ABI ----------------------------------------------------------------------------------------------------------------
def test_host_and_device_forms_agree(pkg, chain):
    import torch

    kw, want, cd = chain
    lib = pkg.load_library()
    w = np.ascontiguousarray(cm.corrupt(cm.corrupt(want, 2, 3), 4, 3))
    dev = torch.from_numpy(w.view(np.int64)).to(f"cuda:{cd.device_index()}")
    reps = (pkg.prover._WitnessReport * 2)()
    n, R = cd.degree, cd.num_routed_wires
    st, fl = np.zeros((2, n), dtype=np.uint16), np.zeros((2, R, n), dtype=np.uint8)
    rc0 = lib.p2gpu_check_witness(cd._h, w.ctypes.data, None, 0, ctypes.byref(reps[0]), st[0].ctypes.data, fl[0].ctypes.data)
    msg0 = lib.p2gpu_last_error().decode()
    rc1 = lib.p2gpu_check_witness_dev(cd._h, ctypes.c_void_p(dev.data_ptr()), 1, None, 0, ctypes.byref(reps[1]), st[1].ctypes.data, fl[1].ctypes.data)
    assert rc0 == rc1 == E_UNSATISFIED and msg0 == lib.p2gpu_last_error().decode()
    assert bytes(reps[0]) == bytes(reps[1]) and np.array_equal(st[0], st[1]) and np.array_equal(fl[0], fl[1])
    # the error string of a failing call: the row and the gate's name
    assert msg0.startswith("row 2 (U32SubtractionGate, gate 6): constraint ") and "0x" in msg0
    # a batch of two device matrices, the second clean: the lowest failing witness is worded, behind its number
    both = torch.stack([dev, torch.from_numpy(np.ascontiguousarray(want).view(np.int64)).to(dev.device)]).contiguous()
    reports = cd.check_witness_batch(both)
    assert not reports[0].ok and reports[1].ok and reports[0].message.startswith("witness 0 of the batch: row 2 (U32SubtractionGate")
    assert pkg.WitnessReport(reps[0]).first_gate == reports[0].first_gate
