"""The witness from the solver's values on the GPU (p2gpu_witness_plan_create / p2gpu_generate_witness / p2gpu_prove_seeds,
csrc/genwit.hip) against the pure-Python event loop of translate.py (`CircuitBuilder.build`, pinned by the reference's own
proofs in test_translate.py), tests/gate_wires.py and the committed digests.  Expected values never come from the code under
test."""
import ctypes
import hashlib
import json
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN, P

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_build_inputs as dbi  # noqa: E402
import gen_proof_digests as gen  # noqa: E402
import witness_gen_inputs as wgi  # noqa: E402

E_ARG, E_UNSATISFIED = -7, -5


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


def _matrix(t):
    return t.cpu().numpy().view(np.uint64)


def _raises(pkg, code, fn, *words):
    with pytest.raises(pkg.P2GpuError) as e:
        fn()
    assert e.value.code == code, e.value
    for w in words:
        assert w in str(e.value), e.value
    return str(e.value)


def _sha_witness(block, state):
    wit = {i: v for i, v in enumerate(block)}
    wit.update({16 + i: v for i, v in enumerate(state)})
    return wit


# ---- CPU: the seeds of the translator -----------------------------------------------------------------------------
@pytest.mark.parametrize("prog", [wgi.FIBONACCI, wgi.QUADRATIC, wgi.BITWISE], ids=["fibonacci", "quadratic", "bitwise"])
def test_seed_cells_and_values_agree_with_build(pkg, prog):
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cb2 = wgi.translated(pkg, prog)                        # a fresh builder: the same random PublicInputGate row
    cells, values = cb2.witness_seeds(prog["witness"])
    assert cells == cb.builder.seed_cells() and len(set(cells)) == len(cells)
    assert values == [int(wires[c, r]) for r, c in cells]
    inputs = len(cells) - (cb.builder.num_wires - 4)
    assert inputs == len(prog["witness"])                  # one seed per input witness, then the PublicInputGate row
    assert cells[inputs:] == [(cb.builder.pi_row, c) for c in range(4, cb.builder.num_wires)]
    assert np.array_equal(cb2.blob(), blob)
    with pytest.raises(ValueError):
        wgi.translated(pkg, prog).witness_seeds({})        # "stuck": no input assigned


def test_sha256_seed_count(pkg):
    cb = wgi.translated(pkg, dict(opcodes=[("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))]))
    cells, values = cb.witness_seeds(_sha_witness([1 << 31] + [0] * 15, gen.SHA256_IV))
    assert len(cells) == 24 + (234 - 4) == len(values)
    assert values[:24] == [1 << 31] + [0] * 15 + gen.SHA256_IV


def test_plan_create_without_a_prover_handle(pkg):
    """Argument errors need no device (like p2gpu_circuit_build's); without a prover handle there is nothing else to refuse."""
    lib = pkg.load_library()
    out = ctypes.c_void_p()
    cells = np.zeros((1, 2), dtype=np.uint32)
    assert lib.p2gpu_witness_plan_create(None, cells.ctypes.data, 1, ctypes.byref(out)) == E_ARG and not out.value
    assert lib.p2gpu_generate_witness(None, None, None) == E_ARG
    assert lib.p2gpu_prove_seeds(None, None, None, 0, None, None, None) == E_ARG
    lib.p2gpu_witness_plan_destroy(None)


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("prog,d", [(wgi.FIBONACCI, 2), (wgi.QUADRATIC, 3)], ids=["fibonacci", "quadratic"])
def test_assert_zero_programs(pkg, gpu, prog, d):
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    assert int(blob[:256].view(np.uint32)[2]) == d         # (the sizes of tests/golden/mini_builder.py's two circuits)
    cells, values = wgi.seeds_from_wires(cb, wires)
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    assert np.array_equal(_matrix(plan.generate(values)), wires)
    assert plan.prove(values).to_bytes() == cd.prove(wires).to_bytes()
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_range_and_xor_opcodes(pkg, gpu):
    """Both BaseSum directions: split_le of the RANGE / AND / XOR operands, le_sum of the 32 XOR bits."""
    prog = wgi.BITWISE
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cells, values = wgi.seeds_from_wires(cb, wires)
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    assert np.array_equal(_matrix(plan.generate(values)), wires)
    assert plan.prove(values).to_bytes() == cd.prove(wires).to_bytes()
    # seeds over derived classes are compared: the outputs 3 and 4 seeded as well (5 is a seed already)
    tm = cb.witness_target_map
    extra = [cb.builder.cells_of(tm[w])[-1] for w in (3, 4)]
    assert not set(extra) & set(cells)
    plan2 = cd.witness_plan(cells + extra)
    assert np.array_equal(_matrix(plan2.generate(values + [prog["outputs"][3], prog["outputs"][4]])), wires)
    _raises(pkg, E_UNSATISFIED, lambda: plan2.generate(values + [prog["outputs"][3] ^ 1, prog["outputs"][4]]), "row")
    plan2.close()
    # 256 is not 8 bits, 2^33 not 33 bits
    for w, bad in ((0, 256), (1, 1 << 33)):
        v = list(values)
        v[w] = bad                                          # (the input seeds come first, in witness order)
        assert values[w] == prog["witness"][w]
        _raises(pkg, E_UNSATISFIED, lambda: plan.generate(v), "row")
        _raises(pkg, E_UNSATISFIED, lambda: plan.prove(v), "row")
    v = list(values)
    v[2] = P                                                # not canonical
    _raises(pkg, E_UNSATISFIED, lambda: plan.generate(v), "canonical")
    assert np.array_equal(_matrix(plan.generate(values)), wires)     # and the plan is as good as before
    plan.close()
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["basic_if", "basic_div"])
def test_reference_programs(pkg, gpu, name):
    """The reference's shipped programs (public parameters: the in-circuit Poseidon row): its proof file, byte for byte."""
    import reference_proofs as rp
    import test_translate

    ref, prog = rp.ReferenceCase(name), test_translate._reference_programs()[name]
    cb = wgi.translated(pkg, prog, num_wires=135, public_parameters=prog["public"], private_parameters=prog["private"])
    blob = cb.blob()
    cells = cb.builder.seed_cells()
    pi_row = cb.builder.pi_row
    cls, roots = cb.builder._seed_classes()
    by_root = {cb.builder.find(cb.witness_target_map[w]): v for w, v in prog["witness"].items()}
    values = [by_root[rt] for rt in roots] + [int(ref.wires[c, pi_row]) for c in range(4, 135)]
    cd = pkg.CircuitData(blob)
    cd.set("pow_hint", ref.pow_witness)
    plan = cd.witness_plan(cells)
    assert np.array_equal(_matrix(plan.generate(values)), ref.wires)
    proof = plan.prove(values, public_inputs=list(ref.public_inputs))
    assert proof.to_bytes() == ref.uncompressed()
    assert cd.compress(proof.to_bytes()) == ref.compressed
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_sha256_compression(pkg, gpu):
    """The workload's own size (d = 15): nothing smaller has a chain of 6 000 levels."""
    with open(os.path.join(GOLDEN, "proof_digests_hand.json")) as f:
        g = {x["name"]: x for x in json.load(f)}["sha256_compression"]
    cb = wgi.translated(pkg, dict(opcodes=[("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))]))
    block, state = [1 << 31] + [0] * 15, gen.SHA256_IV
    cells, values = cb.witness_seeds(_sha_witness(block, state))      # (the random row: the generator build() draws from)
    blob = cb.blob()
    assert hashlib.sha256(blob.tobytes()).hexdigest() == g["blob_sha256"]
    cd = pkg.CircuitData(blob)
    # (output word 24 is seeded as well -- the solver knows it -- so that ONE plan serves the right and the wrong output)
    out_cell = cb.builder.cells_of(cb.witness_target_map[24])[0]
    cells, values = cells + [out_cell], values + [g["outputs"][0]]
    plan = cd.witness_plan(cells)
    info = plan.info()
    print("sha256 plan:", info)
    assert info["levels"] > 6000 and info["seeds"] == len(cells)
    got = _matrix(plan.generate(values))
    assert hashlib.sha256(got.tobytes()).hexdigest() == g["wires_sha256"]
    proof = plan.prove(values)
    assert hashlib.sha256(proof.to_bytes()).hexdigest() == g["proof_sha256"]
    # a wrong output word, and an input that is no 32-bit word
    _raises(pkg, E_UNSATISFIED, lambda: plan.generate(values[:-1] + [(g["outputs"][0] + 1) & 0xFFFFFFFF]), "row")
    v = list(values)
    v[3] = 1 << 32
    _raises(pkg, E_UNSATISFIED, lambda: plan.generate(v), "row")
    # another block through the same plan, then the first again: no state is left behind
    import test_translate

    rng = np.random.default_rng(99)
    block2 = [int(x) for x in rng.integers(0, 1 << 32, size=16)]
    state2 = [int(x) for x in rng.integers(0, 1 << 32, size=8)]
    want2 = test_translate._sha256_compress(state2, block2)
    w2 = _matrix(plan.generate(block2 + state2 + values[24:-1] + [want2[0]]))
    out_cells = [cb.builder.cells_of(cb.witness_target_map[24 + i])[0] for i in range(8)]
    assert [int(w2[c, r]) for r, c in out_cells] == want2
    assert hashlib.sha256(_matrix(plan.generate(values)).tobytes()).hexdigest() == g["wires_sha256"]
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_custom_gate_chain(pkg, gpu):
    kw, cells, values, want = wgi.custom_gate_chain()
    cd = pkg.CircuitData.build(**kw)
    plan = cd.witness_plan(cells)
    got = _matrix(plan.generate(values))
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(c), int(r), int(got[c, r]), int(want[c, r])) for c, r in bad[:8]]
    assert plan.prove(values).to_bytes() == cd.prove(want).to_bytes()      # (the self-check accepts: the copies hold)
    plan.close()
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_blob_handle_and_built_handle_give_the_same_matrix(pkg, gpu, hasher):
    prog = wgi.BITWISE
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cells, values = wgi.seeds_from_wires(cb, wires)
    a = pkg.CircuitData(dbi.with_hasher(blob, hasher))
    b = pkg.CircuitData.build(hasher=hasher, **dbi.decompose(pkg, blob))
    pa, pb = a.witness_plan(cells), b.witness_plan(cells)
    ia, ib = pa.info(), pb.info()
    assert {k: ia[k] for k in ("ops", "levels", "widest_level", "slots")} == {k: ib[k] for k in ("ops", "levels", "widest_level", "slots")}
    ma, mb = _matrix(pa.generate(values)), _matrix(pb.generate(values))
    assert np.array_equal(ma, wires) and np.array_equal(mb, wires)
    assert pa.prove(values).to_bytes() == pb.prove(values).to_bytes() == a.prove(wires).to_bytes()
    for x in (pa, pb, a, b):
        x.close()


@pytest.mark.gpu
def test_plan_errors(pkg, gpu):
    prog = wgi.BITWISE
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cells, _ = wgi.seeds_from_wires(cb, wires)
    n = wires.shape[1]
    cd = pkg.CircuitData(blob)
    _raises(pkg, E_ARG, lambda: cd.witness_plan(cells + [(n, 0)]), f"row {n}, column 0")
    _raises(pkg, E_ARG, lambda: cd.witness_plan(cells + [(0, 234)]), "row 0, column 234")
    _raises(pkg, E_ARG, lambda: cd.witness_plan(cells + [cells[1]]), "row %d, column %d" % cells[1], "twice")
    # witness 2 feeds the AND and the XOR: without its seed its class is stuck
    msg = _raises(pkg, E_ARG, lambda: cd.witness_plan(cells[:2] + cells[3:]), "row", "seed is missing")
    stuck_cells = cb.builder.cells_of(cb.witness_target_map[2])
    assert any("(row %d, column %d)" % rc in msg for rc in stuck_cells), (msg, stuck_cells)
    # a verifier-only handle, a device group
    lib = pkg.load_library()
    out = ctypes.c_void_p()
    arr = np.array(cells, dtype=np.uint32)
    vd = cd.verifier_data()
    assert lib.p2gpu_witness_plan_create(vd._h, arr.ctypes.data, len(arr), ctypes.byref(out)) == E_ARG and not out.value
    vd.close()
    cd.close()
    try:
        pkg.init([0, 0])
        grp = pkg.CircuitData(blob)
        _raises(pkg, E_ARG, lambda: grp.witness_plan(cells), "device group")
        grp.close()
    finally:
        pkg.init([0])
    # a generator that waits for its own output
    kw, seeds = wgi.arithmetic_cycle()
    cyc = pkg.CircuitData.build(**kw)
    _raises(pkg, E_ARG, lambda: cyc.witness_plan(seeds), "cycle", "row 0")
    cyc.close()


@pytest.mark.gpu
def test_memory(pkg, gpu):
    """After plan.close() and cd.close() the process's device memory is back where it was (test_gpu_device_build's method)."""
    import torch

    prog = wgi.BITWISE
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cells, values = wgi.seeds_from_wires(cb, wires)

    def cycle():
        cd = pkg.CircuitData(blob)
        plan = cd.witness_plan(cells)
        plan.prove(values)
        plan.close()
        cd.close()

    for _ in range(2):          # (first round: whatever the runtime allocates once per process)
        cycle()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    assert torch.cuda.mem_get_info()[0] <= free0
    plan.close()
    cd.close()
    assert torch.cuda.mem_get_info()[0] == free0
    for _ in range(5):
        cycle()
    assert torch.cuda.mem_get_info()[0] == free0
