"""The witness plan compiled on the device (p2gpu_witness_plan_build, csrc/genplan.hip) against the host compiler
(p2gpu_witness_plan_create): the exported arrays byte for byte, the same refusals with the same cell, and the matrices and
proofs the existing witness tests expect.  The host compiler is the differential oracle; the three-op case also states its
levels outright."""
import ctypes
import os
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_build_inputs as dbi  # noqa: E402
import gen_proof_digests as gen  # noqa: E402
import witness_gen_inputs as wgi  # noqa: E402
import witness_plan_inputs as wpi  # noqa: E402
import witness_plan_recorded as wpr  # noqa: E402

E_ARG = -7
COUNTS = ("ops", "levels", "widest_level", "slots", "seeds")
RECORDED = wpr.load(GOLDEN)


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


def _matrix(t):
    return t.cpu().numpy().view(np.uint64)


def _same_plan(cd, cells, keep=False, recorded=None):
    """Both compilers on one handle: every exported array and every count equal; the host compiler's also equal the plan
    recorded under the name `recorded` (tests/witness_plan_recorded.py).  Returns the device plan when `keep`."""
    host, dev = cd.witness_plan(cells), cd.witness_plan(cells, compile="device")
    try:
        ih, idv = host.info(), dev.info()
        assert {k: ih[k] for k in COUNTS} == {k: idv[k] for k in COUNTS}
        assert idv["compile_ms"] > 0
        eh, ed = host.export(), dev.export()
        if recorded is not None:
            wpr.compare(recorded, RECORDED[recorded], [ih[k] for k in COUNTS], eh)
        for name, a, b in zip(("cell_slot", "ops", "level_off"), eh, ed):
            assert a.shape == b.shape and a.dtype == b.dtype, name
            bad = np.argwhere(a != b)
            assert bad.size == 0, (name, len(bad), bad[:4].tolist(), a[tuple(bad[0])], b[tuple(bad[0])])
        assert len(ed[1]) == idv["ops"] and len(ed[2]) == idv["levels"] + 1
        return (dev, ed) if keep else None
    finally:
        host.close()
        if not keep:
            dev.close()


def _errors_agree(pkg, cd, cells, *words):
    msgs = []
    for how in ("host", "device"):
        with pytest.raises(pkg.P2GpuError) as e:
            cd.witness_plan(cells, compile=how)
        assert e.value.code == E_ARG, (how, e.value)
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1]
    for w in words:
        assert w in msgs[1], msgs[1]
    return msgs[1]


def _bitwise(pkg):
    prog = wgi.BITWISE
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cells, values = wgi.seeds_from_wires(cb, wires)
    return cb, blob, wires, cells, values


# ---- plan equality ----
@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(wpi.HAND_BUILT))
def test_hand_built(pkg, gpu, name):
    kw, cells = wpi.HAND_BUILT[name]()
    cd = pkg.CircuitData.build(**kw)
    _same_plan(cd, cells, recorded=name)
    cd.close()


@pytest.mark.gpu
def test_waiting_op_claims_nothing_levels(pkg, gpu):
    """i takes level 1, j waits for level 2 and claims nothing, so k takes level 1 -- stated here, not taken from the host."""
    kw, cells = wpi.waiting_op_claims_nothing()
    cd = pkg.CircuitData.build(**kw)
    for how in ("device", "host"):
        plan = cd.witness_plan(cells, compile=how)
        cell_slot, ops, level_off = plan.export()
        lv = wpi.op_levels(ops, level_off)
        assert lv[(0, wpi.OP_ARITHMETIC, 0)] == 1 and lv[(1, wpi.OP_U32_ARITHMETIC, 0)] == 2 and lv[(2, wpi.OP_ARITHMETIC, 0)] == 1, (how, lv)
        assert all(lv[(i, wpi.OP_SEED, 0)] == 0 for i in range(len(cells)))
        # the writers: i its output, k its output; j neither of the two words it shares, but its own inverse and limbs
        W = 0x80000000
        assert cell_slot[3, 0] & W and cell_slot[3, 2] & W and not cell_slot[3, 1] & W and not cell_slot[4, 1] & W and cell_slot[5, 1] & W
        plan.close()
    cd.close()


@pytest.mark.gpu
def test_twins_and_contenders_levels(pkg, gpu):
    kw, cells = wpi.base_sum_twins()
    cd = pkg.CircuitData.build(**kw)
    plan = cd.witness_plan(cells, compile="device")
    lv = wpi.op_levels(*plan.export()[1:])
    assert lv[(0, wpi.OP_BASE_SPLIT, 0)] == 1 and (0, wpi.OP_BASE_JOIN, 0) not in lv
    assert lv[(1, wpi.OP_BASE_JOIN, 0)] == 1 and (1, wpi.OP_BASE_SPLIT, 0) not in lv
    plan.close()
    cd.close()
    kw, cells = wpi.same_level_contenders()
    cd = pkg.CircuitData.build(**kw)
    plan = cd.witness_plan(cells, compile="device")
    lv = wpi.op_levels(*plan.export()[1:])
    assert [lv[(r, wpi.OP_ARITHMETIC, 0)] for r in range(3)] == [1, 2, 2]
    plan.close()
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["fibonacci", "quadratic"])
def test_assert_zero_programs(pkg, gpu, name):
    prog = {"fibonacci": wgi.FIBONACCI, "quadratic": wgi.QUADRATIC}[name]
    cb = wgi.translated(pkg, prog)
    blob, wires = cb.build(prog["witness"])
    cells, values = wgi.seeds_from_wires(cb, wires)
    cd = pkg.CircuitData(blob)
    _same_plan(cd, cells, recorded=name)
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_bitwise_blob_and_built_handles(pkg, gpu, hasher):
    cb, blob, wires, cells, values = _bitwise(pkg)
    a = pkg.CircuitData(dbi.with_hasher(blob, hasher))
    b = pkg.CircuitData.build(hasher=hasher, **dbi.decompose(pkg, blob))
    (pa, ea), (pb, eb) = _same_plan(a, cells, keep=True, recorded="bitwise"), _same_plan(b, cells, keep=True, recorded="bitwise")
    for x, y in zip(ea, eb):
        assert np.array_equal(x, y)
    assert np.array_equal(_matrix(pa.generate(values)), wires) and np.array_equal(_matrix(pb.generate(values)), wires)
    assert pa.prove(values).to_bytes() == pb.prove(values).to_bytes() == a.prove(wires).to_bytes()
    for x in (pa, pb, a, b):
        x.close()


@pytest.mark.gpu
def test_custom_gate_chain(pkg, gpu):
    kw, cells, values, want = wgi.custom_gate_chain()
    cd = pkg.CircuitData.build(**kw)
    plan, _ = _same_plan(cd, cells, keep=True, recorded="custom_gate_chain")
    got = _matrix(plan.generate(values))
    bad = np.argwhere(got != want)
    assert bad.size == 0, [(int(c), int(r), int(got[c, r]), int(want[c, r])) for c, r in bad[:8]]
    assert plan.prove(values).to_bytes() == cd.prove(want).to_bytes()
    plan.close()
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["basic_if", "basic_div"])
def test_reference_programs(pkg, gpu, name):
    import test_translate

    prog = test_translate._reference_programs()[name]
    cb = wgi.translated(pkg, prog, num_wires=135, public_parameters=prog["public"], private_parameters=prog["private"])
    cd = pkg.CircuitData(cb.blob())
    _same_plan(cd, cb.builder.seed_cells(), recorded=name)
    cd.close()


@pytest.mark.gpu
def test_sha256_compression(pkg, gpu):
    """d = 15: the only input with thousands of levels and real contention inside a level."""
    cb = wgi.translated(pkg, dict(opcodes=[("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))]))
    wit = {i: v for i, v in enumerate([1 << 31] + [0] * 15)}
    wit.update({16 + i: v for i, v in enumerate(gen.SHA256_IV)})
    cells, values = cb.witness_seeds(wit)
    cd = pkg.CircuitData(cb.blob())
    host = cd.witness_plan(cells)
    dev = cd.witness_plan(cells, compile="device")
    ih, idv = host.info(), dev.info()
    print("sha256 plan: host", ih, "device", idv)
    assert idv["levels"] > 6000 and {k: ih[k] for k in COUNTS} == {k: idv[k] for k in COUNTS}
    eh = host.export()
    wpr.compare("sha256_compression", RECORDED["sha256_compression"], [ih[k] for k in COUNTS], eh)
    for name, a, b in zip(("cell_slot", "ops", "level_off"), eh, dev.export()):
        assert np.array_equal(a, b), name
    assert np.array_equal(_matrix(dev.generate(values)), _matrix(host.generate(values)))
    host.close()
    dev.close()
    cd.close()


# ---- errors ----
@pytest.mark.gpu
def test_errors(pkg, gpu):
    cb, blob, wires, cells, values = _bitwise(pkg)
    n = wires.shape[1]
    cd = pkg.CircuitData(blob)
    _errors_agree(pkg, cd, cells + [(n, 0)], f"row {n}, column 0")
    _errors_agree(pkg, cd, cells + [cells[1]], "row %d, column %d" % cells[1], "twice")
    msg = _errors_agree(pkg, cd, cells[:2] + cells[3:], "seed is missing")
    stuck_cells = cb.builder.cells_of(cb.witness_target_map[2])
    assert any("(row %d, column %d)" % rc in msg for rc in stuck_cells), (msg, stuck_cells)
    cd.close()
    kw, seeds = wgi.arithmetic_cycle()
    cyc = pkg.CircuitData.build(**kw)
    _errors_agree(pkg, cyc, seeds, "dependency cycle", "row 0")
    cyc.close()
    # a sigma value that names no routed cell: two tampered cells, the smaller key (column 1) is the one reported
    bad = wpi.tamper_sigma(wpi.tamper_sigma(blob, 1, 3, 11), 2, 1, 5)
    t = pkg.CircuitData(bad)
    _errors_agree(pkg, t, cells, "sigma of cell (row 2, column 1) names no routed cell")
    t.close()
    # the front checks: a verifier-only handle
    cd = pkg.CircuitData(blob)
    vd = cd.verifier_data()
    out = ctypes.c_void_p()
    arr = np.array(cells, dtype=np.uint32)
    assert pkg.load_library().p2gpu_witness_plan_build(vd._h, arr.ctypes.data, len(arr), ctypes.byref(out)) == E_ARG and not out.value
    vd.close()
    cd.close()


# ---- memory ----
@pytest.mark.gpu
def test_memory(pkg, gpu):
    """The scratch is gone when _build returns: a device plan holds what a host plan holds, and close() gives it all back
    (test_gpu_witness_gen.py::test_memory's method)."""
    import torch

    cb, blob, wires, cells, values = _bitwise(pkg)

    def cycle(how):
        cd = pkg.CircuitData(blob)
        plan = cd.witness_plan(cells, compile=how)
        plan.prove(values)
        plan.close()
        cd.close()

    for _ in range(2):          # (first rounds: whatever the runtime allocates once per process)
        cycle("device")
        cycle("host")
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    cd = pkg.CircuitData(blob)
    free_cd = torch.cuda.mem_get_info()[0]
    held = {}
    for how in ("host", "device"):
        plan = cd.witness_plan(cells, compile=how)
        held[how] = free_cd - torch.cuda.mem_get_info()[0]
        plan.close()
        assert torch.cuda.mem_get_info()[0] == free_cd
    assert held["device"] <= held["host"], held      # (both may read 0: the runtime hands small buffers out of a block it keeps)
    cd.close()
    assert torch.cuda.mem_get_info()[0] == free0
    for _ in range(3):
        cycle("device")
    assert torch.cuda.mem_get_info()[0] == free0
