"""Many witnesses of one circuit in one batched level walk (p2gpu_generate_witness_batch, WitnessPlan.generate_batch /
prove_batch; csrc/genwit.hip).  As in test_gpu_witness_gen.py the expected matrices come from translate.py's build() event
loop, tests/gate_wires.py and the committed digests, never from the code under test."""
import ctypes
import hashlib
import json
import os
import re
import sys

import numpy as np
import pytest

from conftest import GOLDEN, P

sys.path.insert(0, GOLDEN)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import device_build_inputs as dbi  # noqa: E402
import gen_proof_digests as gen  # noqa: E402
import witness_batch_inputs as wbi  # noqa: E402
import witness_gen_inputs as wgi  # noqa: E402

E_ARG, E_UNSATISFIED = -7, -5
with open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "acvm-backend-plonky2_amd", "csrc", "genwit.hip")) as _f:
    GROUP = int(re.search(r"constexpr uint32_t WALK_GROUP = (\d+);", _f.read()).group(1))   # witnesses per workgroup of the walk
CELL = re.compile(r"\(row (\d+), column (\d+)\)")


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


def _bitwise_batch(pkg, B):
    """(blob, cells, [values], [expected wires]) of the members 0 .. B-1: one circuit, one seed set."""
    members = [wbi.bitwise_member(pkg, k) for k in range(B)]
    blob, cells = members[0][0], members[0][1]
    for m in members:
        assert np.array_equal(m[0], blob) and m[1] == cells
    assert len({tuple(m[2]) for m in members}) == B        # the members differ
    return blob, cells, [m[2] for m in members], [m[3] for m in members]


def _assert_members(got, want, members=None):
    for b in range(len(want)) if members is None else members:
        bad = np.argwhere(_matrix(got[b]) != want[b])
        assert bad.size == 0, (b, [(int(c), int(r)) for c, r in bad[:8]])


# ---- CPU ----------------------------------------------------------------------------------------------------------
def test_batch_entry_point_without_a_plan(pkg):
    """Argument errors need no device, as for the lone entry points."""
    lib = pkg.load_library()
    assert lib.p2gpu_generate_witness_batch(None, None, 1, None, None, None) == E_ARG
    assert lib.p2gpu_generate_witness(None, None, None) == E_ARG


def test_python_methods(pkg):
    assert callable(pkg.prover.WitnessPlan.generate_batch) and callable(pkg.prover.WitnessPlan.prove_batch)


# ---- GPU ----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("B", [1, 3, GROUP, 2 * GROUP + 1])
def test_bitwise_batch(pkg, gpu, B):
    """One member, a width that is no power of two, a full group, two groups and a ragged third."""
    blob, cells, values, want = _bitwise_batch(pkg, B)
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    got, status, bad = plan.generate_batch(values)
    assert tuple(got.shape) == (B, cd.num_wires, cd.degree) and status == [0] * B and bad == [None] * B
    _assert_members(got, want)
    for b in {0, B - 1}:
        lone = plan.generate(values[b])
        assert np.array_equal(_matrix(plan.generate_batch([values[b]])[0][0]), _matrix(lone))
        assert np.array_equal(_matrix(lone), want[b])
    proofs = plan.prove_batch(values)
    assert [p.to_bytes() for p in proofs] == [cd.prove(w).to_bytes() for w in want]
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_isolation(pkg, gpu):
    """Three bad members of eight lower their own status only; the plan is as good as before afterwards."""
    B = 8
    blob, cells, values, want = _bitwise_batch(pkg, B)
    values = [list(v) for v in values]
    values[2][0] = 256                                      # witness 0: not 8 bits
    values[5][2] = P                                        # witness 2: not canonical
    values[7][3] += 1                                       # witness 5: fails the final assert_zero
    good = [0, 1, 3, 4, 6]
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    lone = {b: CELL.findall(_raises(pkg, E_UNSATISFIED, lambda: plan.generate(values[b]))) for b in (2, 5, 7)}
    _raises(pkg, E_UNSATISFIED, lambda: plan.generate(values[5]), "canonical")
    import torch

    lib = pkg.load_library()
    v = np.array(values, dtype=np.uint64)
    out = torch.empty((B, cd.num_wires, cd.degree), dtype=torch.int64, device=f"cuda:{cd.device_index()}")
    status, cellsb = np.full(B, 99, dtype=np.intc), np.zeros((B, 2), dtype=np.uint32)
    rc = lib.p2gpu_generate_witness_batch(plan._h, v.ctypes.data, B, ctypes.c_void_p(out.data_ptr()), status.ctypes.data, cellsb.ctypes.data)
    assert rc == E_UNSATISFIED
    assert status.tolist() == [0, 0, -5, 0, 0, -5, 0, -5]
    msg = lib.p2gpu_last_error().decode()
    assert "witness 2 of the batch" in msg and CELL.findall(msg) == lone[2], msg
    for b in (2, 5, 7):
        assert lone[b] and str(int(cellsb[b][0])) in {r for r, _ in lone[b]}, (b, cellsb[b], lone[b])
        assert (str(int(cellsb[b][0])), str(int(cellsb[b][1]))) == lone[b][-1]
    for b in good:
        assert cellsb[b].tolist() == [0xFFFFFFFF] * 2
    _assert_members(out, want, good)
    # status and bad cells may be asked for without the cells; the Python wrapper reports the same
    assert lib.p2gpu_generate_witness_batch(plan._h, v.ctypes.data, B, ctypes.c_void_p(out.data_ptr()), status.ctypes.data, None) == E_UNSATISFIED
    got, st, bad = plan.generate_batch(values)
    assert st == [0, 0, -5, 0, 0, -5, 0, -5] and [x is None for x in bad] == [s == 0 for s in st]
    _assert_members(got, want, good)
    res = plan.prove_batch(values)
    for b in range(B):
        if b in good:
            assert res[b].to_bytes() == cd.prove(want[b]).to_bytes()
        else:
            assert isinstance(res[b], pkg.P2GpuError) and res[b].code == E_UNSATISFIED and "row %d" % bad[b][0] in str(res[b])
    # no state is left behind: an all-good batch, then a lone call
    _, _, good_values, _ = _bitwise_batch(pkg, B)
    got, st, _ = plan.generate_batch(good_values)
    assert st == [0] * B
    _assert_members(got, want)
    assert np.array_equal(_matrix(plan.generate(good_values[2])), want[2])
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_lone_and_batched_calls_share_one_set_of_buffers(pkg, gpu):
    """One plan, in order: lone, a batch of 9 with member 4 contradictory, lone, a batch of 3, lone.  The value buffers hold
    9 witnesses from the second call on, and every later call lays its own B out in their front: a stride taken from the
    capacity, or a contradiction word left over from member 4, would show in a matrix or a status."""
    blob, cells, values, want = _bitwise_batch(pkg, 9)
    cd = pkg.CircuitData(blob)
    nine = [list(v) for v in values]
    nine[4][3] += 1                                         # member 4: ACIR witness 5 off by one fails the final assert_zero
    other = cd.witness_plan(cells)                          # (the cell a lone call names, asked of another plan: the sequence stays)
    cell = CELL.findall(_raises(pkg, E_UNSATISFIED, lambda: other.generate(nine[4])))[-1]
    other.close()
    plan = cd.witness_plan(cells)
    assert np.array_equal(_matrix(plan.generate(values[0])), want[0])
    got, status, bad = plan.generate_batch(nine)
    assert status == [0] * 4 + [E_UNSATISFIED] + [0] * 4
    assert [b is None for b in bad] == [s == 0 for s in status] and tuple(str(x) for x in bad[4]) == cell
    _assert_members(got, want, [0, 1, 2, 3, 5, 6, 7, 8])
    assert np.array_equal(_matrix(plan.generate(values[4])), want[4])        # (P2GPU_OK: generate raises otherwise)
    got, status, bad = plan.generate_batch(values[6:9])
    assert status == [0] * 3 and bad == [None] * 3
    _assert_members(got, want[6:9])
    assert np.array_equal(_matrix(plan.generate(values[8])), want[8])
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_custom_gate_chain_batch(pkg, gpu):
    """Every custom gate kind, with members whose comparison rows differ next to each other in one wave.  Member 3 of the
    first batch has seed (3, 1), the comparison's second operand, at 0 instead of 0x80000000: the first operand is
    0xFFFFFFFF, so the result stays 0 and the top chunk, the most significant difference and its bits change.  In the second
    batch the operand is 0xFFFFFFFF: every chunk is equal, the result flips to 1 and the range-check row after it changes."""
    kw, cells, values, want = wgi.custom_gate_chain()
    same_values, same_want, le = wbi.custom_gate_chain()
    zero_values, zero_want, zero_le = wbi.custom_gate_chain(0)
    flip_values, flip_want, flip_le = wbi.custom_gate_chain(wgi.F)
    assert same_values == values and (le, zero_le, flip_le) == (0, 0, 1)
    assert not np.array_equal(zero_want, want) and not np.array_equal(flip_want[:, 4], want[:, 4])
    cd = pkg.CircuitData.build(**kw)
    plan = cd.witness_plan(cells)
    for batch, expect in (([values, values, values, zero_values, values], [want, want, want, zero_want, want]),
                          ([flip_values, values], [flip_want, want])):
        got, status, _ = plan.generate_batch(batch)
        assert status == [0] * len(batch)
        _assert_members(got, expect)
        assert [p.to_bytes() for p in plan.prove_batch(batch)] == [cd.prove(w).to_bytes() for w in expect]
    plan.close()
    cd.close()


@pytest.mark.gpu
@pytest.mark.parametrize("hasher", [0, 1])
def test_blob_handle_and_built_handle_give_the_same_matrices(pkg, gpu, hasher):
    B = 3
    blob, cells, values, want = _bitwise_batch(pkg, B)
    a = pkg.CircuitData(dbi.with_hasher(blob, hasher))
    b = pkg.CircuitData.build(hasher=hasher, **dbi.decompose(pkg, blob))
    pa, pb = a.witness_plan(cells), b.witness_plan(cells)
    ga, gb = pa.generate_batch(values), pb.generate_batch(values)
    assert ga[1] == gb[1] == [0] * B
    _assert_members(ga[0], want)
    _assert_members(gb[0], want)
    assert [p.to_bytes() for p in pa.prove_batch(values)] == [p.to_bytes() for p in pb.prove_batch(values)] == [a.prove(w).to_bytes() for w in want]
    for x in (pa, pb, a, b):
        x.close()


@pytest.mark.gpu
def test_sha256_compression_batch(pkg, gpu):
    """The workload's own size (d = 15; test_gpu_witness_gen.py says why nothing smaller has the chain of 6 000 levels).
    Also here, where the buffers are large enough to see: the value buffers grow with the first batched call and not
    before -- after lone calls the plan holds what the lone layout needs (schedule, cell -> slot map, one set of values;
    every allocation rounded up to 2 MiB at the most), and the first batch of 4 grows that one set to four: the lone set is
    given back, so the call takes at least three sets less that set's rounding."""
    import test_translate
    import torch

    with open(os.path.join(GOLDEN, "proof_digests_hand.json")) as f:
        g = {x["name"]: x for x in json.load(f)}["sha256_compression"]
    cb = wgi.translated(pkg, dict(opcodes=[("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))]))
    block, state = [1 << 31] + [0] * 15, gen.SHA256_IV
    cells, values = cb.witness_seeds({i: v for i, v in enumerate(block + state)})
    blob = cb.blob()
    assert hashlib.sha256(blob.tobytes()).hexdigest() == g["blob_sha256"] and values[:24] == block + state
    rng = np.random.default_rng(4242)
    inputs = [[int(x) for x in rng.integers(0, 1 << 32, size=24)] for _ in range(2)]
    bad = list(values)
    bad[3] = 1 << 32
    batch = [values, inputs[0] + values[24:], inputs[1] + values[24:], bad]
    out_cells = [cb.builder.cells_of(cb.witness_target_map[24 + i])[0] for i in range(8)]
    cd = pkg.CircuitData(blob)
    routed = int(blob[:256].view(np.uint32)[4])

    def used(free_then, reserved_then):                     # device bytes taken since then, torch's own tensors apart
        torch.cuda.synchronize()
        return (free_then - torch.cuda.mem_get_info()[0]) - (torch.cuda.memory_reserved() - reserved_then)

    torch.cuda.synchronize()
    free0, res0 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    plan = cd.witness_plan(cells)
    info = plan.info()
    assert hashlib.sha256(_matrix(plan.generate(values)).tobytes()).hexdigest() == g["wires_sha256"]
    lone_bytes = used(free0, res0)
    layout = 8 * info["ops"] + 4 * (info["levels"] + 1) + 4 * routed * cd.degree + 8 * info["slots"] + 16 * info["seeds"] + 8
    free1, res1 = torch.cuda.mem_get_info()[0], torch.cuda.memory_reserved()
    got, status, cellsb = plan.generate_batch(batch)
    batch_bytes = used(free1, res1)
    print("sha256 plan after a batch of 4:", plan.info(), "device bytes: lone", lone_bytes, "layout", layout, "batch", batch_bytes)
    assert lone_bytes <= layout + 7 * (2 << 20)
    # four sets come in and the lone one goes out, which was rounded up by 2 MiB at the most
    assert batch_bytes >= 3 * 8 * info["slots"] - (2 << 20)
    assert status == [0, 0, 0, E_UNSATISFIED] and cellsb[:3] == [None] * 3 and cellsb[3] is not None
    assert plan.info()["walk_ms"] > 0
    m = [_matrix(got[b]) for b in range(3)]
    assert hashlib.sha256(m[0].tobytes()).hexdigest() == g["wires_sha256"]
    for b in (1, 2):
        assert [int(m[b][c, r]) for r, c in out_cells] == test_translate._sha256_compress(inputs[b - 1][16:], inputs[b - 1][:16])
    proofs = plan.prove_batch(batch)
    assert hashlib.sha256(proofs[0].to_bytes()).hexdigest() == g["proof_sha256"]
    for b in (1, 2):                                        # (prove's self-check accepted the matrix)
        assert len(proofs[b].to_bytes()) == len(proofs[0].to_bytes())
    assert isinstance(proofs[3], pkg.P2GpuError) and proofs[3].code == E_UNSATISFIED
    plan.close()
    cd.close()


@pytest.mark.gpu
def test_memory(pkg, gpu):
    """After plan.close() and cd.close() the process's device memory is back where it was, the buffers that batches of
    growing size made the plan allocate included (test_gpu_witness_gen's method)."""
    import torch

    blob, cells, values, _ = _bitwise_batch(pkg, 9)

    def cycle():
        cd = pkg.CircuitData(blob)
        plan = cd.witness_plan(cells)
        for B in (2, 9):
            got, status, _ = plan.generate_batch(values[:B])
            assert status == [0] * B
        plan.generate(values[0])
        del got
        plan.close()
        cd.close()

    for _ in range(2):          # (first round: whatever the runtime and torch's allocator take once per process)
        cycle()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    free0 = torch.cuda.mem_get_info()[0]
    for _ in range(3):
        cycle()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        assert torch.cuda.mem_get_info()[0] == free0


@pytest.mark.gpu
def test_arguments(pkg, gpu):
    import torch

    blob, cells, values, want = _bitwise_batch(pkg, 2)
    cd = pkg.CircuitData(blob)
    plan = cd.witness_plan(cells)
    _raises(pkg, E_ARG, lambda: plan.generate_batch([]))
    _raises(pkg, E_ARG, lambda: plan.prove_batch([]))
    _raises(pkg, E_ARG, lambda: plan.generate_batch([values[0], values[1][:-1]]), "seed values expected")
    lib = pkg.load_library()
    v = np.array(values, dtype=np.uint64)
    out = torch.empty((2, cd.num_wires, cd.degree), dtype=torch.int64, device=f"cuda:{cd.device_index()}")
    status = np.zeros(2, dtype=np.intc)
    ptr = ctypes.c_void_p(out.data_ptr())
    assert lib.p2gpu_generate_witness_batch(plan._h, v.ctypes.data, 0, ptr, status.ctypes.data, None) == E_ARG
    assert lib.p2gpu_generate_witness_batch(plan._h, None, 2, ptr, status.ctypes.data, None) == E_ARG
    assert lib.p2gpu_generate_witness_batch(plan._h, v.ctypes.data, 2, None, status.ctypes.data, None) == E_ARG
    assert lib.p2gpu_generate_witness_batch(plan._h, v.ctypes.data, 2, ptr, None, None) == E_ARG
    assert lib.p2gpu_generate_witness_batch(plan._h, v.ctypes.data, 2, ptr, status.ctypes.data, None) == 0
    _assert_members(out, want)
    plan.close()
    cd.close()
