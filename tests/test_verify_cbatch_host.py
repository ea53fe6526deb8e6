"""A batch of compressed proofs through the decompression core on the host (p2gpu_verify_batch_compressed_host:
csrc/decompresscore.hpp, then csrc/verifycore.hpp, in plain loops, no device) against the lone p2gpu_verify_compressed
(csrc/proofio.hip: sequential, a cursor and maps -- the code the reference's proof files pin) on the oracle's proofs: the same
verdict and the same words for every member of a batch, p2gpu_last_error for the lowest failing one.

The lone path is the oracle here, and what it answers is itself pinned from outside: the mutation list must reach every reject
site of the decompressor that can be reached and the verifier's sites behind it (asserted on the lone entry point, before the
batch is judged), and the proofs must hold the duplicates the lane-wise rules are about (asserted from the transcript)."""
import collections
import ctypes
import os
import subprocess

import numpy as np
import pytest

import verify_batch_cases as vb
import verify_cbatch_cases as vcb
from conftest import ROOT
from test_verifier import make


def words_of(lib, raw):
    rr = vb.RawReport(*raw)
    text = ctypes.create_string_buffer(400)
    assert lib.p2gpu_verify_reason(ctypes.byref(rr), text, len(text)) == 0
    return text.value.decode()


def reports_equal_lone(lib, handle, batch, raw):
    """Every report of a batch carries the lone call's code and words; returns the lone verdicts."""
    alone = [vcb.lone(lib, handle, data) for data in batch]
    for i, (r, (rc, code, words)) in enumerate(zip(raw, alone)):
        assert r[0] == rc and words_of(lib, r) == words, (i, r, words_of(lib, r), rc, words)
        if code is not None:       # accepted, or a reject site of the decompressor: the code is the table's, it names no query
            assert r[1:] == (code, vcb.NONE, vcb.NONE), (i, r, code)
        else:
            assert 0 < r[1] < 16, (i, r)
    return alone


@pytest.mark.parametrize("d,mix,seed,npi,nw,hasher", vb.CIRCUITS)
def test_interleaved_mutations_get_the_lone_verdict(pkg, orc, d, mix, seed, npi, nw, hasher):
    oc, vd, wires, pis = make(pkg, orc, d, mix, seed, npi, nw, hasher=hasher)
    proof, _ = oc.prove(wires, public_inputs=pis)
    lib = pkg.load_library()
    comp, muts = vcb.mutations(vd, oc, wires, pis, proof)
    # ---- coverage, on the lone entry point ----
    alone = {name: vcb.lone(lib, vd._h, m) for name, m in muts}
    assert not any(rc == 0 for rc, _, _ in alone.values())
    reached = {code for _, code, _ in alone.values() if code}
    steps = bool(vb.Layout(vd.to_bytes()).arity)
    want = set(vcb.C_WORDS) - vcb.UNREACHABLE - (set() if steps else {20, 25})      # (no fold step: no step entry, no step path)
    assert reached == want, (sorted(reached), sorted(want))
    said = {vb.reason_class(words) for _, code, words in alone.values() if code is None}
    for part in ("vanishing(zeta)", "proof-of-work", "non-canonical field element in final polynomial", "query #: Merkle path of initial oracle"):
        assert any(part in s for s in said), (part, said)
    assert alone["PoW witness changed before compression"][2].startswith("proof-of-work")
    assert alone["proof of an unsatisfied witness"][2].startswith("vanishing")
    trap = [name for name in alone if name.startswith("PoW witness") and name.endswith("before compression") and "changed" not in name]
    assert alone[trap[0]][2].startswith("non-canonical")                 # the head's VR_TAIL, after a decompression that went through
    assert alone["PoW witness = 2^64 - 1"][1] == 23                        # ... and in front of it when the indices no longer fit
    # ---- the batch ----
    batch = vb.interleaved(comp, muts)
    rc, raw, err = vcb.raw_cbatch(lib, vd._h, batch, device=False)
    assert all(r == (0, 0, vcb.NONE, vcb.NONE) for r in raw[0::2]) and all(r[0] == -9 for r in raw[1::2])
    reports_equal_lone(lib, vd._h, batch, raw)
    assert rc == -9 and err == "proof 1 of the batch: " + vcb.lone_error(lib, vd._h, batch[1])
    # the Python face: the same reports, the message through p2gpu_verify_reason
    reports = vd.verify_batch_compressed(batch[:9], device=False)
    assert [(r.ok, r.reason, r.message) for r in reports] == [(x[0] == 0, x[1], words_of(lib, x)) for x in raw[:9]]
    assert reports[0].message == "accepted" and reports[1].query is None and reports[1].index is None


def test_lowest_failing_proof_and_lone_members(pkg, orc):
    oc, vd, wires, pis = make(pkg, orc, 6, "sha", 2)
    proof, _ = oc.prove(wires, public_inputs=pis)
    lib = pkg.load_library()
    comp = vd.compress(proof)
    w = vcb.Walk(vd.to_bytes(), comp)
    late = vb.flip(comp, w.init[w.idx[2]][1][0] + 8)           # a wires leaf word of query 2: only the verifier sees it
    early = comp[:-1]
    rc, raw, err = vcb.raw_cbatch(lib, vd._h, [comp, comp, late, early, comp], device=False)
    assert rc == -9 and [r[0] for r in raw] == [0, 0, -9, -9, 0]
    # (the query named is the lowest whose rebuilt path hangs on that leaf's digest: query 2 or one before it)
    assert err == "proof 2 of the batch: " + vcb.lone_error(lib, vd._h, late) and "proof rejected: query " in err
    assert (raw[2][1], raw[2][3]) == (10, 1) and raw[2][2] <= 2 and raw[3][1:] == (21, vcb.NONE, vcb.NONE)
    rc, raw, err = vcb.raw_cbatch(lib, vd._h, [early], device=False)
    assert rc == -9 and err == "malformed proof: final polynomial / length"
    rc, raw, err = vcb.raw_cbatch(lib, vd._h, [comp], device=False)
    assert (rc, raw, err) == (0, [(0, 0, vcb.NONE, vcb.NONE)], "")
    # codes 0 - 15 keep their words
    for reason, query, index, text in ((7, vcb.NONE, vcb.NONE, "proof-of-work response has too few leading zeros"),
                                      (13, 4, 1, "query 4: Merkle path of fold step 1 does not lead to its cap")):
        assert words_of(lib, (-9, reason, query, index)) == text
    for code, text in vcb.C_WORDS.items():
        assert words_of(lib, (-9, code, vcb.NONE, vcb.NONE)) == text


def test_duplicate_condition(pkg, orc):
    """The proofs of the circuit list hold what the duplicate rules are about: a query index that repeats (one initial entry,
    two queries) and two different indices that share a leaf of a fold step (the later query copies, and stops inferring)."""
    found = {}
    for row in (vcb.REPEATED_INDEX, vcb.SHARED_FOLD_LEAF):
        assert row in vb.CIRCUITS
        d, mix, seed, npi, nw, hasher = row
        oc, vd, wires, pis = make(pkg, orc, d, mix, seed, npi, nw, hasher=hasher)
        proof, tr = oc.prove(wires, public_inputs=pis)
        L = vb.Layout(vd.to_bytes())
        idx = [int(x) for x in tr.query_indices[:L.num_queries]]
        comp = vd.compress(proof)
        assert vcb.Walk(vd.to_bytes(), comp).idx == idx
        shared, sh = False, 0
        for ab in L.arity:
            sh += ab
            groups = collections.defaultdict(set)
            for x in idx:
                groups[x >> sh].add(x)
            shared |= any(len(g) > 1 for g in groups.values())
        found[row] = (len(set(idx)) < len(idx), shared)
    assert found[vcb.REPEATED_INDEX][0] and found[vcb.SHARED_FOLD_LEAF][1], found


def test_argument_refusals_need_no_device(pkg, orc):
    oc, vd, wires, _ = make(pkg, orc, 5, "arith", 1)
    comp = vd.compress(oc.prove(wires)[0])
    lib = pkg.load_library()
    buf = np.frombuffer(comp + comp, dtype=np.uint8)
    off = np.array([0, len(comp), 2 * len(comp)], dtype=np.uintp)
    down = np.array([0, len(comp), len(comp) - 1], dtype=np.uintp)
    rep = (vb.RawReport * 2)()
    for fn in (lib.p2gpu_verify_batch_compressed, lib.p2gpu_verify_batch_compressed_host):
        assert fn(None, buf.ctypes.data, off.ctypes.data, 2, ctypes.byref(rep)) == -7
        assert fn(vd._h, None, off.ctypes.data, 2, ctypes.byref(rep)) == -7
        assert fn(vd._h, buf.ctypes.data, None, 2, ctypes.byref(rep)) == -7
        assert fn(vd._h, buf.ctypes.data, off.ctypes.data, 2, None) == -7
        assert fn(vd._h, buf.ctypes.data, off.ctypes.data, 0, ctypes.byref(rep)) == -7
        assert fn(vd._h, buf.ctypes.data, down.ctypes.data, 2, ctypes.byref(rep)) == -7 and b"decrease" in lib.p2gpu_last_error()
    out = np.zeros(2 * 200000, dtype=np.uint8)
    status = np.zeros(2, dtype=np.int32)
    fn = lib.p2gpu_proof_decompress_batch
    assert fn(None, buf.ctypes.data, off.ctypes.data, 2, out.ctypes.data, status.ctypes.data) == -7
    assert fn(vd._h, buf.ctypes.data, off.ctypes.data, 2, None, status.ctypes.data) == -7
    assert fn(vd._h, buf.ctypes.data, off.ctypes.data, 2, out.ctypes.data, None) == -7
    assert fn(vd._h, buf.ctypes.data, down.ctypes.data, 2, out.ctypes.data, status.ctypes.data) == -7
    assert lib.p2gpu_verify_batch_compressed_host(vd._h, buf.ctypes.data, off.ctypes.data, 2, ctypes.byref(rep)) == 0
    import torch
    if not torch.cuda.is_available():  # no silent fall-back to the host loop
        assert lib.p2gpu_verify_batch_compressed(vd._h, buf.ctypes.data, off.ctypes.data, 2, ctypes.byref(rep)) == -3
        assert fn(vd._h, buf.ctypes.data, off.ctypes.data, 2, out.ctypes.data, status.ctypes.data) == -3
        with pytest.raises(pkg.P2GpuError) as ei:
            vd.verify_batch_compressed([comp])
        assert ei.value.code == -3
        with pytest.raises(pkg.P2GpuError):
            vd.decompress_batch([comp])


def test_core_under_asan_ubsan(pkg, orc, tmp_path):
    """`make asan`: decompresscore.hpp behind p2gpu_verify_batch_compressed_host in the kernel-free library built with
    -fsanitize=address,undefined, and a stand-alone program that pushes seeded mutations through it and compares every report
    with p2gpu_verify_compressed's code and words.  Nothing is loaded into this process under a sanitizer."""
    csrc = os.path.join(ROOT, "acvm-backend-plonky2_amd", "csrc")
    oc, vd, wires, pis = make(pkg, orc, 6, "sha", 2)
    comp = vd.compress(oc.prove(wires, public_inputs=pis)[0])
    (tmp_path / "vk.blob").write_bytes(vd.to_bytes())
    (tmp_path / "comp.bin").write_bytes(comp)
    subprocess.check_call(["make", "-s", "-C", csrc, "build_asan/cbatch_check_asan"])
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([os.path.join(csrc, "build_asan", "cbatch_check_asan"), str(tmp_path / "vk.blob"), str(tmp_path / "comp.bin"), "300", "11"],
                       capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "DIFFERENCES 0" in r.stdout and "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
