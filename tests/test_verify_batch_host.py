"""The batch verifier's core on the host (p2gpu_verify_batch_host: csrc/verifycore.hpp in a plain loop, no device) against the
lone host verifier (p2gpu_verify) and the oracle's verifier, on the oracle's proofs: the same verdict for every proof, the same
words through p2gpu_verify_reason, and p2gpu_last_error for the lowest failing proof of a batch.

What is independent of what: p2gpu_verify and p2gpu_verify_batch_host run ONE core (csrc/verifycore.hpp), so a comparison of the
two checks the batch plumbing -- offsets, reports, wording table, the error of the lowest failing proof -- and not the checks
themselves.  The checks are pinned from outside the core by the oracle's verifier (accept / reject of every byte string), by
the (reason, query, index) a mutation must get, worked out below from the order of the protocol and not read off the code,
and by tests/test_verifier.py, whose messages predate the core and are unchanged."""
import ctypes
import sys

import numpy as np
import pytest

import verify_batch_cases as vb
from conftest import GOLDEN, P
from test_verifier import make


def reports_equal_lone(pkg, vd, batch, reports):
    lib = pkg.load_library()
    for i, (data, r) in enumerate(zip(batch, reports)):
        ok, words = vb.lone(lib, vd._h, data)
        assert (r.ok, r.message) == (ok, words), (i, r, words)
        assert (r.reason == 0) == ok


@pytest.mark.parametrize("d,mix,seed,npi,nw,hasher", vb.CIRCUITS)
def test_agrees_with_the_host_verifier_and_the_oracle(pkg, orc, d, mix, seed, npi, nw, hasher):
    oc, vd, wires, pis = make(pkg, orc, d, mix, seed, npi, nw, hasher=hasher)
    proof, _ = oc.prove(wires, public_inputs=pis)
    L = vb.Layout(vd.to_bytes())
    assert L.want == len(proof)
    rng = np.random.default_rng(d)
    batch = [proof] + [vb.flip(proof, int(p), int(rng.integers(0, 8))) for p in rng.integers(0, len(proof), size=6)] + [proof]
    reports = vd.verify_batch(batch, device=False)
    assert reports[0].ok and reports[-1].ok and reports[0].message == "accepted" and reports[0].query is None
    reports_equal_lone(pkg, vd, batch, reports)
    for data, r in zip(batch, reports):
        assert oc.verify(data) == r.ok


def test_targeted_mutations_in_one_batch(pkg, orc):
    oc, vd, wires, pis = make(pkg, orc, 8, "ecdsa", 3, npi=2)
    proof, tr = oc.prove(wires, public_inputs=pis)
    lib = pkg.load_library()
    L = vb.Layout(vd.to_bytes())
    # the slot that continues the previous value is the query index's low bits: the probe of the helper finds that one
    assert vb.continuing_slot(lib, vd._h, proof, L, query=1) == int(tr.query_indices[1]) & 15
    muts = vb.mutations(lib, vd._h, proof, L)
    # the lone entry point reaches the six checks with these positions (the same core as the batch: this pins the positions)
    alone = {name: vb.lone(lib, vd._h, m) for name, m in muts}
    assert not any(ok for ok, _ in alone.values())
    for want, name in zip(vb.SIX, ("opening = 2^64 - 1", "opening", "initial path length", "initial sibling", "fold value, continuing slot",
                                   "step sibling")):
        assert want in alone[name][1], (name, alone[name])
    assert "Merkle path of initial oracle 1" in alone["leaf element"][1] and "Merkle path of fold step 0" in alone["fold value, another slot"][1]
    assert alone["leaf element"][1].startswith("query 1:")
    batch = vb.interleaved(proof, muts)
    reports = vd.verify_batch(batch, device=False)
    assert all(r.ok for r in reports[0::2]) and not any(r.ok for r in reports[1::2])
    reports_equal_lone(pkg, vd, batch, reports)
    for (name, m), r in zip(muts, reports[1::2]):
        if len(m) == len(proof):
            assert not oc.verify(m), name
    reached = {vb.reason_class(r.message) for r in reports[1::2]}
    for want in vb.SIX:
        assert any(want in x for x in reached), (want, reached)
    # the report's fields: query and oracle / step where the reason names them, the two lengths for a wrong length
    by = {name: r for (name, _), r in zip(muts, reports[1::2])}
    # What each mutation must get, from the verifier's order.  The openings are observed after zeta is drawn, so a changed opening
    # meets the identity at the same zeta (6); a wires cap or a public input changes every challenge: the identity fails first
    # (6).  A step cap, a final-polynomial word and the PoW witness enter the transcript after the identity's inputs and before
    # the PoW response: the response is another 64-bit word and misses its 16 zero bits (7), before any query is looked at.
    # In query 1: a leaf element or a sibling breaks that oracle's path (10), a fold value outside the continuing slot or a
    # step sibling breaks the step's path (13) after the continuation held.
    none = (None, None)
    want = {"wires cap": (6,) + none, "opening": (6,) + none, "opening = 2^64 - 1": (1,) + none, "step cap": (7,) + none,
            "leaf element": (10, 1, 1), "initial sibling": (10, 1, 0), "initial path length": (8, 1, 2),
            "fold value, continuing slot": (12, 1, 0), "fold value, another slot": (13, 1, 0), "step sibling": (13, 1, 0),
            "final polynomial": (7,) + none, "PoW witness": (7,) + none, "public input": (6,) + none,
            "one byte long": (3, len(proof) + 1, len(proof))}
    for name, w in want.items():
        assert (by[name].reason, by[name].query, by[name].index) == w, (name, by[name])
    assert by["PoW witness"].message == "proof-of-work response has too few leading zeros"
    assert by["step sibling"].message == "query 1: Merkle path of fold step 0 does not lead to its cap"
    assert by["leaf element"].message == "query 1: Merkle path of initial oracle 1 does not lead to its cap"
    assert by["one byte short"].message == "length %d, expected %d for this circuit" % (len(proof) - 1, len(proof))
    assert by["100 bytes"].reason == 1 and by["empty"].reason == 1
    # the return code, and p2gpu_last_error for the lowest failing proof, in p2gpu_verify's words
    rc, raw, err = vb.raw_batch(lib, vd._h, batch, device=False)
    assert rc == -9 and err == "proof 1 of the batch: proof rejected: " + alone[muts[0][0]][1]
    assert [x[1] for x in raw] == [r.reason for r in reports]
    rc, raw, err = vb.raw_batch(lib, vd._h, [muts[4][1]], device=False)
    assert rc == -9 and err == "proof rejected: " + alone[muts[4][0]][1]
    rc, raw, err = vb.raw_batch(lib, vd._h, [proof, proof], device=False)
    assert rc == 0 and raw == [(0, 0, 0xFFFFFFFF, 0xFFFFFFFF)] * 2


def test_shipped_reference_proofs_are_accepted(pkg, orc):
    from test_verifier import vk_blob
    sys.path.insert(0, GOLDEN)
    import reference_proofs as rp

    for name in ("basic_if", "basic_div"):
        c = rp.ReferenceCase(name)
        blob = c.blob()
        oc = orc.OracleCircuit(blob)
        vd = pkg.VerifierCircuitData(vk_blob(blob, oc.cap(), oc.digest()))
        ref = vd.decompress(c.compressed).to_bytes()
        good, bad = vd.verify_batch([ref, vb.flip(ref, len(ref) - 9)], device=False)
        assert good.ok and not bad.ok


def test_proof_of_an_unsatisfied_witness(pkg, orc):
    oc, vd, wires, _ = make(pkg, orc, 7, "ecdsa", 9)
    bad = wires.copy()
    bad[3, 5] = (int(bad[3, 5]) + 1) % P
    proofs = [oc.prove(wires)[0], oc.prove(bad)[0]]
    good, r = vd.verify_batch(proofs, device=False)
    assert good.ok and not r.ok and r.reason == 6 and "vanishing" in r.message and r.query is None


def test_argument_refusals_need_no_device(pkg, orc):
    oc, vd, wires, _ = make(pkg, orc, 5, "arith", 1)
    proof, _ = oc.prove(wires)
    lib = pkg.load_library()
    buf = np.frombuffer(proof + proof, dtype=np.uint8)
    off = np.array([0, len(proof), 2 * len(proof)], dtype=np.uintp)
    down = np.array([0, len(proof), len(proof) - 1], dtype=np.uintp)
    rep = (vb.RawReport * 2)()
    for fn in (lib.p2gpu_verify_batch, lib.p2gpu_verify_batch_host):
        assert fn(None, buf.ctypes.data, off.ctypes.data, 2, ctypes.byref(rep)) == -7
        assert fn(vd._h, None, off.ctypes.data, 2, ctypes.byref(rep)) == -7
        assert fn(vd._h, buf.ctypes.data, None, 2, ctypes.byref(rep)) == -7
        assert fn(vd._h, buf.ctypes.data, off.ctypes.data, 2, None) == -7
        assert fn(vd._h, buf.ctypes.data, off.ctypes.data, 0, ctypes.byref(rep)) == -7
        assert fn(vd._h, buf.ctypes.data, down.ctypes.data, 2, ctypes.byref(rep)) == -7 and b"decrease" in lib.p2gpu_last_error()
    assert lib.p2gpu_verify_batch_host(vd._h, buf.ctypes.data, off.ctypes.data, 2, ctypes.byref(rep)) == 0
    text = ctypes.create_string_buffer(4)
    assert lib.p2gpu_verify_reason(ctypes.byref(rep[0]), text, 4) == -2 and lib.p2gpu_verify_reason(None, text, 4) == -7
    import torch
    if not torch.cuda.is_available():  # no silent fall-back to the host loop
        assert lib.p2gpu_verify_batch(vd._h, buf.ctypes.data, off.ctypes.data, 2, ctypes.byref(rep)) == -3
        with pytest.raises(pkg.P2GpuError) as ei:
            vd.verify_batch([proof])
        assert ei.value.code == -3
