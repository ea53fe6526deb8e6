"""Keccak and Poseidon handles alive in one process, used in turn on one thread and from threads that have touched
only the other hasher's handle: every call gives what the handle gives when it is used alone.

The hasher of a circuit is a field of its handle and is passed to the hashing code explicitly (verifycore.hpp, template
parameter HK); nothing may depend on which handle a thread used last.  What each call must give is taken from each handle
before the other one exists (host test), or from each handle in a block of its own and from the oracle (GPU test).
"""
import threading

import numpy as np
import pytest

from test_verifier import make


def in_thread(first, fn):
    """fn() on a fresh thread whose only earlier library call is first(): a call on the OTHER hasher's handle."""
    box = {}

    def run():
        try:
            first()
            box["value"] = fn()
        except BaseException as e:  # noqa: BLE001 -- handed to the caller's thread
            box["error"] = e

    t = threading.Thread(target=run)
    t.start()
    t.join()
    if "error" in box:
        raise box["error"]
    return box["value"]


def verifier_calls(pkg, vd, hasher, proof):
    """Every host entry point of a verifier handle that reads or writes digests, as name -> thunk."""
    comp = vd.compress(proof)
    vk = vd.to_plonky2_bytes()

    def verify():
        vd.verify(proof)
        return True

    def round_trip_vk():
        vd2 = pkg.VerifierCircuitData.from_plonky2_bytes(vk, hasher=hasher)
        try:
            vd2.verify(proof)
            return vd2.to_bytes(), vd2.to_plonky2_bytes(), vd2.circuit_digest(), vd2.constants_sigmas_cap()
        finally:
            vd2.close()

    return {
        "to_plonky2_bytes": vd.to_plonky2_bytes,
        "from_plonky2_bytes": round_trip_vk,
        "to_bytes": vd.to_bytes,
        "verify": verify,
        "compress": lambda: vd.compress(proof),
        "decompress": lambda: vd.decompress(comp).to_bytes(),
    }


@pytest.fixture
def keccak_oracle_after(orc):
    """The oracle's stage-level helpers hash with its last circuit's hasher, process-wide: leave it as the tests before found it."""
    yield
    orc.lib().orc_set_hasher(0)


def test_verifier_handles_of_both_hashers_interleaved(pkg, orc, keccak_oracle_after):
    side = []
    for hasher in (0, 1):
        oc, vd, wires, pis = make(pkg, orc, 6, "sha", 2, hasher=hasher)
        proof, _ = oc.prove(wires, public_inputs=pis)
        calls = verifier_calls(pkg, vd, hasher, proof)
        # alone: the second handle is made only after the first one's results are taken
        side.append((vd, calls, {name: fn() for name, fn in calls.items()}))
    (vd_k, calls_k, alone_k), (vd_p, calls_p, alone_p) = side
    assert vd_k.hash_bytes() == 25 and vd_p.hash_bytes() == 32
    assert alone_k["to_plonky2_bytes"] != alone_p["to_plonky2_bytes"]
    # one thread, call by call in turn, in both orders
    for _ in range(2):
        for name in calls_k:
            assert calls_k[name]() == alone_k[name], ("keccak", name)
            assert calls_p[name]() == alone_p[name], ("poseidon", name)
        for name in reversed(list(calls_k)):
            assert calls_p[name]() == alone_p[name], ("poseidon", name)
            assert calls_k[name]() == alone_k[name], ("keccak", name)
    # fresh threads that have touched only the other hasher's handle
    for name in calls_k:
        assert in_thread(calls_p["verify"], calls_k[name]) == alone_k[name], ("keccak after poseidon", name)
        assert in_thread(calls_k["verify"], calls_p[name]) == alone_p[name], ("poseidon after keccak", name)
        assert in_thread(calls_p["to_plonky2_bytes"], calls_k[name]) == alone_k[name], ("keccak after poseidon vk", name)
        assert in_thread(calls_k["to_plonky2_bytes"], calls_p[name]) == alone_p[name], ("poseidon after keccak vk", name)
    vd_k.close()
    vd_p.close()


# ---- prover handles (GPU) ----------------------------------------------------------------------------------------------
SHAPES = [(5, "arith", 0, 0), (5, "arith", 0, 1), (8, "ecdsa", 3, 1)]  # d, mix, public inputs, hasher; the last has a reduction step


def size_bound(cd):
    return int(cd._lib.p2gpu_proof_size_bound(cd._h))


def prover_calls(cd, wires, pis, proof):
    def verify():
        cd.verify(proof)
        return True

    return {
        "prove": lambda: cd.prove(wires, public_inputs=pis).to_bytes(),
        "to_plonky2_bytes": lambda: cd.verifier_data().to_plonky2_bytes(),
        "to_blob": lambda: cd.to_blob().tobytes(),
        "verify": verify,
    }


@pytest.mark.gpu
def test_prover_handles_of_both_hashers_interleaved(pkg, orc, keccak_oracle_after):
    import torch

    assert torch.cuda.is_available(), "this test needs the MI355X"
    circuits = []
    for d, mix, npi, hasher in SHAPES:
        out = pkg.make_circuit(d, mix, 47, num_public_inputs=npi, hasher=hasher)
        blob, wires, pis = out[0], out[1], (out[2] if npi else ())
        oc = orc.OracleCircuit(blob)
        expect, _ = oc.prove(wires, public_inputs=pis)
        # alone: no other prover handle exists while this one's results are taken
        cd = pkg.CircuitData(blob)
        alone = {name: fn() for name, fn in prover_calls(cd, wires, pis, expect).items()}
        cd.close()
        assert alone["prove"] == expect and oc.verify(expect), (d, mix, hasher)
        circuits.append((blob, wires, pis, expect, alone))
    # all three alive together
    handles = [pkg.CircuitData(blob) for blob, *_ in circuits]
    calls = [prover_calls(cd, wires, pis, expect) for cd, (_, wires, pis, expect, _) in zip(handles, circuits)]
    alone = [c[4] for c in circuits]
    for cd, (_, _, _, expect, _) in zip(handles, circuits):
        assert size_bound(cd) == len(expect)
    names = list(calls[0])
    # one thread: every call on every handle in turn, then handle by handle in the other order
    for name in names:
        for i in range(len(handles)):
            assert calls[i][name]() == alone[i][name], (SHAPES[i], name)
    for i in reversed(range(len(handles))):
        for name in reversed(names):
            assert calls[i][name]() == alone[i][name], (SHAPES[i], name)
    # two threads at once, one on the Keccak handle, one on a Poseidon handle (a handle proves one proof at a time)
    for other in (1, 2):
        errors = []

        def work(i, first):
            try:
                calls[first]["verify"]()  # this thread's first call is on the other hasher's handle
                for _ in range(2):
                    for name in names:
                        if calls[i][name]() != alone[i][name]:
                            errors.append((SHAPES[i], name))
            except BaseException as e:  # noqa: BLE001
                errors.append((SHAPES[i], repr(e)))

        th = [threading.Thread(target=work, args=(0, other)), threading.Thread(target=work, args=(other, 0))]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
    for cd in handles:
        cd.close()


@pytest.mark.gpu
def test_proof_size_bound_is_the_proof_length_at_cap_height_3(pkg):
    """(8, "ecdsa") rebuilt with cap height 3, 16 PoW bits, 28 queries: p2gpu_proof_size_bound is the length of the proof."""
    import ctypes

    import test_build as tb

    blob0, wires = pkg.make_circuit(8, "ecdsa", 61)[:2]
    params, gates, ng, row_gate, gconst, copies = tb.decompose(blob0)
    params.cap_height, params.proof_of_work_bits, params.num_query_rounds = 3, 16, 28
    fn = pkg.load_library().p2gpu_build_blob
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    blob = tb.build_with(fn, params, gates, ng, row_gate, gconst, copies)
    assert int(blob[:256].view(np.uint32)[10]) == 3
    cd = pkg.CircuitData(blob)
    proof = cd.prove(wires).to_bytes()
    cd.verify(proof)
    assert size_bound(cd) == len(proof)
    # a buffer as long as the proof is enough; a shorter one is refused with the length needed
    w = np.ascontiguousarray(wires, dtype=np.uint64)
    for cap, rc_want in ((len(proof), 0), (len(proof) - 1, -2)):  # P2GPU_OK, P2GPU_E_BUFFER
        out = np.zeros(len(proof), dtype=np.uint8)
        plen = ctypes.c_size_t(cap)
        rc = cd._lib.p2gpu_prove(cd._h, w.ctypes.data, None, 0, out.ctypes.data, ctypes.byref(plen), None)
        assert rc == rc_want and plen.value == len(proof), (cap, rc, plen.value)
        if rc == 0:
            assert out.tobytes() == proof
        else:
            assert b"proof buffer too small: need %d bytes" % len(proof) in cd._lib.p2gpu_last_error()
    cd.close()
