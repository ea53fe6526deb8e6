"""Regenerates tests/golden/proofio_codes.json: what p2gpu_proof_compress, p2gpu_proof_decompress and p2gpu_verify_compressed
answer -- the return code and, where it is 0, the SHA-256 of the output -- for oracle proofs of six small circuits, their
compressed forms and a fixed list of damaged copies of both.  It was run ONCE, with the library built at the commit named in
the file ("parent"), before proofio.hip was rewritten on top of verifycore.hpp; tests/test_proofio_pinned.py replays the same
cases against the library under test and demands equality.  Run from the repo root, with the library of that commit built:
    python tests/golden/gen_proofio_codes.py
The cases (``cases`` below) per circuit, each fed to all three entry points:
  * the proof and its compressed form as they are;
  * 40 seeded single-bit flips of each; each cut by 1 and by 3 bytes and extended by 7 zero bytes;
  * damage aimed by offset at every check of the proof's well-formedness (names "wf: ..."): a leaf word, a fold evaluation
    word, a final-polynomial word, a public input and, under PoseidonHash, a sibling digest word re-encoded as itself plus p
    -- the same field element, so that only the canonicity check can object -- and an initial and a step path-length byte
    +1 and -1.  w + p fits 64 bits only for w < 2^32 - 1; where a part of a proof holds no such word (field elements are
    rarely that small) its first word becomes 2^64 - 1 instead: another value, but compress looks at nothing except
    well-formedness, so there too no other check can object;
  * one opening changed to another canonical value: the proof no longer verifies, and compresses all the same;
  * the PoW witness of each form set to 2^64 - 1: both formats carry it as a u64, so both conversions still succeed.
"""
import ctypes
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
for p in (TESTS, HERE):
    if p not in sys.path:
        sys.path.insert(0, p)

import test_param_space as ps  # noqa: E402
import verify_batch_cases as vb  # noqa: E402
from test_verifier import make, vk_blob  # noqa: E402

P = vb.P
FIXTURE = os.path.join(HERE, "proofio_codes.json")
ENTRY_POINTS = ("compress", "decompress", "verify_compressed")
# name -> how to make it: (d, mix, seed, npi, hasher) of test_verifier.make, or the name of a test_param_space.GRID entry
CIRCUITS = {
    "d5_arith": (5, "arith", 1, 0, 0),
    "d9_ecdsa_pi4": (9, "ecdsa", 4, 4, 0),
    "d8_ecdsa_pi3_poseidon": (8, "ecdsa", 9, 3, 1),
    "arity_3_1_2": "arity_3_1_2",
    "arity_4_1": "arity_4_1",
    "K1_arity_1_2": "K1_arity_1_2",
}


def circuit(pkg, orc, name):
    """(verifier handle, the oracle's proof) of CIRCUITS[name]"""
    how = CIRCUITS[name]
    if isinstance(how, str):
        _, circ, patch = next(g for g in ps.GRID if g[0] == how)
        blob, wires = ps.make(pkg, orc, circ, patch)
        oc = orc.OracleCircuit(blob)
        vd = pkg.VerifierCircuitData(vk_blob(blob, oc.cap(), oc.digest()))
        pis = ()
    else:
        d, mix, seed, npi, hasher = how
        oc, vd, wires, pis = make(pkg, orc, d, mix, seed, npi, hasher=hasher)
    proof, _ = oc.prove(wires, public_inputs=pis)
    oc.close()
    return vd, proof


def word(data, at):
    return int.from_bytes(data[at:at + 8], "little")


def put_word(data, at, value):
    b = bytearray(data)
    b[at:at + 8] = value.to_bytes(8, "little")
    return bytes(b)


def plus_p(proof, at, count):
    """The proof with one of the `count` words from `at` re-encoded as itself plus p; 2^64 - 1 in the first where none is small enough."""
    for i in range(count):
        w = word(proof, at + 8 * i)
        if w < (1 << 32) - 1:
            return put_word(proof, at + 8 * i, w + P)
    return put_word(proof, at, (1 << 64) - 1)


def bump(data, at, by):
    b = bytearray(data)
    b[at] = (b[at] + by) & 0xFF
    return bytes(b)


def cases(proof, comp, L, hasher, seed):
    """[(name, bytes)] in a fixed order; L: verify_batch_cases.Layout of the circuit's key"""
    assert len(proof) == L.want
    out = []
    rng = np.random.default_rng(seed)
    for what, data in (("proof", proof), ("compressed", comp)):
        out.append((what, data))
        for pos in rng.integers(0, len(data), size=40):
            bit = int(rng.integers(0, 8))
            out.append(("%s: bit %d of byte %d" % (what, bit, pos), vb.flip(data, int(pos), bit)))
        out += [(what + ": 1 byte short", data[:-1]), (what + ": 3 bytes short", data[:-3]), (what + ": 7 zero bytes long", data + bytes(7))]
    q = L.queries_at + (L.num_queries // 2) * L.query_bytes      # a query in the middle
    leaf_at, leaf_words = q + L.init_at[1], L.cols[1]            # the wires leaf
    len_at = q + L.init_at[2] + 8 * L.cols[2]
    out += [
        ("wf: leaf word + p", plus_p(proof, leaf_at, leaf_words)),
        ("wf: final polynomial word + p", plus_p(proof, L.tail_at, (L.pow_at - L.tail_at) // 8)),
        ("wf: initial path length + 1", bump(proof, len_at, 1)),
        ("wf: initial path length - 1", bump(proof, len_at, -1)),
    ]
    if L.num_pi:
        out.append(("wf: public input + p", plus_p(proof, L.pis_at, L.num_pi)))
    if L.step_at:
        s = len(L.step_at) - 1                                   # the last step
        vals_at, nvals = q + L.step_at[s], 2 << L.arity[s]
        out += [
            ("wf: fold evaluation word + p", plus_p(proof, vals_at, nvals)),
            ("wf: step path length + 1", bump(proof, vals_at + 8 * nvals, 1)),
            ("wf: step path length - 1", bump(proof, vals_at + 8 * nvals, -1)),
        ]
    if hasher:
        sib_at = q + L.init_at[0] + 8 * L.cols[0] + 1
        out.append(("wf: sibling digest word + p", plus_p(proof, sib_at, 4 * proof[sib_at - 1])))
    at = L.open_at + 16 * 3
    out.append(("opening changed to another canonical value", put_word(proof, at, (word(proof, at) + 1) % P)))
    # the PoW witness is a u64 to both formats, not a field element: only the verifier minds
    for what, data in (("proof", proof), ("compressed", comp)):
        out.append((what + ": PoW witness 2^64 - 1", put_word(data, len(data) - 8 * L.num_pi - 8, (1 << 64) - 1)))
    return out


def answers(lib, handle, data):
    """[[rc, sha256 of the output or None] of compress, the same of decompress, [rc, None] of verify_compressed].  The size
    probe (out == NULL) must give the same code and, at code 0, the length the call then writes."""
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    res = []
    for fn in (lib.p2gpu_proof_compress, lib.p2gpu_proof_decompress):
        n = ctypes.c_size_t(0)
        probe = fn(handle, buf.ctypes.data, len(data), None, ctypes.byref(n))
        out = np.zeros(max(n.value, 1), dtype=np.uint8)
        m = ctypes.c_size_t(n.value)
        rc = fn(handle, buf.ctypes.data, len(data), out.ctypes.data, ctypes.byref(m))
        assert probe == rc and (rc != 0 or m.value == n.value), (probe, rc, n.value, m.value)
        res.append([rc, hashlib.sha256(out[:m.value].tobytes()).hexdigest() if rc == 0 else None])
    res.append([lib.p2gpu_verify_compressed(handle, buf.ctypes.data, len(data)), None])
    return res


def replay(pkg, orc, name):
    """{"proof_sha256", "cases": [[case name, answers]]} of one circuit with the library that is loaded"""
    vd, proof = circuit(pkg, orc, name)
    vk = vd.to_bytes()
    hasher = int(np.frombuffer(vk[:256], dtype=np.uint32)[22])
    comp = vd.compress(proof)
    seed = list(CIRCUITS).index(name) + 1
    lib = pkg.load_library()
    got = [[what, answers(lib, vd._h, data)] for what, data in cases(proof, comp, vb.Layout(vk), hasher, seed)]
    vd.close()
    return {"proof_sha256": hashlib.sha256(proof).hexdigest(), "cases": got}


def main():
    import __graft_entry__ as entry

    entry.build()
    pkg, orc = entry.load_package(), entry.load_oracle()
    root = os.path.dirname(TESTS)
    assert not subprocess.check_output(["git", "-C", root, "status", "--porcelain", "--", "acvm-backend-plonky2_amd", "include"]), "library sources differ from the commit"
    commit = subprocess.check_output(["git", "-C", root, "rev-parse", "HEAD"]).decode().strip()
    out = {"parent": commit, "entry_points": list(ENTRY_POINTS), "circuits": {name: replay(pkg, orc, name) for name in CIRCUITS}}
    with open(FIXTURE, "w") as f:
        json.dump(out, f, separators=(",", ":"))
        f.write("\n")


if __name__ == "__main__":
    main()
