"""Shared by the batch-verifier tests (test_verify_batch_host.py, test_verifycore_host.py, test_gpu_verify_batch.py): the proof
layout worked out from a verifier key in Python (its own arithmetic), the targeted mutations of the issue at
positions computed from it, the lone verdict of ``p2gpu_verify`` and the raw call of the two batch entry points."""
import ctypes
import re

import numpy as np

P = 0xFFFFFFFF00000001
CIRCUITS = [  # d, mix, seed, npi, num_wires, hasher: tests/test_verifier.py::test_accepts_oracle_proofs, then two under PoseidonHash
    (5, "arith", 1, 0, 234, 0),     # no reduction step
    (6, "sha", 2, 0, 234, 0),
    (8, "ecdsa", 3, 2, 234, 0),
    (9, "ecdsa", 4, 4, 234, 0),
    (7, "arith", 5, 1, 135, 0),
    (10, "sha", 6, 0, 234, 0),      # two reduction steps
    (6, "sha", 2, 0, 234, 1),
    (8, "ecdsa", 3, 2, 234, 1),
]
SIX = ("non-canonical", "vanishing", "malformed initial opening", "Merkle path of initial oracle", "does not continue",
       "Merkle path of fold step")


class Layout:
    """Byte offsets of a proof of the circuit behind verifier key `vk` (header | gate table | cap | k_is)."""

    def __init__(self, vk):
        h = np.frombuffer(vk[:256], dtype=np.uint32)
        d, W, R, NC, K, QF, rate_bits, cap_h = (int(h[i]) for i in (2, 3, 4, 5, 7, 8, 9, 10))
        self.num_queries, n_steps, arity, hasher, self.num_pi, PP = int(h[12]), int(h[13]), [int(x) for x in h[14:22]], int(h[22]), int(h[24]), int(h[26])
        self.hb = hb = 32 if hasher else 25
        ncap = 1 << cap_h
        self.cols = [NC + R, W, K * (1 + PP), K * QF]
        nall = sum(self.cols)
        lgN = d + rate_bits
        self.open_at = 3 * hb * ncap
        self.num_openings = nall + K
        self.step_caps_at = self.open_at + 16 * (nall + K)
        self.queries_at = self.step_caps_at + n_steps * hb * ncap
        at, self.init_at = 0, []
        for o in range(4):
            self.init_at.append(at)
            at += 8 * self.cols[o] + 1 + hb * (lgN - cap_h)
        self.step_at, self.arity = [], arity[:n_steps]
        lg, final_len = lgN, 1 << d
        for ab in self.arity:
            self.step_at.append(at)
            lg -= ab
            final_len >>= ab
            at += (16 << ab) + 1 + hb * (lg - cap_h)
        self.query_bytes = at
        self.tail_at = self.queries_at + at * self.num_queries
        self.pow_at = self.tail_at + 16 * final_len
        self.pis_at = self.pow_at + 8
        self.want = self.pis_at + 8 * self.num_pi


def lone(lib, handle, data):
    """``p2gpu_verify`` on one byte string: (ok, the words behind "proof rejected: " or "accepted").  An empty string goes in
    with a valid pointer, as a member of a batch does."""
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    rc = lib.p2gpu_verify(handle, buf.ctypes.data, len(data))
    assert rc in (0, -9), (rc, lib.p2gpu_last_error())
    return (True, "accepted") if rc == 0 else (False, lib.p2gpu_last_error().decode().split("proof rejected: ", 1)[1])


def flip(proof, pos, bit=0):
    b = bytearray(proof)
    b[pos] ^= 1 << bit
    return bytes(b)


def continuing_slot(lib, handle, proof, L, query=0, step=0):
    """The slot of fold step `step` of query `query` that holds the value the previous step left: the one whose change the lone
    verifier calls a broken continuation (every other slot only breaks the step's Merkle path)."""
    at = L.queries_at + query * L.query_bytes + L.step_at[step]
    hits = [i for i in range(1 << L.arity[step]) if "does not continue" in lone(lib, handle, flip(proof, at + 16 * i))[1]]
    assert len(hits) == 1, hits
    return hits[0]


def mutations(lib, handle, proof, L, seed=5):
    """[(name, bytes)]: the targeted mutations, 150 seeded single-bit flips, the wrong lengths."""
    assert len(proof) == L.want and L.step_at, "the mutation list needs a circuit with a reduction step"
    q1 = L.queries_at + 1 * L.query_bytes                  # (query 1: the reports then name a query other than 0)
    slot = continuing_slot(lib, handle, proof, L, query=1)
    step0 = q1 + L.step_at[0]
    a = 1 << L.arity[0]
    big = bytearray(proof)
    big[L.open_at + 16 * 7:L.open_at + 16 * 7 + 8] = b"\xff" * 8
    out = [
        ("wires cap", flip(proof, 3, 2)),
        ("opening", flip(proof, L.open_at + 16 * 5 + 1, 4)),
        ("opening = 2^64 - 1", bytes(big)),
        ("step cap", flip(proof, L.step_caps_at + 2 * L.hb + 1, 1)),
        ("leaf element", flip(proof, q1 + L.init_at[1] + 8 * 3, 0)),
        ("initial sibling", flip(proof, q1 + L.init_at[0] + 8 * L.cols[0] + 1 + L.hb + 2, 5)),
        ("initial path length", flip(proof, q1 + L.init_at[2] + 8 * L.cols[2], 0)),
        ("fold value, continuing slot", flip(proof, step0 + 16 * slot, 3)),
        ("fold value, another slot", flip(proof, step0 + 16 * ((slot + 1) % a) + 8, 3)),
        ("step sibling", flip(proof, step0 + 16 * a + 1 + 4, 6)),
        ("final polynomial", flip(proof, L.tail_at + 8, 0)),
        ("PoW witness", flip(proof, L.pow_at, 0)),
        ("public input", flip(proof, L.pis_at, 0)),
    ]
    rng = np.random.default_rng(seed)
    for pos in rng.integers(0, len(proof), size=150):
        out.append(("bit flip at %d" % pos, flip(proof, int(pos), int(rng.integers(0, 8)))))
    out += [("one byte short", proof[:-1]), ("one byte long", proof + b"\0"), ("100 bytes", proof[:100]), ("empty", b"")]
    return out


def interleaved(proof, muts):
    """untouched, mutation 0, untouched, mutation 1, ..., untouched"""
    batch = [proof]
    for _, m in muts:
        batch += [m, proof]
    return batch


class RawReport(ctypes.Structure):
    _fields_ = [("status", ctypes.c_int32), ("reason", ctypes.c_uint32), ("query", ctypes.c_uint32), ("index", ctypes.c_uint32)]


def raw_batch(lib, handle, datas, device):
    """The C entry point itself: (return code, [(status, reason, query, index)], p2gpu_last_error after a rejection)."""
    offsets = np.zeros(len(datas) + 1, dtype=np.uintp)
    offsets[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    buf = np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)
    reports = (RawReport * len(datas))()
    fn = lib.p2gpu_verify_batch if device else lib.p2gpu_verify_batch_host
    rc = fn(handle, buf.ctypes.data, offsets.ctypes.data, len(datas), ctypes.byref(reports))
    err = lib.p2gpu_last_error().decode() if rc else ""
    return rc, [(r.status, r.reason, r.query, r.index) for r in reports], err


def reason_class(message):
    return re.sub(r"\d+", "#", message)
