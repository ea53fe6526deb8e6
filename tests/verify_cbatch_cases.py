"""Shared by the tests of the batch entry points for compressed proofs (test_verify_cbatch_host.py, test_gpu_verify_cbatch.py):
a walk of the compressed container in Python with its own arithmetic (verify_batch_cases.Layout, the stored indices and the
length bytes), the targeted mutations at positions computed from it, the lone verdict of ``p2gpu_verify_compressed`` and the raw
calls of the batch entry points."""
import ctypes

import numpy as np

import verify_batch_cases as vb

# reason code -> the words behind "malformed proof: " (one per reject site of the lone decompressor, in its order)
C_WORDS = {
    16: "bad reduction arity in circuit",
    17: "caps / openings",
    18: "query indices",
    19: "initial tree entry",
    20: "fold step entry",
    21: "final polynomial / length",
    22: "final polynomial / public inputs",
    23: "query indices differ from the transcript's",
    24: "compressed Merkle path (initial tree)",
    25: "compressed Merkle path (fold step)",
    26: "fold chain",
}
C_CODES = {w: c for c, w in C_WORDS.items()}
UNREACHABLE = {16, 26}
NONE = 0xFFFFFFFF

# Circuits (verify_batch_cases.CIRCUITS rows) whose oracle proof has what the duplicate rules need, found on the CPU from the
# transcript's query indices and asserted by test_verify_cbatch_host.py::test_duplicate_condition:
REPEATED_INDEX = (5, "arith", 1, 0, 234, 0)          # 28 queries into 2^8 leaves: two queries with one index
SHARED_FOLD_LEAF = (10, "sha", 6, 0, 234, 0)          # two queries with different indices and one leaf of a fold step


class Walk:
    """Where everything lies in a compressed proof `comp` of the circuit behind verifier key `vk`."""

    def __init__(self, vk, comp):
        h = np.frombuffer(vk[:256], dtype=np.uint32)
        L = self.L = vb.Layout(vk)
        self.lgN, self.cap_h = int(h[2]) + int(h[9]), int(h[10])
        hb, nq = L.hb, L.num_queries
        at = L.queries_at
        self.idx_at = at
        self.idx = [int(x) for x in np.frombuffer(comp[at:at + 4 * nq], dtype=np.uint32)]
        assert all(x < 1 << self.lgN for x in self.idx)
        at += 4 * nq
        self.init = {}          # leaf index -> [(leaf_at, len_at, n)] * 4
        for x in sorted(set(self.idx)):
            ent = []
            for t in range(4):
                leaf_at, len_at = at, at + 8 * L.cols[t]
                n = comp[len_at]
                assert n <= self.lgN - self.cap_h
                ent.append((leaf_at, len_at, n))
                at = len_at + 1 + hb * n
            self.init[x] = ent
        self.steps = []         # per step: leaf index -> (evals_at, len_at, n)
        cur, lg = list(self.idx), self.lgN
        for ab in L.arity:
            cur = [x >> ab for x in cur]
            lg -= ab
            ents = {}
            for x in sorted(set(cur)):
                evals_at, len_at = at, at + 16 * ((1 << ab) - 1)
                n = comp[len_at]
                assert n <= lg - self.cap_h
                ents[x] = (evals_at, len_at, n)
                at = len_at + 1 + hb * n
            self.steps.append(ents)
        self.tail_at = at
        self.pow_at = at + (L.pow_at - L.tail_at)
        self.pis_at = self.pow_at + 8
        assert self.pis_at + 8 * L.num_pi == len(comp), "the walk ends where the container ends"


def lone(lib, handle, data):
    """``p2gpu_verify_compressed`` on one byte string: (return code, reason code or None, words).  The reason code is known
    for a rejection of the decompressor ("malformed proof: <words>": the table above); for the verifier's ("proof rejected:
    <words>") it is None and the words are what identify it."""
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    rc = lib.p2gpu_verify_compressed(handle, buf.ctypes.data, len(data))
    assert rc in (0, -9), (rc, lib.p2gpu_last_error())
    if rc == 0:
        return 0, 0, "accepted"
    err = lib.p2gpu_last_error().decode()
    if err.startswith("malformed proof: "):
        words = err[len("malformed proof: "):]
        return rc, C_CODES[words], words
    return rc, None, err.split("proof rejected: ", 1)[1]


def lone_error(lib, handle, data):
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    return lib.p2gpu_last_error().decode() if lib.p2gpu_verify_compressed(handle, buf.ctypes.data, len(data)) else ""


def put(data, at, new):
    return data[:at] + bytes(new) + data[at + len(new):]


U64_MAX = b"\xff" * 8


def mutations(vd, oc, wires, pis, proof, seed=5):
    """[(name, bytes)]: the targeted mutations of compress(proof), containers that are sound but hold a proof that is not,
    150 seeded single-bit flips, the wrong lengths.  oc, wires, pis: the oracle's circuit, to prove a broken witness."""
    comp = vd.compress(proof)
    w = Walk(vd.to_bytes(), comp)
    L, hb = w.L, w.L.hb
    x1 = w.idx[1]                                             # (query 1's entry: the reports then name a query other than 0)
    leaf_at, len_at, n = w.init[x1][1]
    # an initial entry with a kept sibling, and one whose path may grow
    some = [(x, t) for x in sorted(w.init) for t in range(4) if w.init[x][t][2] > 0]
    assert some, "no initial path keeps a sibling"
    sx, st = some[len(some) // 2]
    s_leaf, s_len, s_n = w.init[sx][st]
    out = [
        ("stored index -> another valid index", put(comp, w.idx_at + 4, (x1 ^ 1).to_bytes(4, "little"))),
        ("stored index >= 2^lgN", put(comp, w.idx_at + 4 * 3, (1 << w.lgN).to_bytes(4, "little"))),
        ("opening = 2^64 - 1", put(comp, L.open_at + 16 * 7, U64_MAX)),
        ("leaf word", vb.flip(comp, leaf_at + 8 * 3, 0)),
        ("leaf word = 2^64 - 1", put(comp, leaf_at + 8 * 3, U64_MAX)),
        ("path length + 1", put(comp, s_len, [s_n + 1])),
        ("path length - 1", put(comp, s_len, [s_n - 1])),
        ("kept sibling", vb.flip(comp, s_len + 1 + 2, 5)),
        ("kept sibling dropped", comp[:s_len] + bytes([s_n - 1]) + comp[s_len + 1:s_len + 1 + hb * (s_n - 1)] + comp[s_len + 1 + hb * s_n:]),
        ("final polynomial word", vb.flip(comp, w.tail_at + 8, 0)),
        ("final polynomial word = 2^64 - 1", put(comp, w.tail_at + 8, U64_MAX)),
        ("PoW witness", vb.flip(comp, w.pow_at, 0)),
        ("PoW witness = 2^64 - 1", put(comp, w.pow_at, U64_MAX)),
    ]
    if s_n < w.lgN - w.cap_h:
        out.append(("sibling added", comp[:s_len] + bytes([s_n + 1]) + comp[s_len + 1:s_len + 1 + hb * s_n] + bytes(hb) + comp[s_len + 1 + hb * s_n:]))
    if L.num_pi:
        out += [("public input", vb.flip(comp, w.pis_at, 0)), ("public input = 2^64 - 1", put(comp, w.pis_at, U64_MAX))]
    if w.steps:
        ents = w.steps[0]
        ex = sorted(ents)[len(ents) // 2]
        e_at, e_len, e_n = ents[ex]
        out += [("stored fold evaluation", vb.flip(comp, e_at + 16 + 8, 3)),
                ("stored fold evaluation = 2^64 - 1", put(comp, e_at + 16, U64_MAX))]
        kept = [x for x in sorted(ents) if ents[x][2] > 0]
        if kept:
            k_at, k_len, k_n = ents[kept[0]]
            out += [("step sibling", vb.flip(comp, k_len + 1 + 4, 6)),
                    ("step sibling dropped", comp[:k_len] + bytes([k_n - 1]) + comp[k_len + 1:k_len + 1 + hb * (k_n - 1)] + comp[k_len + 1 + hb * k_n:])]
        else:   # every path of the step is determined by the other leaves: one that claims a sibling it does not need
            k_at, k_len, k_n = ents[ex]
            out.append(("step sibling added", comp[:k_len] + bytes([1]) + bytes(hb) + comp[k_len + 1:]))
    # sound containers of unsound proofs: what only the verifier behind the decompressor can reject
    bad = wires.copy()
    bad[3, 5] = (int(bad[3, 5]) + 1) % vb.P
    out.append(("proof of an unsatisfied witness", vd.compress(oc.prove(bad, public_inputs=pis)[0])))
    out.append(("PoW witness changed before compression", vd.compress(vb.flip(proof, L.pow_at, 0))))
    witness = int.from_bytes(proof[L.pow_at:L.pow_at + 8], "little")
    if witness + vb.P < 1 << 64:     # the same field element, no canonical word: compress and decompress take it as a u64
        out.append(("PoW witness + p before compression", vd.compress(put(proof, L.pow_at, (witness + vb.P).to_bytes(8, "little")))))
    else:
        out.append(("PoW witness = 2^64 - 1 before compression", vd.compress(put(proof, L.pow_at, U64_MAX))))
    rng = np.random.default_rng(seed)
    for pos in rng.integers(0, len(comp), size=150):
        out.append(("bit flip at %d" % pos, vb.flip(comp, int(pos), int(rng.integers(0, 8)))))
    out += [("one byte short", comp[:-1]), ("one byte long", comp + b"\0"), ("100 bytes", comp[:100]), ("empty", b"")]
    return comp, out


def raw_cbatch(lib, handle, datas, device):
    """The C entry point itself: (return code, [(status, reason, query, index)], p2gpu_last_error after a rejection)."""
    offsets = np.zeros(len(datas) + 1, dtype=np.uintp)
    offsets[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    buf = np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)
    reports = (vb.RawReport * len(datas))()
    fn = lib.p2gpu_verify_batch_compressed if device else lib.p2gpu_verify_batch_compressed_host
    rc = fn(handle, buf.ctypes.data, offsets.ctypes.data, len(datas), ctypes.byref(reports))
    err = lib.p2gpu_last_error().decode() if rc else ""
    return rc, [(r.status, r.reason, r.query, r.index) for r in reports], err


def raw_decompress_batch(lib, handle, datas, want):
    """``p2gpu_proof_decompress_batch``: (return code, [status], [bytes])"""
    offsets = np.zeros(len(datas) + 1, dtype=np.uintp)
    offsets[1:] = np.cumsum([len(d) for d in datas], dtype=np.uint64)
    buf = np.frombuffer(b"".join(datas) or b"\0", dtype=np.uint8)
    out = np.full((len(datas), want), 0xA5, dtype=np.uint8)
    status = np.full(len(datas), 77, dtype=np.int32)
    rc = lib.p2gpu_proof_decompress_batch(handle, buf.ctypes.data, offsets.ctypes.data, len(datas), out.ctypes.data, status.ctypes.data)
    return rc, [int(s) for s in status], [out[i].tobytes() for i in range(len(datas))]


def lone_decompress(lib, handle, data):
    """``p2gpu_proof_decompress`` on one byte string: (return code, bytes or None)"""
    buf = np.frombuffer(bytes(data) or b"\0", dtype=np.uint8)
    n = ctypes.c_size_t(0)
    rc = lib.p2gpu_proof_decompress(handle, buf.ctypes.data, len(data), None, ctypes.byref(n))
    if rc:
        return rc, None
    out = np.zeros(n.value, dtype=np.uint8)
    assert lib.p2gpu_proof_decompress(handle, buf.ctypes.data, len(data), out.ctypes.data, ctypes.byref(n)) == 0
    return 0, out[:n.value].tobytes()
