"""Circuits off the reference's shape, on the CPU: every value of the parameters the circuit blob loader accepts
(csrc/hostcore.hip circuit_parse) and the edges of what it refuses.

Accepted (each one proved by the oracle and checked below, and by the GPU in test_gpu_param_space.py):
  num_challenges K     1, 2
  rate_bits            1, 2, 3   (QF = 2^rate_bits; C = QF cosets)
  FRI arity bits       1, 2, 3, 4 per step, in any order, 0 to 8 steps
  routed wires R       <= 128 with ceil(R / QF) <= 16 partial-product chunks (16 itself included)
  PoW bits             0 .. 32
  query rounds         1 .. 64
Refused with P2GPU_E_BLOB (test_loader_refuses_out_of_range_parameters): K 0 / 3, rate_bits 0 / 4, QF != 2^rate_bits,
arity bits 0 / 5, a step that leaves fewer rows than the cap (or than its own arity), 17 chunks, 9 steps, 0 / 65 queries,
33 PoW bits.

For every accepted grid point: the oracle's proof passes the oracle verifier, the product's host verifier, a compress /
decompress round trip and tests/golden/fri_check.py (the independent pure-Python reader); one flipped byte of a fold value
and one of a step Merkle path are rejected by all three.
"""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import fri_check  # noqa: E402
import param_circuits as pc  # noqa: E402
import proof_stages  # noqa: E402
from test_verifier import vk_blob  # noqa: E402

E_BLOB = -1

# (name, circuit, patch): circuit = ("synth", mix, d) or (generator, d, R, W, K, rate_bits, cap_h); patch = with_params kwargs
GRID = [
    ("K1", ("synth", "sha", 10), dict(K=1)),
    ("arity_1", ("synth", "ecdsa", 9), dict(arity=[1])),
    ("arity_2_3", ("synth", "sha", 10), dict(arity=[2, 3])),
    ("arity_3_1_2", ("synth", "sha", 10), dict(arity=[3, 1, 2])),
    ("arity_1_1_1_1", ("synth", "sha", 10), dict(arity=[1, 1, 1, 1])),
    ("arity_4_1", ("synth", "ecdsa", 9), dict(arity=[4, 1])),
    ("arity_8_steps", ("synth", "sha", 10), dict(arity=[1] * 8)),
    ("K1_arity_1_2", ("synth", "sha", 10), dict(K=1, arity=[1, 2])),
    ("pow0", ("synth", "sha", 10), dict(pow_bits=0)),
    ("queries1", ("synth", "ecdsa", 9), dict(queries=1)),
    ("queries64", ("synth", "sha", 10), dict(queries=64)),
    ("rate2_R64_16chunks", ("arith", 10, 64, 64, 2, 2, 2), {}),
    ("rate2_K1_W135", ("arith", 10, 64, 135, 1, 2, 2), {}),
    ("rate2_R40_cap6", ("arith", 9, 40, 80, 2, 2, 6), {}),
    ("rate2_K1_arity_3_1", ("arith", 10, 48, 96, 1, 2, 3), dict(arity=[3, 1])),
    ("rate3_K1_generated", ("arith", 9, 80, 234, 1, 3, 4), dict(arity=[2, 2], pow_bits=12)),
    ("rate1_R32_16chunks", ("degree1", 10, 32, 32, 2, 1, 1), {}),
    ("rate1_K1_R20_cap5", ("degree1", 9, 20, 40, 1, 1, 5), dict(arity=[3])),
]


def builders(pkg, orc):
    return [pc.build_fn(pkg.load_library().p2gpu_build_blob), pc.build_fn(orc.lib().orc_build_blob)]


def make(pkg, orc, circuit, patch, seed=5):
    """(blob, wires) of a grid point."""
    if circuit[0] == "synth":
        blob, wires = pkg.make_circuit(circuit[2], circuit[1], seed)
    else:
        gen = pc.arith_circuit if circuit[0] == "arith" else pc.degree1_circuit
        blob, wires = gen(*circuit[1:], seed=seed, builders=builders(pkg, orc))
    return (pc.with_params(blob, **patch) if patch else blob), wires


def fault_offsets(blob, proof):
    """Byte offsets, in the first query round, of one fold value of the first reduction step and of a byte inside the
    first sibling of that step's Merkle path."""
    c = proof_stages.header(blob)
    st = proof_stages.stages(blob, proof)
    q0 = sum(len(st[k]) for k in ("wires_cap", "zs_partial_products_cap", "quotient_polys_cap", "openings", "fri_commit_caps"))
    lg = c["d"] + c["rate_bits"]
    init_len = sum(8 * n + 1 + 25 * max(lg - c["cap_h"], 0)
                   for n in (c["NC"] + c["R"], c["W"], c["K"] * (1 + c["PP"]), c["K"] * c["QF"]))
    a = c["arity"][0]
    assert lg - a - c["cap_h"] >= 1, "the first step's path must be non-empty for the path fault"
    fold = q0 + init_len + 16 * ((1 << a) - 1) + 3
    path = q0 + init_len + (16 << a) + 1 + 3
    return fold, path


def pow_bits(blob):
    return int(np.frombuffer(bytes(blob[:256]), dtype=np.uint32)[11])


def cap_list(cap_bytes):
    return [cap_bytes[i:i + 25] for i in range(0, len(cap_bytes), 25)]


@pytest.mark.parametrize("name,circuit,patch", GRID, ids=[g[0] for g in GRID])
def test_oracle_proofs_across_the_parameter_space(pkg, orc, name, circuit, patch):
    blob, wires = make(pkg, orc, circuit, patch)
    h = blob[:256].view(np.uint32)
    for k, word in (("K", 7), ("pow_bits", 11), ("queries", 12)):
        if k in patch:
            assert int(h[word]) == patch[k]
    if "arity" in patch:
        assert [int(x) for x in h[14:14 + int(h[13])]] == patch["arity"]
    oc = orc.OracleCircuit(blob)
    proof, _ = oc.prove(wires)
    assert oc.verify(proof)
    vd = pkg.VerifierCircuitData(vk_blob(blob, oc.cap(), oc.digest()))
    vd.verify(proof)
    comp = vd.compress(proof)
    assert vd.decompress(comp).to_bytes() == proof
    vd.verify_compressed(comp)
    c = proof_stages.header(blob)
    fri_check.check(c, proof, oc.digest(), cap_list(oc.cap()), pow_bits=pow_bits(blob))
    if c["steps"] == 0:
        return
    for what, off in zip(("fold value", "step path"), fault_offsets(blob, proof)):
        bad = bytearray(proof)
        bad[off] ^= 1
        bad = bytes(bad)
        assert not oc.verify(bad), what
        with pytest.raises(pkg.P2GpuError):
            vd.verify(bad)
        with pytest.raises(AssertionError):
            fri_check.check(c, bad, oc.digest(), cap_list(oc.cap()), pow_bits=pow_bits(blob))
    vd.close()
    oc.close()


def test_the_grid_covers_every_accepted_value():
    """A reader's table of what is proved: every K, rate_bits and arity the loader accepts, 16 chunks, 8 steps, and the
    ends of the PoW and query ranges appear in the CPU grid above and in the GPU grid."""
    import test_gpu_param_space as g

    for grid in (GRID, g.GRID):
        K, rates, ab, steps, chunks, pows, queries = set(), set(), set(), set(), set(), set(), set()
        for _, circuit, patch in grid:
            if circuit[0] == "synth":
                K0, rate, R, arity = 2, 3, 80, None
            else:
                K0, rate, R, arity = circuit[4], circuit[5], circuit[2], None
            K.add(patch.get("K", K0))
            rates.add(rate)
            arity = patch.get("arity", arity)
            if arity is not None:
                ab.update(arity)
                steps.add(len(arity))
            chunks.add(-(-R // (1 << rate)))
            pows.add(patch.get("pow_bits", 16))
            queries.add(patch.get("queries", 28))
        assert K == {1, 2} and rates == {1, 2, 3} and ab >= {1, 2, 3, 4}
        assert 16 in chunks and 8 in steps and 0 in pows and {1, 64} <= queries


# ---- what the loader refuses -------------------------------------------------------------------------------------------
def vk_of(blob, **words):
    """A verifier blob (flags 0b11, all-zero cap and digest: p2gpu_verifier_create only parses them) with header words
    replaced ("w<index>" = value)."""
    h = blob[:256].view(np.uint32)
    cap_bytes = bytes(25 << int(words.get("w10", h[10])))
    vk = np.frombuffer(vk_blob(pc.patch_header(blob, **words), cap_bytes, bytes(25)), dtype=np.uint8)
    return vk


def create(pkg, vk):
    try:
        pkg.VerifierCircuitData(vk).close()
        return 0
    except pkg.P2GpuError as e:
        return e.code


def _refusals(pkg, orc):
    """(what, accepted neighbour blob, refused blob): each refused blob differs from its neighbour in the one parameter."""
    base = pkg.make_circuit(10, "sha", 3)[0]                                   # K 2, rate 3, QF 8, R 80 (PP 9), cap 4, arity [4]
    small = pc.degree1_circuit(5, 16, 16, 2, 1, 1, 1, builders(pkg, orc))[0]   # rate 1, QF 2, R 16 (PP 7)
    r64 = pc.arith_circuit(6, 64, 64, 2, 2, 2, 1, builders(pkg, orc))[0]      # rate 2, 16 chunks
    r68 = pc.arith_circuit(6, 68, 68, 2, 2, 2, 1, builders(pkg, orc))[0]      # rate 2, 17 chunks
    assert int(r64[:256].view(np.uint32)[26]) == 15 and int(r68[:256].view(np.uint32)[26]) == 16
    ar = lambda a: dict(w13=len(a), **{f"w{14 + i}": x for i, x in enumerate(a + [0] * (8 - len(a)))})  # noqa: E731
    base1 = pkg.make_circuit(12, "sha", 3)[0]
    return [
        ("K 0", vk_of(base, w7=1), vk_of(base, w7=0)),
        ("K 3", vk_of(base, w7=2), vk_of(base, w7=3)),
        ("rate_bits 0", vk_of(small, w9=1, w8=2, w26=7), vk_of(small, w9=0, w8=1, w26=15)),
        ("rate_bits 4", vk_of(base, w9=3, w8=8, w26=9), vk_of(base, w9=4, w8=16, w26=4)),
        ("QF != 2^rate", vk_of(base, w8=8, w26=9), vk_of(base, w8=16, w26=4)),
        ("arity bits 0", vk_of(base, **ar([4, 1])), vk_of(base, **ar([4, 0]))),
        ("arity bits 5", vk_of(base, **ar([4])), vk_of(base, **ar([5]))),
        ("step below the cap", vk_of(base, **ar([4, 4, 1])), vk_of(base, **ar([4, 4, 2]))),
        ("step beyond the rows", vk_of(base, **ar([4, 4, 1])), vk_of(base, **ar([4, 4, 4]))),
        ("17 chunks", vk_of(r64), vk_of(r68)),
        ("9 steps", vk_of(base1, **ar([1] * 8)), vk_of(base1, w13=9, **{f"w{14 + i}": 1 for i in range(8)})),
        ("0 queries", vk_of(base, w12=1), vk_of(base, w12=0)),
        ("65 queries", vk_of(base, w12=64), vk_of(base, w12=65)),
        ("33 PoW bits", vk_of(base, w11=32), vk_of(base, w11=33)),
    ]


def test_loader_refuses_out_of_range_parameters(pkg, orc):
    """p2gpu_verifier_create runs the same circuit_parse as p2gpu_circuit_create: each refused value comes back as
    P2GPU_E_BLOB (never accepted, never a crash) while the neighbouring accepted value, one header word away, parses."""
    for what, ok, bad in _refusals(pkg, orc):
        assert create(pkg, ok) == 0, what
        assert create(pkg, bad) == E_BLOB, what
    # PoW 0 and 33 is the only change needed between accepted and refused at the low end too
    base = pkg.make_circuit(10, "sha", 3)[0]
    assert create(pkg, vk_of(base, w11=0)) == 0
