"""tests/plonk_stage_model.py against the oracle, and the chosen inputs of tests/test_gpu_plonk_stages.py against what they claim
to place -- both without a GPU.

Anchor: on three circuits the oracle proves a satisfying witness; the model, given the trace's beta, gamma, alpha and public
input hash, computes Z, the partial products and the quotient chunk polynomials, and their values at the trace's zeta (Z also at
g zeta) must be the proof's openings.  Coverage: by the model's own account every input family puts at least one case in each
position the GPU test's docstring names; the counts are printed (run with -s).
"""
import sys

import numpy as np
import pytest

import plonk_stage_cases as cases
import plonk_stage_model as psm
from conftest import GOLDEN
from plonk_stage_model import EDGE, P

sys.path.insert(0, GOLDEN)
import param_circuits as pc  # noqa: E402
import proof_stages  # noqa: E402


def builders(pkg, orc):
    return [pc.build_fn(pkg.load_library().p2gpu_build_blob), pc.build_fn(orc.lib().orc_build_blob)]


ANCHORS = {
    "arith_d5_K1": lambda pkg, orc: pc.arith_circuit(5, 80, 80, 1, 3, 2, 1, builders(pkg, orc)) + ((),),
    "degree1_rate1": lambda pkg, orc: pc.degree1_circuit(5, 16, 16, 2, 1, 1, 1, builders(pkg, orc)) + ((),),
    "sha_d6_4pi": lambda pkg, orc: pkg.make_circuit(6, "sha", 3, num_public_inputs=4),
}


@pytest.mark.parametrize("name", list(ANCHORS))
def test_model_gives_the_oracles_openings(pkg, orc, name):
    blob, wires, pis = ANCHORS[name](pkg, orc)
    proof, tr = orc.OracleCircuit(blob).prove(wires, pis)
    cir = psm.Circuit(blob)
    K = cir.K
    st = psm.stages(orc, cir, wires, tr.pi_hash, [int(x) for x in tr.betas[:K]], [int(x) for x in tr.gammas[:K]],
                    [int(x) for x in tr.alphas[:K]])
    op = [tuple(int(x) for x in e) for e in np.frombuffer(proof_stages.stages(blob, proof)["openings"], dtype=np.uint64).reshape(-1, 2)]
    zeta = (int(tr.zeta[0]), int(tr.zeta[1]))
    g_zeta = psm.ext_mul(zeta, (cir.omega, 0))
    base = cir.NC + cir.R + cir.W          # OpeningSet order: constants, sigmas, wires, zs, zs_next, partial products, quotient
    for c in range(K):
        assert psm.eval_values_at(orc, st["zp"][c], zeta) == op[base + c], ("Z", c)
        assert psm.eval_values_at(orc, st["zp"][c], g_zeta) == op[base + K + c], ("Z at g zeta", c)
    for j in range(K * cir.PP):
        assert psm.eval_values_at(orc, st["zp"][K + j], zeta) == op[base + 2 * K + j], ("partial product", j)
    for j in range(K * cir.C):
        assert psm.eval_coeffs_at(st["quot"][j], zeta) == op[base + 2 * K + K * cir.PP + j], ("quotient chunk", j)
    assert len(op) == base + 2 * K + K * cir.PP + K * cir.C


def test_raw_word_formula_is_a_congruence():
    """raw_nc (used only to choose inputs) returns a u64 congruent to its argument, >= p on the example of its docstring."""
    rng = np.random.default_rng(3)
    for a, b in rng.integers(0, 1 << 64, size=(2000, 2), dtype=np.uint64):
        assert psm.raw_mul(int(a), int(b)) % P == int(a) * int(b) % P
    a, b = psm.raw_pair()
    assert psm.raw_mul(a, b) >= P and psm.raw_mul(psm.M32, (1 << 32) + 1) == psm.M64


def test_pin_coset_round_trip(pkg, orc):
    b = cases.circuit(pkg, orc, "arith32")
    rng = np.random.default_rng(4)
    for r in range(b.cir.C):
        t = cases.rand_words(rng, b.cir.n)
        assert np.array_equal(psm.lde(orc, b.cir, [psm.pin_coset(orc, b.cir, r, t)])[0, r::b.cir.C], t)


def test_every_family_places_its_cases(pkg, orc):
    # 2. challenge edges: every edge word, and each named special case, on two shapes at least
    ed = cases.family(pkg, orc, "edges")
    seen = set().union(*(c.account["words"] for c in ed))
    assert set(EDGE) <= seen
    for key in ("beta0", "gamma0", "alpha0", "alpha1", "repeat", "K1"):
        count = sum(bool(c.account[key]) for c in ed)
        print("edges: %s in %d cases" % (key, count))
        assert count >= 1
    assert len({c.circuit for c in ed}) >= 2
    # 3. targeted factors: a zero numerator in the first, a middle and the last chunk; row 0, row n - 1, a block boundary
    tg = cases.family(pkg, orc, "targets")
    zeros = [z for c in tg for z in c.account["zeros"]]
    for pos in ("first", "middle", "last"):
        print("targets: zero numerator in the %s chunk: %d" % (pos, sum(z[1] == pos for z in zeros)))
        assert any(z[1] == pos for z in zeros)
    for pl in ("row0", "last_row", "block_boundary"):
        print("targets: zero numerator at %s: %d" % (pl, sum(z[0] == pl for z in zeros)))
        assert any(z[0] == pl for z in zeros)
    print("targets: edge-word factors %d, zero words in Z / partial products %d" % (
        sum(c.account["edge_factors"] for c in tg), sum(c.account["zero_words_in_zp"] for c in tg)))
    assert all(c.account["z0"] == [1] * len(c.betas) and c.account["zero_words_in_zp"] > 0 for c in tg)
    assert len({c.circuit for c in tg}) >= 2
    # 4. pinned coset: one even and one odd coset on each of two shapes, every pinned word an edge word
    pn = cases.family(pkg, orc, "pinned")
    for c in pn:
        print("pinned: %s: %d wire words, %d Z / partial-product words, Z - 1 on zero %d times, wv + gamma >= p %d times" % (
            c.name, c.account["wire_words"], c.account["zp_words"], c.account["z_minus_1_wraps"], c.account["wv_plus_gamma_wraps"]))
        assert c.account["z_minus_1_wraps"] > 0 and c.account["wv_plus_gamma_wraps"] > 0
    for name in cases.PINNED:
        assert {c.account["parity"] for c in pn if c.circuit == name} == {0, 1}
    # 5. steered raw words: each of the four products has a raw word >= p, on each of two shapes
    st = cases.family(pkg, orc, "steered")
    for c in st:
        print("steered: %s: %s" % (c.name, c.account))
        if "raw_canonicalised" in c.account:
            assert c.account["raw_canonicalised"]["num"] >= 1 and c.account["raw_canonicalised"]["den"] >= 1
        else:
            assert all(c.account[k] == 1 for k in ("prev_n", "next_d", "next_d_last_chunk", "f_sum"))
    assert len({c.circuit for c in st}) >= 2


def test_zero_denominator_is_refused_by_the_model(pkg, orc):
    b = cases.circuit(pkg, orc, "arith32")
    wires = np.array(b.wires, copy=True)
    psm.target_factor(b.cir, wires, 5, 7, 0, 12345, 678, "den")
    assert not psm.denominators_nonzero(b.cir, wires, [12345, 1], [678, 2])
    with pytest.raises(AssertionError):
        psm.zs(b.cir, wires, [12345, 1], [678, 2])
