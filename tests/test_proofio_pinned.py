"""p2gpu_proof_compress / p2gpu_proof_decompress / p2gpu_verify_compressed against the answers recorded before proofio.hip
was rewritten on top of verifycore.hpp (tests/golden/proofio_codes.json, written once by tests/golden/gen_proofio_codes.py
with the library of the commit the file names): for every case the return code of each entry point and, where it is 0, the
SHA-256 of its output must be the recorded ones -- accepted inputs give the same bytes, refused ones the same refusal.  The
cases (gen_proofio_codes.cases) are rebuilt here from the oracle's proofs, not stored."""
import json
import sys

import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import gen_proofio_codes as gen  # noqa: E402

with open(gen.FIXTURE) as f:
    RECORDED = json.load(f)
E_VERIFY = -9
# the damage aimed at one check of well-formedness each: where the circuit has the part, the case must be there
WF_CHECKS = {
    "wf: leaf word + p": lambda name: True,
    "wf: fold evaluation word + p": lambda name: name != "d5_arith",             # (d5_arith has no reduction step)
    "wf: final polynomial word + p": lambda name: True,
    "wf: public input + p": lambda name: "_pi" in name,
    "wf: initial path length + 1": lambda name: True,
    "wf: initial path length - 1": lambda name: True,
    "wf: step path length + 1": lambda name: name != "d5_arith",
    "wf: step path length - 1": lambda name: name != "d5_arith",
    "wf: sibling digest word + p": lambda name: name.endswith("poseidon"),
}


@pytest.fixture(scope="module")
def replayed(pkg, orc):
    """name -> what gen.replay gives with the library under test; each circuit is proved and replayed once"""
    assert RECORDED["entry_points"] == list(gen.ENTRY_POINTS) and list(RECORDED["circuits"]) == list(gen.CIRCUITS)
    done = {}

    def get(name):
        if name not in done:
            done[name] = gen.replay(pkg, orc, name)
        return done[name]
    return get


def pairs(replayed, name, select):
    """[(case name, answers now, answers recorded)] of the cases `select` picks; the inputs must be the recorded ones"""
    now, then = replayed(name), RECORDED["circuits"][name]
    assert now["proof_sha256"] == then["proof_sha256"], "the oracle's proof is not the one the fixture was recorded from"
    assert [c[0] for c in now["cases"]] == [c[0] for c in then["cases"]]
    return [(a[0], a[1], b[1]) for a, b in zip(now["cases"], then["cases"]) if select(a[0])]


@pytest.mark.parametrize("name", list(gen.CIRCUITS))
def test_proof_and_compressed_form_as_they_are(replayed, name):
    (_, proof_now, proof_then), (_, comp_now, comp_then) = pairs(replayed, name, lambda what: what in ("proof", "compressed"))
    assert proof_now == proof_then and comp_now == comp_then
    # compress takes the proof and nothing else does; decompress gives the proof back, and it verifies
    assert [a[0] for a in proof_now] == [0, E_VERIFY, E_VERIFY] and [a[0] for a in comp_now] == [E_VERIFY, 0, 0]
    assert comp_now[1][1] == replayed(name)["proof_sha256"]


@pytest.mark.parametrize("name", list(gen.CIRCUITS))
def test_bit_flips_truncations_and_extensions(replayed, name):
    got = pairs(replayed, name, lambda what: ": bit " in what or "short" in what or "long" in what)
    assert len(got) == 2 * (40 + 3)
    for what, now, then in got:
        assert now == then, what
        assert now[2][0] == E_VERIFY, what        # no damaged form verifies


@pytest.mark.parametrize("check", list(WF_CHECKS))
def test_well_formedness_check_still_objects(replayed, check):
    """One check of vc::well_formed per test: the damage leaves every other check of it content, so compress refuses these
    bytes (as recorded) only while that check is made."""
    seen = 0
    for name in gen.CIRCUITS:
        got = pairs(replayed, name, lambda what: what == check)
        assert len(got) == (1 if WF_CHECKS[check](name) else 0), name
        for what, now, then in got:
            assert now == then and [a[0] for a in now] == [E_VERIFY] * 3, name
            seen += 1
    assert seen >= 1


@pytest.mark.parametrize("name", list(gen.CIRCUITS))
def test_compress_does_not_verify(replayed, name):
    """A proof that is well-formed but does not verify still compresses, to the recorded bytes: an opening changed to another
    canonical value, a PoW witness that is no field element.  The same witness in the compressed form moves the transcript's
    query indices away from the stored ones."""
    got = pairs(replayed, name, lambda what: what.startswith("opening changed") or "PoW witness" in what)
    assert len(got) == 3
    for what, now, then in got:
        assert now == then, what
        assert [a[0] for a in now] == ([E_VERIFY] * 3 if what.startswith("compressed") else [0, E_VERIFY, E_VERIFY]), what
