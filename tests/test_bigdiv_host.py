"""The long division of the device witness's div-rem generator (csrc/bigdiv.hpp: Knuth's algorithm D on 32-bit words), without
a GPU: the stand-alone program csrc/tests/bigdiv_check.cpp compiles the header the level walk compiles, once plain and once
with -fsanitize=address,undefined (a host program, run here), and every quotient and remainder is compared with Python's
divmod on the integers `get_biguint_target` folds the limbs into."""
import os
import random
import subprocess

import pytest

import biguint_inputs as bi

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "acvm-backend-plonky2_amd", "csrc")
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("bigdiv_" + request.param) / "bigdiv_check")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if request.param == "sanitized":     # can g++ link its sanitizer runtime at all?  Asked of a trivial program, before the code under test
        probe = str(tmp_path_factory.mktemp("probe") / "probe")
        r = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input=b"int main() { return 0; }\n", capture_output=True, timeout=120)
        if r.returncode:
            pytest.skip("g++ cannot link its sanitizer runtime on this machine: " + r.stderr.decode()[-200:])
    r = subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(CSRC, "tests", "bigdiv_check.cpp")],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run(exe, tmp_path, cases):
    """cases: [(a limbs, b limbs)] -> per case None (the divisor is zero) or (add-back steps, quotient, remainder)."""
    path = str(tmp_path / "cases")
    with open(path, "w") as f:
        for a, b in cases:
            f.write("%d %d %s\n" % (len(a), len(b), " ".join("%x" % v for v in list(a) + list(b))))
    r = subprocess.run([exe, path], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(cases)
    out = []
    for line in lines:
        word = line.split()
        out.append(None if word == ["zero"] else (int(word[1]), int(word[2], 16), int(word[3], 16)))
        assert word == ["zero"] or word[0] == "ok"
    return out


def fold(limbs):
    return sum(v << (32 * i) for i, v in enumerate(limbs))


def check(exe, tmp_path, cases):
    got = run(exe, tmp_path, cases)
    for (a, b), g in zip(cases, got):
        if fold(b) == 0:
            assert g is None, (a, b, g)
        else:
            assert g is not None and g[1:] == divmod(fold(a), fold(b)), (a, b, g)
    return got


def test_edges(checker, tmp_path):
    """0; 2^32 - 1 in every limb; a < b; a = b; b one limb; b with a zero top limb; lb > la + 1 (div has no limbs); b = 0."""
    d = bi.digits
    cases = [(d(a, la), d(b, lb)) for _, la, lb, a, b in bi.DIV_REM_EDGES]
    cases += [(d(bi.X128 & bi.M, 1), d(bi.Y128, 4)),                 # lb > la + 1
              (d(bi.X128, 4), [0, 0, 0, 0]), ([0], [0]),             # b = 0
              ([0, 0, 0, 0], [5]), ([7], [7]), ([bi.M] * 8, [bi.M]), ([bi.M] * 8, [bi.M] * 8), ([1, 0, 0, 0], [0, 0, 0, 1])]
    check(checker, tmp_path, cases)


def test_quotient_words_of_all_ones(checker, tmp_path):
    (g,) = check(checker, tmp_path, [(bi.digits(2**128 - 1, 4), bi.digits(2**64 + 1, 3))])
    assert g[1:] == (2**64 - 1, 0)


def test_the_add_back_branch_runs(checker, tmp_path):
    """The estimate from the top two words is 4, the third word does not correct it, the subtraction goes negative: q = 3."""
    a, b = bi.ADD_BACK_A, bi.ADD_BACK_B
    assert divmod(a, b) == (3, 0x20000000 << 64)
    (g,) = check(checker, tmp_path, [(bi.digits(a, 3), bi.digits(b, 3))])
    assert g == (1, 3, 0x20000000 << 64)


def test_limbs_at_or_above_two_to_the_32_carry(checker, tmp_path):
    cases = [([P - 1, P - 1, 1 << 32, 5], [(1 << 32) + 9, 3]), ([1 << 63, 1 << 63], [1 << 32]), ([P - 1] * 32, [P - 1] * 16),
             ([P - 1] * 4, [1 << 32, 0, 0]), ([1 << 32], [1 << 32]), ([0, 1 << 32], [0, 0, 1])]
    check(checker, tmp_path, cases)


def test_the_largest_shape(checker, tmp_path):
    rng = random.Random(32016)
    cases = [([rng.getrandbits(32) for _ in range(32)], [rng.getrandbits(32) for _ in range(16)]) for _ in range(20)]
    cases += [([bi.M] * 32, [bi.M] * 16), ([bi.M] * 32, [1] + [0] * 15), ([0] * 31 + [1], [bi.M] * 15 + [0x80000000])]
    cases += [(bi.digits((0x1234_5678_9ABC_DEF0 << 448) % bi.SECP256K1_P ** 2, 16), bi.digits(bi.SECP256K1_P, 8))]
    check(checker, tmp_path, cases)


def test_seeded_random_cases_over_all_small_shapes(checker, tmp_path):
    """Every (la, lb) with la, lb <= 8, 50 cases each: 3 200 in all.  Small and extreme words are over-represented: they are
    where the estimate of a quotient word is wrong."""
    rng = random.Random(20240607)

    def word():
        k = rng.randrange(8)
        return (0, 1, bi.M, 0x80000000, 0x7FFFFFFF)[k] if k < 5 else rng.getrandbits(32)

    cases = [([word() for _ in range(la)], [word() for _ in range(lb)]) for la in range(1, 9) for lb in range(1, 9) for _ in range(50)]
    got = check(checker, tmp_path, cases)
    assert sum(1 for g in got if g is None) < len(cases) // 4
    assert any(g and g[0] for g in got)          # (the add-back branch is reached by random cases too)
