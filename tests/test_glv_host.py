"""The GLV decomposition three times over, without a GPU: the integer function (gadgets_glv.decompose_secp256k1_scalar), the
Python body of the "glvdec" generator (CircuitBuilderGlv.glv_values, on limbs), and csrc/glv.hpp -- the text the level walk runs
-- behind the stand-alone program csrc/tests/glv_check.cpp, compiled once plain and once with -fsanitize=address,undefined (a
host program, run here).  All three are compared with tests/curve_inputs.py's model, which rounds by exact halves on Python
integers, and with the defining identity k1 + GLV_S k2 = k (mod N)."""
import os
import random
import subprocess

import pytest

import curve_inputs as ci

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "acvm-backend-plonky2_amd", "csrc")
GL_P = 0xFFFFFFFF00000001          # a limb is a canonical Goldilocks element


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("glv_" + request.param) / "glv_check")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if request.param == "sanitized":     # can g++ link its sanitizer runtime at all?  Asked of a trivial program, before the code under test
        probe = str(tmp_path_factory.mktemp("probe") / "probe")
        r = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input=b"int main() { return 0; }\n", capture_output=True, timeout=120)
        if r.returncode:
            pytest.skip("g++ cannot link its sanitizer runtime on this machine: " + r.stderr.decode()[-200:])
    r = subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(CSRC, "tests", "glv_check.cpp")],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def run(exe, tmp_path, limb_lists):
    """[(k1, k2, k1_neg, k2_neg)] as the program prints them for the scalars given as limb lists"""
    path = str(tmp_path / "cases")
    with open(path, "w") as f:
        for limbs in limb_lists:
            f.write("%d %s\n" % (len(limbs), " ".join("%x" % v for v in limbs)))
    r = subprocess.run([exe, path], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(limb_lists)
    return [(int(a, 16), int(b, 16), bool(int(c)), bool(int(d))) for a, b, c, d in (line.split() for line in lines)]


def holds(k, k1, k2, n1, n2):
    return ((-k1 if n1 else k1) + ci.GLV_S * (-k2 if n2 else k2)) % ci.N == k % ci.N and k1 < 1 << 128 and k2 < 1 << 128


def test_constants_are_the_lattice_basis(pkg):
    """(A1, -MINUS_B1) and (A2, B2) are lattice vectors: a + b GLV_S = 0 (mod N); beta and S are cube roots of one"""
    t = pkg.translate
    assert (t.A1, t.MINUS_B1, t.A2, t.B2, t.GLV_S, t.GLV_BETA) == (ci.A1, ci.MINUS_B1, ci.A2, ci.B2, ci.GLV_S, ci.GLV_BETA)
    assert (ci.A1 - ci.MINUS_B1 * ci.GLV_S) % ci.N == 0 and (ci.A2 + ci.B2 * ci.GLV_S) % ci.N == 0
    assert pow(ci.GLV_S, 3, ci.N) == 1 and pow(ci.GLV_BETA, 3, ci.P) == 1 and ci.GLV_S != 1 and ci.GLV_BETA != 1
    assert ci.mul(ci.GLV_S, ci.G) == (ci.GLV_BETA * ci.GX % ci.P, ci.GY)


def test_integer_function_and_python_body(pkg):
    t = pkg.translate
    for k in ci.SCALARS:
        want = ci.decompose(k)
        assert t.decompose_secp256k1_scalar(k) == want and holds(k, *want), hex(k)
        assert t.CircuitBuilderGlv.glv_values(ci.digits(k, 8)) == ci.digits(want[0], 4) + ci.digits(want[1], 4) + [int(want[2]), int(want[3])]
    for limbs in ci.LIMB_LISTS:
        want = ci.decompose(ci.fold(limbs) % ci.N)
        assert t.CircuitBuilderGlv.glv_values(limbs) == ci.digits(want[0], 4) + ci.digits(want[1], 4) + [int(want[2]), int(want[3])]
    assert [ci.decompose(k)[2:] for k in ci.SCALARS[-4:]] == [(False, False), (False, True), (True, False), (True, True)]
    # the rounding edges round as exact halves say: the remainder half a unit below the tie rounds down, above it up
    for c, (lo, hi) in ((ci.B2, ci.ROUNDING_EDGES[:2]), (ci.MINUS_B1, ci.ROUNDING_EDGES[2:])):
        assert (c * lo) % ci.N == ci.HALF and (c * hi) % ci.N == ci.HALF + 1
    assert ci.decompose(ci.SCALARS[-1])[0] >> 96
    with pytest.raises(ValueError, match="more digits"):
        t.CircuitBuilderGlv.glv_values(ci.digits(ci.SCALARS[-1], 8), k1_limbs=3)


def test_the_checker_agrees_on_the_stated_scalars(checker, tmp_path):
    lists = [ci.digits(k, 8) for k in ci.SCALARS] + ci.LIMB_LISTS + [[0], [1], ci.digits(ci.N, 8), ci.digits(ci.N - 1, 16), [GL_P - 1] * 16]
    got = run(checker, tmp_path, lists)
    for limbs, g in zip(lists, got):
        k = ci.fold(limbs) % ci.N
        assert g == ci.decompose(k) and holds(k, *g), limbs
    assert max(max(g[:2]).bit_length() for g in got) == 128


def test_the_checker_agrees_on_seeded_random_scalars(checker, tmp_path):
    """20 000 scalars: uniform ones, small ones, ones near N and limb lists of 1 .. 16 limbs with limbs of up to 64 bits"""
    rng = random.Random(20261019)
    lists = [ci.digits(rng.randrange(ci.N), 8) for _ in range(14000)]
    lists += [ci.digits(rng.getrandbits(rng.randrange(1, 130)), 8) for _ in range(2000)]
    lists += [ci.digits(ci.N - 1 - rng.getrandbits(rng.randrange(1, 130)), 8) for _ in range(2000)]
    lists += [[rng.choice((0, 1, 0xFFFFFFFF, 1 << 32, GL_P - 1, rng.getrandbits(64) % GL_P, rng.getrandbits(32))) for _ in range(rng.randrange(1, 17))] for _ in range(2000)]
    got = run(checker, tmp_path, lists)
    signs = set()
    for limbs, g in zip(lists, got):
        k = ci.fold(limbs) % ci.N
        assert g == ci.decompose(k) and holds(k, *g), limbs
        signs.add(g[2:])
    assert len(signs) == 4
