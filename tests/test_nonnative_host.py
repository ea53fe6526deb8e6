"""The modular arithmetic of the device witness's four nonnative generators (csrc/nonnative.hpp: fold and reduce through bigdiv.hpp,
the 8 x 8-word product, the binary extended Euclidean inverse), without a GPU: the stand-alone program
csrc/tests/nonnative_check.cpp compiles the header the level walk compiles, once plain and once with
-fsanitize=address,undefined (a host program, run here), and every result is compared with Python's %, divmod and
pow(x, -1, M) on the integers `get_biguint_target` folds the limbs into."""
import os
import random
import subprocess

import pytest

import nonnative_inputs as ni

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "acvm-backend-plonky2_amd", "csrc")
P = 0xFFFFFFFF00000001


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("nonnative_" + request.param) / "nonnative_check")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if request.param == "sanitized":     # can g++ link its sanitizer runtime at all?  Asked of a trivial program, before the code under test
        probe = str(tmp_path_factory.mktemp("probe") / "probe")
        r = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input=b"int main() { return 0; }\n", capture_output=True, timeout=120)
        if r.returncode:
            pytest.skip("g++ cannot link its sanitizer runtime on this machine: " + r.stderr.decode()[-200:])
    r = subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(CSRC, "tests", "nonnative_check.cpp")],
                       capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def fold(limbs):
    return sum(v << (32 * i) for i, v in enumerate(limbs))


def check(exe, tmp_path, cases):
    """cases: [(op, field name, a limbs, b limbs)]; every printed pair is what Python computes, the inverse of zero is reported."""
    path = str(tmp_path / "cases")
    with open(path, "w") as f:
        for op, field, a, b in cases:
            f.write("%s %d %d %d %s\n" % (op, ni.FIELD_IDS[field], len(a), len(b), " ".join("%x" % v for v in list(a) + list(b))))
    r = subprocess.run([exe, path], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.decode().split("\n")[:-1]
    assert len(lines) == len(cases)
    zeros = 0
    for (op, field, a, b), line in zip(cases, lines):
        word = line.split()
        if op == "inv" and fold(a) % ni.ORDER[field] == 0:
            assert word == ["zero"], (op, field, a, line)
            zeros += 1
            continue
        assert word[0] == "ok", (op, field, a, b, line)
        assert (int(word[1], 16), int(word[2], 16)) == ni.expected(op, field, fold(a), fold(b)), (op, field, a, b, line)
    return zeros


def test_edges(checker, tmp_path):
    """The edge operands of tests/nonnative_inputs.py for both fields, the inverse of zero and of M, operands of M and above."""
    cases = []
    for f in ni.FIELDS:
        m = ni.ORDER[f]
        for _, kind, la, lb, fa, fb in ni.EDGES:
            op = "sub" if kind == "neg" else kind
            cases.append((op, f, ni.digits(fa(f), la), ni.digits(fb(f), lb)))
        cases += [("inv", f, [0] * 8, []), ("inv", f, ni.digits(m, 8), []), ("inv", f, [0], []), ("inv", f, ni.digits(2 * m, 9), []),
                  ("inv", f, ni.digits(m + 1, 8), []), ("inv", f, [ni.M] * 16, []),
                  ("add", f, ni.digits(m, 8), ni.digits(m, 8)), ("add", f, [ni.M] * 16, [ni.M] * 16), ("add", f, [], [5]), ("add", f, [5], []),
                  ("sub", f, [], ni.digits(m, 8)), ("sub", f, [ni.M] * 8, [ni.M] * 16), ("sub", f, [], [1]),
                  ("mul", f, [ni.M] * 16, [ni.M] * 16), ("mul", f, [ni.M] * 8, [ni.M] * 8), ("mul", f, ni.digits(m - 1, 8), []),
                  ("mul", f, ni.digits(m, 8), ni.digits(ni.X256, 8))]
    assert check(checker, tmp_path, cases) == 2 * 4


def test_limbs_at_or_above_two_to_the_32_carry(checker, tmp_path):
    cases = []
    for f in ni.FIELDS:
        cases += [("add", f, [P - 1] * 8, [1 << 32] * 8), ("sub", f, [1 << 32], [P - 1] * 16), ("mul", f, [P - 1] * 16, [P - 1] * 16),
                  ("mul", f, [1 << 63] * 8, [(1 << 32) + 9, 3]), ("inv", f, [P - 1] * 16, []), ("inv", f, [1 << 32], []), ("inv", f, [0, 1 << 32, P - 1], [])]
    assert check(checker, tmp_path, cases) == 0


def test_seeded_random_operands(checker, tmp_path):
    """1 500 cases per operation and field, 3 000 per operation, 12 000 in all: limb counts 0 .. 16, small and extreme limbs
    over-represented, limbs of 2^32 and above and operands of M and above among them."""
    rng = random.Random(20241019)

    def limb():
        k = rng.randrange(10)
        return (0, 1, ni.M, 0x80000000, P - 1, 1 << 32, rng.getrandbits(63))[k] if k < 7 else rng.getrandbits(32)

    cases = []
    for op in ("add", "sub", "mul", "inv"):
        for f in ni.FIELDS:
            for _ in range(1500):
                la, lb = rng.randrange(17), 0 if op == "inv" else rng.randrange(17)
                cases.append((op, f, [limb() for _ in range(la)], [limb() for _ in range(lb)]))
    assert any(fold(a) >= ni.ORDER[f] for _, f, a, _ in cases) and any(v >> 32 for _, _, a, _ in cases for v in a)
    zeros = check(checker, tmp_path, cases)
    assert 0 < zeros < 600
