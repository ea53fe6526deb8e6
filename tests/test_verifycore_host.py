"""The verifier core (csrc/verifycore.hpp) behind a stand-alone program, without the library and without a GPU:
csrc/tests/verifycore_check.cpp compiles the header the kernels compile, once plain and once with -fsanitize=address,undefined
(a host program, run here).  It verifies a proof, every truncation it is given -- each in a heap block of exactly that length --
and a few thousand seeded single-bit flips; every verdict must be the one p2gpu_verify_batch_host gives for the same bytes, and
the sanitizers must stay silent."""
import os
import subprocess

import pytest

import verify_batch_cases as vb
from test_verifier import make

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "acvm-backend-plonky2_amd", "csrc")
FLIP_COUNTS = {0: 2048, 1: 96}   # per hasher: a Poseidon permutation on the host costs ten times a Keccak one
M64 = (1 << 64) - 1


@pytest.fixture(scope="module", params=["plain", "sanitized"])
def checker(request, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("verifycore_" + request.param) / "verifycore_check")
    flags = ["-O2"] if request.param == "plain" else ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]
    if request.param == "sanitized":     # can g++ link its sanitizer runtime at all?  Asked of a trivial program, before the code under test
        probe = str(tmp_path_factory.mktemp("probe") / "probe")
        r = subprocess.run(["g++", "-fsanitize=address,undefined", "-x", "c++", "-", "-o", probe], input=b"int main() { return 0; }\n", capture_output=True, timeout=120)
        if r.returncode:
            pytest.skip("g++ cannot link its sanitizer runtime on this machine: " + r.stderr.decode()[-200:])
    r = subprocess.run(["g++", *flags, "-std=c++17", "-Wall", "-Werror", "-o", exe, os.path.join(CSRC, "tests", "verifycore_check.cpp")],
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


def flips(seed, count, size):
    """(position, bit) as verifycore_check.cpp's step() draws them"""
    out = []
    for _ in range(count):
        seed = (seed * 6364136223846793005 + 1442695040888963407) & M64
        r = seed >> 24
        out.append(((r >> 3) % size, r & 7))
    return out


@pytest.mark.parametrize("hasher", [0, 1])
def test_core_alone_gives_the_library_verdicts(pkg, orc, checker, tmp_path, hasher):
    oc, vd, wires, pis = make(pkg, orc, 6, "sha", 2, hasher=hasher)
    proof, _ = oc.prove(wires, public_inputs=pis)
    L = vb.Layout(vd.to_bytes())
    # one length inside every part of a proof, the part boundaries, one byte short and long, nothing at all
    q0 = L.queries_at
    lens = [0, 1, L.open_at - 1, L.open_at, L.open_at + 9, L.step_caps_at + 3, q0 - 1, q0, q0 + L.init_at[1] + 5, q0 + L.init_at[3] + 8 * L.cols[3],
            q0 + L.step_at[0] + 17, q0 + L.query_bytes, L.tail_at, L.tail_at + 7, L.pow_at, L.pow_at + 8, L.want - 1, L.want + 1, L.want + 64]
    seed, FLIPS = 20240917 + hasher, FLIP_COUNTS[hasher]
    vk_path, proof_path = str(tmp_path / "vk"), str(tmp_path / "proof")
    with open(vk_path, "wb") as f:
        f.write(vd.to_bytes())
    with open(proof_path, "wb") as f:
        f.write(proof)
    r = subprocess.run([checker, vk_path, proof_path, str(seed), str(FLIPS)] + [str(n) for n in lens], capture_output=True, timeout=600)
    assert r.returncode == 0 and b"runtime error" not in r.stderr and b"Sanitizer" not in r.stderr, r.stderr[-2000:]
    lines = r.stdout.decode().split("\n")[:-1]
    got = [tuple(int(x) for x in line.split()[:3]) for line in lines[:-1]]   # (a fourth column, well_formed(), is the program's own to check)
    cases = [proof] + [(proof + bytes(64))[:n] for n in lens] + [vb.flip(proof, p, b) for p, b in flips(seed, FLIPS, len(proof))]
    rc, raw, _ = vb.raw_batch(pkg.load_library(), vd._h, cases, device=False)
    assert rc == -9 and got == [x[1:] for x in raw]
    counts = [int(x) for x in lines[-1].split()[1:]]
    assert lines[-1].startswith("counts") and counts == [sum(1 for x in raw if x[1] == k) for k in range(len(counts))]
    assert counts[0] == 1 + lens.count(L.want) and counts[1] >= 7 and counts[3] >= 8 and sum(counts[8:]) > FLIPS // 2   # accepted as it is (and cut to its own length); shape verdicts; query verdicts
