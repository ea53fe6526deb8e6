"""The batched prover's core (csrc/provebatchcore.hpp) behind a stand-alone program, without the library and without a GPU:
tests/provebatch_check.cpp runs the bodies of the kernels in the order the library launches them, one thread per block,
and every proof of the batch must equal the CPU oracle's bytes for that circuit and witness -- the shapes without and with a
reduction step, with public inputs, under both hashers."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "acvm-backend-plonky2_amd", "csrc")
ORACLE = os.path.join(ROOT, "oracle")


@pytest.fixture(scope="module")
def checker(built, tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("provebatch") / "provebatch_check")
    r = subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Wno-unused-function", "-I", CSRC, "-I", ORACLE, "-o", exe,
                        os.path.join(HERE, "provebatch_check.cpp"), "-L", ORACLE, "-loracle", "-Wl,-rpath," + ORACLE],
                       capture_output=True, timeout=900)
    assert r.returncode == 0, r.stderr[-2000:]
    return exe


@pytest.mark.parametrize("d,mix,npi,nw,hasher", [(5, "arith", 0, 234, 0), (6, "sha", 0, 234, 1), (7, "arith", 1, 135, 0), (8, "ecdsa", 2, 234, 0)])
def test_core_alone_gives_the_oracle_bytes(pkg, checker, tmp_path, d, mix, npi, nw, hasher):
    out = pkg.make_circuit(d, mix, seed=3, num_public_inputs=npi, num_wires=nw, hasher=hasher)
    paths = [str(tmp_path / name) for name in ("blob", "wires", "pis")]
    out[0].tofile(paths[0])
    out[1].tofile(paths[1])
    (out[2] if npi else np.zeros(0, dtype=np.uint64)).tofile(paths[2])
    r = subprocess.run([checker, *paths, "2"], capture_output=True, timeout=600)
    text = r.stdout.decode()
    assert r.returncode == 0 and text.count("bytes equal") == 2 and "DIFF" not in text, text[-2000:] + r.stderr.decode()[-1000:]
