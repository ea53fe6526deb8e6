"""The public surface of the nonnative generators, without a device: the defines in the header, the op codes, the kind words
WitnessPlan makes of a generator list, and the argument refusals of the _genv pair with the new kinds."""
import ctypes
import os
import re

import numpy as np
import pytest

E_ARG = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_and_op_codes(pkg):
    with open(os.path.join(ROOT, "include", "p2gpu.h")) as f:
        flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    for line in ("#define P2GPU_GEN_NONNATIVE_ADD 2", "#define P2GPU_GEN_NONNATIVE_SUB 3", "#define P2GPU_GEN_NONNATIVE_MUL 4",
                 "#define P2GPU_GEN_NONNATIVE_INV 5", "#define P2GPU_FIELD_SECP256K1_BASE 0", "#define P2GPU_FIELD_SECP256K1_SCALAR 1",
                 "#define P2GPU_GEN_EQUALITY 0", "#define P2GPU_GEN_BIGUINT_DIVREM 1"):
        assert line + " " in flat + " ", line
    with open(os.path.join(ROOT, "acvm-backend-plonky2_amd", "csrc", "genops.hpp")) as f:
        text = f.read()
    for code in ("OP_NONNATIVE_ADD == 15", "OP_NONNATIVE_SUB == 16", "OP_NONNATIVE_MUL == 17", "OP_NONNATIVE_INV == 18"):
        assert code in text
    t = pkg.translate
    assert (t.GEN_NONNATIVE_ADD, t.GEN_NONNATIVE_SUB, t.GEN_NONNATIVE_MUL, t.GEN_NONNATIVE_INV) == (2, 3, 4, 5)
    assert {k: v[0] for k, v in t.NONNATIVE_FIELDS.items()} == pkg.prover.WitnessPlan.NONNATIVE_FIELDS == {"secp256k1_base": 0, "secp256k1_scalar": 1}
    assert t.NONNATIVE_FIELDS["secp256k1_base"][1] == 2**256 - 2**32 - 977
    assert t.NONNATIVE_FIELDS["secp256k1_scalar"][1] == 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141


def test_kind_words(pkg):
    """(kind, groups, field) -> kind | field << 8; two-element tuples keep meaning what they mean; GENERATOR_KINDS is untouched."""
    wp = pkg.prover.WitnessPlan
    assert wp.GENERATOR_KINDS == {"equality": 0, "biguint_divrem": 1}
    assert wp.NONNATIVE_KINDS == {"nonnative_add": 2, "nonnative_sub": 3, "nonnative_mul": 4, "nonnative_inv": 5}
    word = wp._kind_word
    assert word(("nonnative_add", (), "secp256k1_base")) == 2 and word(("nonnative_inv", (), "secp256k1_scalar")) == 5 | 1 << 8
    assert word(("nonnative_mul", (), 1)) == 4 | 1 << 8 and word((4, (), 7)) == 4 | 7 << 8
    assert word(("equality", ())) == 0 and word(("biguint_divrem", ())) == 1 and word((7, ())) == 7 and word(("nonnative_sub", ())) == 3
    for bad in (("nonnative_pow", (), "secp256k1_base"), ("nonnative_add", (), "bn254"), ("nonnative_pow", ())):
        with pytest.raises(pkg.P2GpuError) as e:
            word(bad)
        assert e.value.code == E_ARG


def test_null_arguments_need_no_device(pkg):
    lib = pkg.load_library()
    out = ctypes.c_void_p(1)
    cells = np.zeros((32, 2), dtype=np.uint32)
    for rec in ([2, 8, 8, 8, 1], [3 | 1 << 8, 0, 8, 8, 1], [4, 8, 8, 8, 8], [5 | 1 << 8, 8, 0, 8, 8]):
        recs = np.array([rec], dtype=np.uint32)
        for make in (lib.p2gpu_witness_plan_create_genv, lib.p2gpu_witness_plan_build_genv):
            out.value = 1
            assert make(None, None, 0, recs.ctypes.data, 1, cells.ctypes.data, sum(rec[1:]), ctypes.byref(out)) == E_ARG and not out.value
            assert make(None, None, 0, recs.ctypes.data, 1, cells.ctypes.data, sum(rec[1:]), None) == E_ARG
