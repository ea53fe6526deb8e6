"""The public surface of the generators with any number of cells, without a device: the three entry points in the library and
the header, their argument refusals, and what WitnessPlan makes of a generator list."""
import ctypes
import os
import re

import numpy as np

E_ARG = -7
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_symbols_and_header_signatures(pkg):
    lib = pkg.load_library()
    with open(os.path.join(ROOT, "include", "p2gpu.h")) as f:
        flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", f.read(), flags=re.S))
    flat = re.sub(r" ?([(),;*]) ?", r"\1", flat)        # (no blanks around punctuation: where a comment stood does not matter)
    for name in ("create", "build"):
        assert hasattr(lib, "p2gpu_witness_plan_%s_genv" % name)
        assert ("int p2gpu_witness_plan_%s_genv(p2gpu_circuit*c,const uint32_t*seed_cells,size_t n_seeds,const p2gpu_generator_v"
                "*generators,size_t n_generators,const uint32_t*cells,size_t n_cells,p2gpu_witness_plan**out);" % name) in flat
    assert hasattr(lib, "p2gpu_witness_plan_export_generators_v")
    assert "int p2gpu_witness_plan_export_generators_v(const p2gpu_witness_plan*p,uint32_t*off,uint32_t*table,size_t sizes[2]);" in flat
    assert "#define P2GPU_GEN_BIGUINT_DIVREM 1" in flat and "typedef struct { uint32_t kind;uint32_t shape[4];} p2gpu_generator_v;" in flat
    with open(os.path.join(ROOT, "acvm-backend-plonky2_amd", "csrc", "genops.hpp")) as f:
        assert "OP_BIGUINT_DIVREM == 14" in f.read()
    assert pkg.prover.WitnessPlan.GENERATOR_KINDS == {"equality": 0, "biguint_divrem": 1}
    assert pkg.translate.GEN_BIGUINT_DIVREM == 1 and callable(pkg.prover.WitnessPlan.export_generators_v)


def test_null_arguments_need_no_device(pkg):
    lib = pkg.load_library()
    out = ctypes.c_void_p(1)
    recs = np.array([[1, 1, 1, 1, 1]], dtype=np.uint32)
    cells = np.zeros((4, 2), dtype=np.uint32)
    for make in (lib.p2gpu_witness_plan_create_genv, lib.p2gpu_witness_plan_build_genv):
        out.value = 1
        assert make(None, None, 0, recs.ctypes.data, 1, cells.ctypes.data, 4, ctypes.byref(out)) == E_ARG and not out.value
        assert make(None, None, 0, None, 0, None, 0, None) == E_ARG
    sizes = (ctypes.c_size_t * 2)()
    assert lib.p2gpu_witness_plan_export_generators_v(None, None, None, sizes) == E_ARG


def test_generator_groups(pkg):
    """Four plain cells stay a four-cell record; four groups of cells are a shape and a flat list."""
    groups = pkg.prover.WitnessPlan._groups
    assert groups(((1, 2), (3, 4), (5, 6), (7, 8))) is None
    assert groups((((1, 2), (3, 4)), ((5, 6),), ((7, 8), (9, 10)), ((11, 12),))) == [[(1, 2), (3, 4)], [(5, 6)], [(7, 8), (9, 10)], [(11, 12)]]
    assert groups((((1, 2),), ((5, 6),), (), ((11, 12),))) == [[(1, 2)], [(5, 6)], [], [(11, 12)]]
