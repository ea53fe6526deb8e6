"""build() on the device (p2gpu_circuit_build, csrc/build.hip), the part that needs no GPU: the C ABI symbols and their
Python mirror, the argument errors found before a device is touched, and p2gpu_build_blob unchanged by the factoring of
the blob prefix (header, gate table, k_is) into the function both build paths call."""
import ctypes
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import param_circuits as pc  # noqa: E402
import device_build_inputs as dbi  # noqa: E402

E_ARG, E_DEVICE = -7, -3


def test_error_codes_are_the_header_s(pkg):
    import os
    import re

    text = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "p2gpu.h")).read()
    assert int(re.search(r"#define P2GPU_E_ARG\s+(-?\d+)", text).group(1)) == E_ARG
    assert int(re.search(r"#define P2GPU_E_DEVICE\s+(-?\d+)", text).group(1)) == E_DEVICE


def test_symbols_and_argtypes(pkg):
    lib = pkg.load_library()
    vp, sz, u32 = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_uint32
    assert lib.p2gpu_circuit_build.argtypes == [vp, vp, u32, vp, vp, vp, sz, u32, ctypes.POINTER(vp)]
    assert lib.p2gpu_circuit_build_on.argtypes == [vp, vp, u32, vp, vp, vp, sz, u32, ctypes.c_int, ctypes.POINTER(vp)]
    assert lib.p2gpu_circuit_export_blob.argtypes == [vp, vp, ctypes.POINTER(sz)]
    assert callable(pkg.CircuitData.build) and callable(pkg.CircuitData.to_blob)


def _call(lib, kw, hasher=0, on=None, **override):
    bp, gd = dbi.raw_build_args(kw)
    rg, rc, cp = kw["row_gate"], kw["row_constants"], kw["copies"]
    args = dict(bp=ctypes.addressof(bp), gd=ctypes.addressof(gd), ng=len(kw["gates"]), rg=rg.ctypes.data, rc=rc.ctypes.data if rc.size else None,
                cp=cp.ctypes.data if cp.size else None, ncp=len(cp))
    args.update(override)
    out = ctypes.c_void_p(0xDEAD)
    pos = [args["bp"], args["gd"], args["ng"], args["rg"], args["rc"], args["cp"], args["ncp"], hasher]
    rc_ = lib.p2gpu_circuit_build(*pos, ctypes.byref(out)) if on is None else lib.p2gpu_circuit_build_on(*pos, on, ctypes.byref(out))
    return rc_, out.value, bp, gd


def _small(pkg):
    kw = dbi.decompose(pkg, pkg.make_circuit(5, "ecdsa", 1)[0])
    return kw


def test_argument_errors_need_no_device(pkg):
    """NULL pointers, no gates, unsorted gates, degree_bits out of range, a gate with constants but no constants array:
    P2GPU_E_ARG and *out = NULL, on a machine with or without a GPU."""
    lib = pkg.load_library()
    kw = _small(pkg)
    for on in (None, 0):
        for bad in (dict(bp=None), dict(gd=None), dict(rg=None), dict(cp=None), dict(ng=0), dict(rc=None)):
            rc, out, *_ = _call(lib, kw, on=on, **bad)
            assert rc == E_ARG and not out, bad
        rc, out, *_ = _call(lib, kw, hasher=2, on=on)
        assert rc == E_ARG and not out
        for dbits in (0, 25):
            rc, out, *_ = _call(lib, dict(kw, degree_bits=dbits), on=on)
            assert rc == E_ARG and not out
        assert len(kw["gates"]) > 1 and kw["gates"][0][2] < kw["gates"][-1][2]
        rc, out, *_ = _call(lib, dict(kw, gates=kw["gates"][::-1]), on=on)
        assert rc == E_ARG and not out
        assert b"sorted" in lib.p2gpu_last_error()
    bp, gd = dbi.raw_build_args(kw)
    assert lib.p2gpu_circuit_build(ctypes.addressof(bp), ctypes.addressof(gd), len(kw["gates"]), kw["row_gate"].ctypes.data,
                                   kw["row_constants"].ctypes.data, kw["copies"].ctypes.data, len(kw["copies"]), 0, None) == E_ARG
    ln = ctypes.c_size_t(0)
    assert lib.p2gpu_circuit_export_blob(None, None, ctypes.byref(ln)) == E_ARG


def test_valid_arguments_need_a_device(pkg):
    """Valid arguments: P2GPU_E_DEVICE where there is no HIP device (the library has no CPU fallback), a handle where there is one."""
    import torch

    lib = pkg.load_library()
    kw = _small(pkg)
    if torch.cuda.is_available():
        cd = pkg.CircuitData.build(**kw)
        assert cd.to_blob().tobytes() == pkg.build_blob(**kw).tobytes()
        cd.close()
        return
    rc, out, *_ = _call(lib, kw)
    assert rc == E_DEVICE and not out
    with pytest.raises(pkg.P2GpuError) as e:
        pkg.CircuitData.build(**kw)
    assert e.value.code == E_DEVICE


def _builders(pkg, orc):
    return [pc.build_fn(pkg.load_library().p2gpu_build_blob), pc.build_fn(orc.lib().orc_build_blob)]


PARAM_SHAPES = [("arith", 9, 80, 234, 1, 3, 4), ("arith", 10, 64, 64, 2, 2, 2), ("arith", 12, 48, 96, 1, 2, 3), ("arith", 9, 40, 80, 2, 2, 6),
                ("degree1", 10, 32, 32, 2, 1, 1), ("degree1", 11, 20, 40, 1, 1, 5)]


def param_circuit(pkg, orc, shape, seed=5):
    gen = pc.arith_circuit if shape[0] == "arith" else pc.degree1_circuit
    return gen(*shape[1:], seed=seed, builders=_builders(pkg, orc))


@pytest.mark.parametrize("shape", PARAM_SHAPES, ids=["_".join(str(x) for x in s) for s in PARAM_SHAPES])
def test_build_blob_unchanged_off_the_reference_shape(pkg, orc, shape):
    """rate_bits 1 / 2 / 3, K = 1 and 2, other R / W / cap heights: the product's p2gpu_build_blob and the oracle's
    orc_build_blob agree byte for byte (param_circuits asserts it), and the blob taken apart and built again is itself."""
    blob, _ = param_circuit(pkg, orc, shape)
    kw = dbi.decompose(pkg, blob)
    assert pkg.build_blob(**kw).tobytes() == blob.tobytes()
    bp, gd = dbi.raw_build_args(kw)
    fn = _builders(pkg, orc)[1]
    ln = ctypes.c_size_t(len(blob))
    out = np.zeros(len(blob), dtype=np.uint8)
    assert fn(ctypes.addressof(bp), ctypes.addressof(gd), len(kw["gates"]), kw["row_gate"].ctypes.data, kw["row_constants"].ctypes.data,
              kw["copies"].ctypes.data if kw["copies"].size else None, len(kw["copies"]), out.ctypes.data, ctypes.byref(ln)) == 0
    assert out.tobytes() == blob.tobytes()


def test_fast_decompose_agrees_with_the_loop(pkg):
    """device_build_inputs.decompose against tests/test_build.py's reference loop: same gate rows, same classes."""
    import test_build as tb

    blob = pkg.make_circuit(7, "ecdsa", 77)[0]
    kw = dbi.decompose(pkg, blob)
    params, gates, ng, row_gate, gconst, copies = tb.decompose(blob)
    assert (kw["row_gate"] == row_gate).all() and (kw["row_constants"] == gconst).all()
    assert sorted(map(tuple, kw["copies"].tolist())) == sorted(map(tuple, copies.tolist()))
    assert pkg.build_blob(**kw).tobytes() == blob.tobytes()


def test_stress_copy_sets_build_on_the_host(pkg, orc):
    """The copy sets of the GPU test are valid inputs: the product's host build and the oracle's agree on each."""
    fns = _builders(pkg, orc)
    for name, (d, copies) in dbi.stress_copy_sets().items():
        kw = dbi.noop_circuit(d, copies)
        a = pkg.build_blob(**kw)
        full = dict(dbi.header_kwargs(a), **kw)
        bp, gd = dbi.raw_build_args(full)
        ln = ctypes.c_size_t(len(a))
        out = np.zeros(len(a), dtype=np.uint8)
        cp = full["copies"]
        assert fns[1](ctypes.addressof(bp), ctypes.addressof(gd), 1, full["row_gate"].ctypes.data, None, cp.ctypes.data if cp.size else None,
                      len(cp), out.ctypes.data, ctypes.byref(ln)) == 0, name
        assert out.tobytes() == a.tobytes(), name
