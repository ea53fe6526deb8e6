"""Inputs of the batched prover's GPU tests (test infrastructure): the circuit shapes with their synth matrices, the
less-or-equal circuit with one witness per public input, and the raw call with everything a caller can see."""
import ctypes

import numpy as np

import memory_ops_inputs as moi
import witness_gen_inputs as wgi

BOUND = 8    # the one public input of memory_ops_inputs.less_or_equal_circuit may be 0 .. BOUND

# (name, degree_bits, mix, public inputs, wires, hasher); the two translated programs come from witness_gen_inputs
SHAPES = [("fibonacci", 2, None, 0, 234, 0), ("quadratic", 3, None, 0, 234, 0), ("arith5", 5, "arith", 0, 234, 0), ("sha6", 6, "sha", 0, 234, 0),
          ("ecdsa8", 8, "ecdsa", 2, 234, 0), ("arith7_135", 7, "arith", 1, 135, 0), ("sha10", 10, "sha", 0, 234, 0),
          ("sha6_poseidon", 6, "sha", 0, 234, 1), ("ecdsa8_poseidon", 8, "ecdsa", 2, 234, 1), ("arith12", 12, "arith", 0, 234, 0)]


def shape(pkg, name, d, mix, npi, nw, hasher):
    """(blob, wires [W][n] uint64, public inputs) of one shape."""
    if mix is None:
        prog = wgi.FIBONACCI if name == "fibonacci" else wgi.QUADRATIC
        cb = wgi.translated(pkg, prog)
        blob, wires = cb.build(prog["witness"])
        assert int(np.frombuffer(bytes(blob[:256]), dtype=np.uint32)[2]) == d
        return blob, wires, ()
    out = pkg.make_circuit(d, mix, seed=5, num_public_inputs=npi, num_wires=nw, hasher=hasher)
    return out[0], out[1], (list(int(v) for v in out[2]) if npi else ())


def less_or_equal(pkg):
    """(blob, {value: wires}) for the values 0 .. BOUND, each its own public input."""
    b, _ = moi.less_or_equal_circuit(pkg, BOUND)
    blob = b.blob()
    mats = {}
    for value in range(BOUND + 1):
        bb, tt = moi.less_or_equal_circuit(pkg, BOUND)
        _, wires = bb.build({tt: value})
        mats[value] = wires
    return blob, mats


def stacked(mats, device):
    """[B][W][n] int64 tensor on the GPU from uint64 matrices."""
    import torch

    return torch.from_numpy(np.ascontiguousarray(np.stack(mats)).view(np.int64)).to(device)


def raw(pkg, cd, wires_dev, pis):
    """p2gpu_prove_batch_dev as it is: (return code, [status], [proof bytes], p2gpu_last_error)."""
    import torch

    lib = pkg.load_library()
    batch = wires_dev.shape[0]
    p = np.ascontiguousarray(np.array([list(x) for x in pis], dtype=np.uint64).reshape(batch, -1))
    out = np.full((batch, cd._bound), 0xA5, dtype=np.uint8)
    st = np.full(batch, 99, dtype=np.intc)
    torch.cuda.synchronize()
    rc = lib.p2gpu_prove_batch_dev(cd._h, ctypes.c_void_p(wires_dev.data_ptr()), batch, p.ctypes.data, p.shape[1], out.ctypes.data, st.ctypes.data)
    return rc, [int(s) for s in st], [out[b].tobytes() for b in range(batch)], lib.p2gpu_last_error().decode()
