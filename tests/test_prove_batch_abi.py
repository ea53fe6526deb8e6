"""The batched prover's public surface, without a device: p2gpu_prove_batch_dev / p2gpu_prove_seeds_batch in the library and the
header, the degree limit the header states against the one the library enforces, the refusals that need no device -- each
with words of its own --, and the Python entry points."""
import ctypes
import inspect
import os
import re

import numpy as np

E_ARG = -7
P = 0xFFFFFFFF00000001
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_text():
    with open(os.path.join(ROOT, "include", "p2gpu.h")) as f:
        return f.read()


def _verifier_only(pkg, npi):
    """A verifier-only handle made without a device (cap and digest zero: nothing looks at them before a proof does)."""
    out = pkg.make_circuit(8, "ecdsa", seed=1, num_public_inputs=npi)
    blob = out[0]
    h = blob[:256].copy().view(np.uint32)
    ng, R, cap_h = int(h[23]), int(h[4]), int(h[10])
    h[25] = 3
    vk = h.tobytes() + blob[256:256 + 48 * ng].tobytes() + bytes(32 << cap_h) + blob[256 + 48 * ng:256 + 48 * ng + 8 * R].tobytes()
    return pkg.VerifierCircuitData(vk)


def test_symbols_and_header_signatures(pkg):
    lib = pkg.load_library()
    for name in ("p2gpu_prove_batch_dev", "p2gpu_prove_seeds_batch", "p2gpu_prove_batch_max_degree_bits", "p2gpu_prove_batch_info"):
        assert hasattr(lib, name), name
    flat = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", " ", _header_text(), flags=re.S))
    assert ("int p2gpu_prove_batch_dev(p2gpu_circuit *c, const uint64_t *wires_dev, size_t batch, const uint64_t *public_inputs, "
            "uint32_t n_pi, uint8_t *proofs_out, int *status);") in flat
    assert ("int p2gpu_prove_seeds_batch(p2gpu_witness_plan *p, const uint64_t *seed_values , size_t batch, const uint64_t "
            "*public_inputs, uint32_t n_pi, uint8_t *proofs_out, int *status, uint32_t *bad_cells );") in flat


def test_the_limit_in_the_header_is_the_one_enforced(pkg):
    m = re.search(r"^#define P2GPU_PROVE_BATCH_MAX_DEGREE_BITS (\d+)$", _header_text(), flags=re.M)
    assert m and int(m.group(1)) == 12
    assert pkg.load_library().p2gpu_prove_batch_max_degree_bits() == 12


def test_refusals_need_no_device(pkg):
    """Null arguments, batch == 0, a wrong n_pi, a public input >= p and the verifier-only handle itself: P2GPU_E_ARG, each with
    its own words (a verifier-only handle holds no device, so none can have been touched)."""
    lib = pkg.load_library()
    vd = _verifier_only(pkg, 2)
    try:
        h, one = vd._h, ctypes.c_void_p(8)        # (never dereferenced: refused first)
        out = np.zeros(16, dtype=np.uint8)
        st = np.zeros(2, dtype=np.intc)
        good = np.array([[1, 2], [3, 4]], dtype=np.uint64)
        bad = np.array([[1, 2], [3, P]], dtype=np.uint64)
        call = lambda *a: (lib.p2gpu_prove_batch_dev(*a), lib.p2gpu_last_error().decode())   # noqa: E731
        seen = []
        for args, words in (((None, one, 2, good.ctypes.data, 2, out.ctypes.data, st.ctypes.data), "null handle"),
                            ((h, None, 2, good.ctypes.data, 2, out.ctypes.data, st.ctypes.data), "null witness matrix"),
                            ((h, one, 2, good.ctypes.data, 2, None, st.ctypes.data), "null proof buffer"),
                            ((h, one, 2, good.ctypes.data, 2, out.ctypes.data, None), "null status array"),
                            ((h, one, 0, good.ctypes.data, 2, out.ctypes.data, st.ctypes.data), "batch == 0"),
                            ((h, one, 2, good.ctypes.data, 1, out.ctypes.data, st.ctypes.data), "expected 2 public inputs per witness, got 1"),
                            ((h, one, 2, None, 2, out.ctypes.data, st.ctypes.data), "expected 2 public inputs"),
                            ((h, one, 2, bad.ctypes.data, 2, out.ctypes.data, st.ctypes.data), "witness 1 of the batch: public input 1 is not a canonical"),
                            ((h, one, 2, good.ctypes.data, 2, out.ctypes.data, st.ctypes.data), "verifier-only")):
            rc, err = call(*args)
            assert rc == E_ARG and words in err, (words, rc, err)
            seen.append(err)
        assert len(set(seen)) == len(seen)        # every refusal speaks for itself
        assert not out.any() and not st.any()
        assert lib.p2gpu_prove_seeds_batch(None, None, 1, None, 0, out.ctypes.data, st.ctypes.data, None) == E_ARG
        assert "null plan" in lib.p2gpu_last_error().decode()
        info = np.ones(4, dtype=np.uint64)
        assert lib.p2gpu_prove_batch_info(h, info.ctypes.data) == 0 and info[0] == 0 and info[2] == 0 and info[3] > 0
    finally:
        vd.close()


def test_python_entry_points(pkg):
    sig = inspect.signature(pkg.prover.CircuitData.prove_batch)
    assert list(sig.parameters)[1:] == ["wires", "public_inputs"] and sig.parameters["public_inputs"].default is None
    sig = inspect.signature(pkg.prover.WitnessPlan.prove_batch)
    assert list(sig.parameters)[1:] == ["values_list", "public_inputs", "verify", "one_call"]
    assert sig.parameters["one_call"].default is False and sig.parameters["verify"].default is False
