"""build() on the device (p2gpu_circuit_build, csrc/build.hip) on the MI355X: gate rows + copy pairs -> prover handle, with
no blob in host memory.  The expected bytes always come from the host build (p2gpu_build_blob, itself pinned to the
oracle's orc_build_blob and to the reference's circuits by tests/test_build.py) and from the oracle's proofs."""
import ctypes
import hashlib
import sys
import threading

import numpy as np
import pytest

from conftest import GOLDEN, P

sys.path.insert(0, GOLDEN)
import param_circuits as pc  # noqa: E402
import reference_proofs as rp  # noqa: E402
import device_build_inputs as dbi  # noqa: E402
from test_device_build import PARAM_SHAPES, param_circuit  # noqa: E402

pytestmark = pytest.mark.gpu
E_ARG = -7


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


def _no_hip_error():
    import torch

    torch.cuda.synchronize()   # raises if a kernel of this process faulted


def check_blob_parity(pkg, orc, blob, hashers=(0, 1)):
    """export_blob(build(inputs)) == p2gpu_build_blob(inputs) == orc_build_blob(inputs), word 22 = the hasher."""
    kw = dbi.decompose(pkg, blob)
    host = pkg.build_blob(**kw)
    if int(blob[:256].view(np.uint32)[25]) == 0:
        assert dbi.with_hasher(host, 0).tobytes() == dbi.with_hasher(blob, 0).tobytes()
    bp, gd = dbi.raw_build_args(kw)
    fn = pc.build_fn(orc.lib().orc_build_blob)
    ln = ctypes.c_size_t(len(host))
    out = np.zeros(len(host), dtype=np.uint8)
    cp, rc = kw["copies"], kw["row_constants"]
    assert fn(ctypes.addressof(bp), ctypes.addressof(gd), len(kw["gates"]), kw["row_gate"].ctypes.data, rc.ctypes.data if rc.size else None,
              cp.ctypes.data if cp.size else None, len(cp), out.ctypes.data, ctypes.byref(ln)) == 0
    assert out.tobytes() == host.tobytes()
    for hasher in hashers:
        cd = pkg.CircuitData.build(hasher=hasher, **kw)
        got = cd.to_blob()
        cd.close()
        assert got.tobytes() == dbi.with_hasher(host, hasher).tobytes(), f"hasher {hasher}"
    return kw, host


@pytest.mark.parametrize("d,mix,npi,nw", [(5, "arith", 0, 234), (7, "ecdsa", 0, 234), (8, "ecdsa", 9, 234), (9, "sha", 4, 135), (11, "ecdsa", 0, 234)])
def test_blob_parity_workload_generator(pkg, orc, gpu, d, mix, npi, nw):
    check_blob_parity(pkg, orc, pkg.make_circuit(d, mix, 77, num_public_inputs=npi, num_wires=nw)[0])


@pytest.mark.parametrize("name", ["basic_if", "basic_div"])
def test_blob_parity_reference_circuits(pkg, orc, gpu, name):
    """plonky2's own build() output, recovered from the reference's proof files (basic_div: two selector groups)."""
    blob = rp.ReferenceCase(name).blob()
    _, host = check_blob_parity(pkg, orc, blob)
    assert host.tobytes() == blob.tobytes()


@pytest.mark.parametrize("shape", PARAM_SHAPES, ids=["_".join(str(x) for x in s) for s in PARAM_SHAPES])
def test_blob_parity_off_the_reference_shape(pkg, orc, gpu, shape):
    check_blob_parity(pkg, orc, param_circuit(pkg, orc, shape)[0])


@pytest.mark.parametrize("d,mix", [(13, "arith"), (15, "ecdsa"), (17, "sha")])
def test_blob_parity_large(pkg, orc, gpu, d, mix):
    check_blob_parity(pkg, orc, pkg.make_circuit(d, mix, 77)[0])


def _handles(pkg, blob, hasher):
    kw = dbi.decompose(pkg, blob)
    built = pkg.CircuitData.build(hasher=hasher, **kw)
    created = pkg.CircuitData(dbi.with_hasher(pkg.build_blob(**kw), hasher))
    return built, created


@pytest.mark.parametrize("hasher", [0, 1])
@pytest.mark.parametrize("d,mix,npi", [(9, "ecdsa", 0), (12, "sha", 3)])
def test_handle_parity_and_proofs(pkg, orc, gpu, d, mix, npi, hasher):
    """cap, digest and verifier key equal those of p2gpu_circuit_create(blob); p2gpu_prove, _dev and _routed give the
    oracle's bytes for the same witness."""
    import torch

    out = pkg.make_circuit(d, mix, 41, num_public_inputs=npi, pi_row_routed_only=True, hasher=hasher)
    blob, wires = out[0], out[1]
    pis = out[2] if npi else ()
    built, created = _handles(pkg, blob, hasher)
    oc = orc.OracleCircuit(blob)
    assert built.constants_sigmas_cap() == created.constants_sigmas_cap() == oc.cap()
    assert built.circuit_digest() == created.circuit_digest()
    assert bytes(built.verifier_blob()) == bytes(created.verifier_blob())
    assert built.hash_bytes() == created.hash_bytes() == (32 if hasher else 25)
    want = oc.prove(wires, public_inputs=pis)[0]
    assert built.prove(wires, public_inputs=pis).to_bytes() == want
    wd = torch.from_numpy(wires.view(np.int64)).cuda()
    assert built.prove(wd, public_inputs=pis).to_bytes() == want
    assert built.prove_routed(np.ascontiguousarray(wires[:80]), public_inputs=pis).to_bytes() == want
    built.verify(want)
    assert created.prove(wires, public_inputs=pis).to_bytes() == want
    built.close()
    created.close()


@pytest.mark.parametrize("shape", [PARAM_SHAPES[2], PARAM_SHAPES[5]], ids=["rate2_K1", "rate1_K1"])
def test_handle_parity_off_the_reference_shape(pkg, orc, gpu, shape):
    blob, wires = param_circuit(pkg, orc, shape)
    built, created = _handles(pkg, blob, 0)
    oc = orc.OracleCircuit(blob)
    assert built.constants_sigmas_cap() == created.constants_sigmas_cap() == oc.cap()
    assert built.circuit_digest() == created.circuit_digest()
    want = oc.prove(wires)[0]
    assert built.prove(wires).to_bytes() == want
    built.close()
    created.close()


STRESS = dbi.stress_copy_sets()


@pytest.mark.parametrize("name", sorted(STRESS))
def test_copy_sets_that_stress_the_union_find(pkg, gpu, name):
    d, copies = STRESS[name]
    kw = dbi.noop_circuit(d, copies)
    host = pkg.build_blob(**kw)
    cd = pkg.CircuitData.build(**kw)
    got = cd.to_blob()
    cd.close()
    assert got.tobytes() == host.tobytes()
    _no_hip_error()


def test_determinism_from_two_host_threads(pkg, gpu):
    """The same input built eight times, four times each from two host threads at once: one SHA-256."""
    blob = pkg.make_circuit(13, "ecdsa", 5)[0]
    kw = dbi.decompose(pkg, blob)
    sums = [[], []]
    errs = []

    def work(i):
        try:
            for _ in range(4):
                cd = pkg.CircuitData.build(device=0, **kw)
                sums[i].append(hashlib.sha256(cd.to_blob().tobytes() + cd.constants_sigmas_cap() + cd.circuit_digest()).hexdigest())
                cd.close()
        except Exception as e:  # noqa: BLE001
            errs.append(e)
    th = [threading.Thread(target=work, args=(i,)) for i in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    assert len(sums[0]) == 4 and len(sums[1]) == 4 and len(set(sums[0] + sums[1])) == 1
    created = pkg.CircuitData(blob)
    assert sums[0][0] == hashlib.sha256(blob.tobytes() + created.constants_sigmas_cap() + created.circuit_digest()).hexdigest()
    created.close()


def test_refusals(pkg, orc, gpu):
    """The inputs p2gpu_build_blob refuses are refused with P2GPU_E_ARG before anything indexes with them; *out is NULL;
    a following valid build on the same device succeeds and proves; no HIP error is reported."""
    out = pkg.make_circuit(6, "ecdsa", 1)
    blob, wires = out[0], out[1]
    kw = dbi.decompose(pkg, blob)
    n, R = 1 << kw["degree_bits"], kw["num_routed_wires"]
    lib = pkg.load_library()
    want = orc.OracleCircuit(blob).prove(wires)[0]

    def bad(**change):
        k = dict(kw, **change)
        bp, gd = dbi.raw_build_args(k)
        rc, cp = k["row_constants"], k["copies"]
        h = ctypes.c_void_p(0xDEAD)
        code = lib.p2gpu_circuit_build(ctypes.addressof(bp), ctypes.addressof(gd), len(k["gates"]), k["row_gate"].ctypes.data,
                                       rc.ctypes.data if rc is not None else None, cp.ctypes.data, len(cp), 0, ctypes.byref(h))
        msg = lib.p2gpu_last_error().decode()
        assert code == E_ARG and not h.value, (change.keys(), code, msg)
        with pytest.raises(pkg.P2GpuError):         # the host build refuses the same input
            pkg.build_blob(**dict(k, row_constants=rc if rc is not None else np.zeros((0, n), dtype=np.uint64)))
        _no_hip_error()
        good = pkg.CircuitData.build(**kw)
        assert good.prove(wires).to_bytes() == want
        good.close()
        return msg

    rg = kw["row_gate"].copy()
    rg[3] = 99
    assert "row 3 holds gate index 99" in bad(row_gate=rg)
    rg = kw["row_gate"].copy()
    rg[n - 1] = len(kw["gates"])
    assert f"row {n - 1} holds gate index" in bad(row_gate=rg)
    cp = kw["copies"].copy()
    cp[0, 1] = 200
    assert "copy constraint 0 " in bad(copies=cp)
    cp = kw["copies"].copy()
    cp[5, 3] = R
    assert "copy constraint 5 " in bad(copies=cp)
    cp = kw["copies"].copy()
    cp[len(cp) - 1, 2] = n
    assert f"copy constraint {len(cp) - 1} " in bad(copies=cp)
    cp = kw["copies"].copy()
    cp[7, 0] = 0xFFFFFFFF
    assert "copy constraint 7 " in bad(copies=cp)
    rc = kw["row_constants"].copy()
    rc[1, 5] = P
    assert "gate constant (1, 5)" in bad(row_constants=rc)
    rc = kw["row_constants"].copy()
    rc[0, 0] = 0xFFFFFFFFFFFFFFFF
    assert "gate constant (0, 0)" in bad(row_constants=rc)
    bad(row_constants=None)


@pytest.mark.parametrize("ids", [(0, 0), (0, 0, 0, 0)])
def test_device_group(pkg, orc, gpu, ids):
    """After p2gpu_init with several ids the built handle is a device group (every rank runs the build itself) and one
    proof is sharded over it.  Shape as in test_gpu_parity.test_single_process_device_group."""
    import torch

    try:
        pkg.init(list(ids))
        for d, mix, npi in ((9, "ecdsa", 0), (12, "sha", 3)):
            out = pkg.make_circuit(d, mix, 41, num_public_inputs=npi, pi_row_routed_only=True)
            blob, wires = out[0], out[1]
            pis = out[2] if npi else ()
            want = orc.OracleCircuit(blob).prove(wires, public_inputs=pis)[0]
            kw = dbi.decompose(pkg, blob)
            cd = pkg.CircuitData.build(**kw)
            assert cd.to_blob().tobytes() == blob.tobytes()
            assert cd.prove(wires, public_inputs=pis).to_bytes() == want
            wd = torch.from_numpy(wires.view(np.int64)).cuda()
            assert cd.prove(wd, public_inputs=pis).to_bytes() == want
            assert cd.prove_routed(np.ascontiguousarray(wires[:80]), public_inputs=pis).to_bytes() == want
            plain = pkg.CircuitData.build(device=0, **kw)      # a plain handle next to the group
            assert plain.prove(wires, public_inputs=pis).to_bytes() == want
            with pytest.raises(pkg.P2GpuError):
                pkg.CircuitData.build(device=5, **kw)
            plain.close()
            cd.close()
    finally:
        pkg.init([0])


def test_memory(pkg, gpu):
    """A built handle holds the resident bytes of a created one (the scratch of the build is gone), and ten build /
    destroy cycles return every byte."""
    import torch

    blob = pkg.make_circuit(14, "sha", 3)[0]
    kw = dbi.decompose(pkg, blob)
    granule = 2 << 20          # the HIP runtime hands out device memory in 2 MiB pieces
    for _ in range(2):          # (first round: whatever the runtime allocates once per process)
        pkg.CircuitData.build(**kw).close()
        pkg.CircuitData(blob).close()
    torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    created = pkg.CircuitData(blob)
    used_created = free0 - torch.cuda.mem_get_info()[0]
    created.close()
    assert torch.cuda.mem_get_info()[0] == free0
    built = pkg.CircuitData.build(**kw)
    used_built = free0 - torch.cuda.mem_get_info()[0]
    built.close()
    print(f"resident bytes: created {used_created}, built {used_built}")
    assert abs(used_built - used_created) <= granule
    for _ in range(10):
        pkg.CircuitData.build(**kw).close()
    assert torch.cuda.mem_get_info()[0] == free0
