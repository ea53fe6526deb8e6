"""p2gpu_verify_batch_compressed and p2gpu_proof_decompress_batch on the MI355X: the decompression core as kernels
(csrc/decompressdev.hip) against the host's lone decompressor byte for byte (p2gpu_proof_decompress, csrc/proofio.hip) and
against the same core in the host loop report for report (p2gpu_verify_batch_compressed_host), on compressed proofs of the GPU
prover and on the reference's own proof files: every circuit shape of the host tests with the whole mutation list in one
batch, both kinds of handle, the wave edge of the lane-per-proof kernel, members of different lengths, and a batch nothing of
which is uploaded."""
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

import verify_batch_cases as vb
import verify_cbatch_cases as vcb
from conftest import GOLDEN

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


class Case:
    """A synthetic circuit on the GPU, its proof from the GPU prover and that proof compressed, a verifier-only handle."""

    def __init__(self, pkg, d, mix, seed, npi=0, nw=234, hasher=0):
        out = pkg.make_circuit(d, mix, seed, num_public_inputs=npi, num_wires=nw, hasher=hasher)
        self.blob, self.wires, self.pis = out[0], out[1], (out[2] if npi else ())
        self.cd = pkg.CircuitData(self.blob)
        self.vd = self.cd.verifier_data()
        self.proof = self.cd.prove(self.wires, self.pis).to_bytes()
        self.comp = self.vd.compress(self.proof)
        self.L = vb.Layout(self.vd.to_bytes())


@pytest.fixture(scope="module")
def sha6(pkg, gpu):
    return Case(pkg, 6, "sha", 2)


def same_as_host(pkg, handle, batch):
    """Both entry points on the same bytes: everything a caller can see is equal.  Returns the reports."""
    lib = pkg.load_library()
    dev = vcb.raw_cbatch(lib, handle, batch, device=True)
    host = vcb.raw_cbatch(lib, handle, batch, device=False)
    assert dev == host, [(i, a, b) for i, (a, b) in enumerate(zip(dev[1], host[1])) if a != b][:5] + [dev[0], host[0], dev[2], host[2]]
    return dev[1]


def lone_decompress_all(lib, handle, datas):
    """{bytes: (return code, bytes or None)} of the lone p2gpu_proof_decompress, each distinct member once, on a few threads
    (the host's Poseidon is slow; the library's error state is per thread)."""
    distinct = list(dict.fromkeys(datas))
    with ThreadPoolExecutor(8) as pool:
        return dict(zip(distinct, pool.map(lambda data: vcb.lone_decompress(lib, handle, data), distinct)))


def bytes_as_lone(pkg, handle, batch, want, alone=None):
    """p2gpu_proof_decompress_batch: per member the lone call's return code, its bytes where that is 0, zeros elsewhere."""
    lib = pkg.load_library()
    alone = alone or lone_decompress_all(lib, handle, batch)
    rc, status, outs = vcb.raw_decompress_batch(lib, handle, batch, want)
    assert rc == 0, (rc, lib.p2gpu_last_error())
    for i, data in enumerate(batch):
        lrc, lone = alone[data]
        assert status[i] == lrc, (i, status[i], lrc)
        assert outs[i] == (lone if lrc == 0 else bytes(want)), i
    return status


@pytest.mark.parametrize("d,mix,seed,npi,nw,hasher", vb.CIRCUITS)
def test_circuits(pkg, orc, gpu, d, mix, seed, npi, nw, hasher):
    c = Case(pkg, d, mix, seed, npi, nw, hasher)
    oc = orc.OracleCircuit(c.blob)
    comp, muts = vcb.mutations(c.vd, oc, c.wires, c.pis, c.proof)
    assert comp == c.comp
    lib = pkg.load_library()
    batch = vb.interleaved(comp, muts)
    alone = lone_decompress_all(lib, c.vd._h, batch)
    status = bytes_as_lone(pkg, c.vd._h, batch, c.L.want, alone)
    assert all(s == 0 for s in status[0::2]) and sum(1 for s in status[1::2] if s == 0) > 20      # (what only the verifier rejects)
    # The host loop once over the distinct members (untouched, mutation 0, mutation 1, ...): a report depends on the member's
    # bytes alone, and in both orders the lowest failing proof is mutation 0 at place 1, so the call's code and error are equal too.
    distinct = [comp] + [m for _, m in muts]
    rc, host, err = vcb.raw_cbatch(lib, c.vd._h, distinct, device=False)
    by_bytes = dict(zip(distinct, host))
    assert by_bytes[comp] == (0, 0, vcb.NONE, vcb.NONE) and all(r[0] == -9 for r in host[1:]) and rc == -9
    want = (rc, [by_bytes[data] for data in batch], err)
    for handle in (c.vd._h, c.cd._h):
        dev = vcb.raw_cbatch(lib, handle, batch, device=True)
        assert dev == want, [(i, a, b) for i, (a, b) in enumerate(zip(dev[1], want[1])) if a != b][:5] + [dev[0], rc, dev[2], err]
    assert bytes_as_lone(pkg, c.cd._h, batch[:5], c.L.want, alone) == status[:5]
    assert c.cd.prove(c.wires, c.pis).to_bytes() == c.proof       # the prover handle proves the same bytes afterwards


def test_reference_proof_files(pkg, gpu):
    """The reference's own compressed proofs (no fold step): the device's bytes are the host decompressor's, and accepted."""
    sys.path.insert(0, GOLDEN)
    import reference_proofs as rp

    for name in ("basic_if", "basic_div"):
        c = rp.ReferenceCase(name)
        cd = pkg.CircuitData(c.blob())
        vd = cd.verifier_data()
        ref = vd.decompress(c.compressed).to_bytes()
        bad = vb.flip(c.compressed, len(c.compressed) - 9)
        for h in (cd, vd):
            out = h.decompress_batch([c.compressed, bad, c.compressed])
            assert out[0].to_bytes() == ref and out[2].to_bytes() == ref
            reports = h.verify_batch_compressed([c.compressed, bad, c.compressed])
            assert [r.ok for r in reports] == [True, False, True]
        assert same_as_host(pkg, vd._h, [c.compressed, bad, c.compressed])[1][0] == -9
        cd.close()


@pytest.mark.parametrize("size", [1, 65])
def test_batch_sizes(pkg, sha6, size):
    """One member, and the second wave's first lane of the lane-per-proof kernel."""
    c = sha6
    w = vcb.Walk(c.vd.to_bytes(), c.comp)
    bad = vb.flip(c.comp, w.init[w.idx[5]][3][0] + 8)           # a quotient leaf word of query 5's entry
    at = sorted({0, size - 1})
    batch = [bad if i in at else c.comp for i in range(size)]
    reports = same_as_host(pkg, c.vd._h, batch)
    # (the query named is the lowest whose rebuilt path hangs on that leaf's digest: query 5 or one before it)
    assert [i for i, r in enumerate(reports) if r[0]] == at and all(r[:2] == (-9, 10) and r[2] <= 5 and r[3] == 3 for r in (reports[i] for i in at))
    good = [c.comp] * size
    assert same_as_host(pkg, c.vd._h, good) == [(0, 0, vcb.NONE, vcb.NONE)] * size
    outs = c.vd.decompress_batch(good)
    assert all(o.to_bytes() == c.proof for o in outs)


def test_members_of_different_lengths(pkg, sha6):
    """Proofs of different witnesses have different query indices, so different sets of kept siblings and different lengths;
    walk failures and a rejection sit among them, and the members around them are still accepted."""
    c = sha6
    comps = [c.comp]
    for row in (7, 30, 55):
        w = c.wires.copy()
        w[233, row] = (int(w[233, row]) + 1 + row) % vb.P
        comps.append(c.vd.compress(c.cd.prove(w, c.pis).to_bytes()))
    assert len({len(x) for x in comps}) > 1
    batch = comps[:2] + [c.comp[:-1], vb.flip(comps[2], c.L.open_at + 3), b""] + comps[2:] + [c.comp + b"\0"]
    reports = same_as_host(pkg, c.vd._h, batch)
    # (a changed opening moves every later challenge: the stored indices are no longer the transcript's)
    assert [r[0] for r in reports] == [0, 0, -9, -9, -9, 0, 0, -9] and [r[1] for r in reports] == [0, 0, 21, 23, 17, 0, 0, 21]
    bytes_as_lone(pkg, c.vd._h, batch, c.L.want)
    outs = c.vd.decompress_batch(batch)
    assert [isinstance(o, pkg.P2GpuError) for o in outs] == [False, False, True, True, True, False, False, True]
    assert outs[2].code == -9 and "final polynomial / length" in str(outs[2]) and "differ from the transcript" in str(outs[3])
    assert outs[0].to_bytes() == c.proof and len({o.to_bytes() for o in outs if not isinstance(o, pkg.P2GpuError)}) == 4


def test_nothing_is_uploaded(pkg, sha6):
    """Every member fails the host's walk: every verdict from the lone path, no launch -- on both kinds of handle."""
    c = sha6
    w = vcb.Walk(c.vd.to_bytes(), c.comp)
    batch = [c.comp[:-1], b"", c.comp + b"\0", c.comp[:100], vcb.put(c.comp, w.idx_at, (1 << w.lgN).to_bytes(4, "little"))]
    for h in (c.cd._h, c.vd._h):
        assert [r[1] for r in same_as_host(pkg, h, batch)] == [21, 17, 21, 17, 18]
        assert bytes_as_lone(pkg, h, batch, c.L.want) == [-9] * 5
