"""p2gpu_verify_batch on the MI355X: the verifier core as kernels (csrc/verifydev.hip) against the same core in the host loop
(p2gpu_verify_batch_host) on the same bytes -- status, reason, query, index and p2gpu_last_error -- on proofs the GPU prover
made: every circuit shape of the host tests, the targeted mutations in one batch, the wave and block edges of the
lane-per-proof mapping, a deep tree, both kinds of handle, and a batch verified while another thread proves."""
import threading

import numpy as np
import pytest

import memory_ops_inputs as moi
import verify_batch_cases as vb

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


class Case:
    """A synthetic circuit on the GPU, its witness, its proof from the GPU prover, a verifier-only handle of it."""

    def __init__(self, pkg, d, mix, seed, npi=0, nw=234, hasher=0):
        out = pkg.make_circuit(d, mix, seed, num_public_inputs=npi, num_wires=nw, hasher=hasher)
        self.wires, self.pis = out[1], (out[2] if npi else ())
        self.cd = pkg.CircuitData(out[0])
        self.vd = self.cd.verifier_data()
        self.proof = self.cd.prove(self.wires, self.pis).to_bytes()
        self.L = vb.Layout(self.vd.to_bytes())


@pytest.fixture(scope="module")
def sha6(pkg, gpu):
    return Case(pkg, 6, "sha", 2)


@pytest.fixture(scope="module")
def ecdsa8(pkg, gpu):
    return Case(pkg, 8, "ecdsa", 3, npi=2)


def same_as_host(pkg, handle, batch, host_handle=None):
    """Both entry points on the same bytes: everything a caller can see is equal.  Returns the reports."""
    lib = pkg.load_library()
    dev = vb.raw_batch(lib, handle, batch, device=True)
    host = vb.raw_batch(lib, host_handle or handle, batch, device=False)
    assert dev == host, [(i, a, b) for i, (a, b) in enumerate(zip(dev[1], host[1])) if a != b][:5] + [dev[0], host[0], dev[2], host[2]]
    return dev[1]


@pytest.mark.parametrize("d,mix,seed,npi,nw,hasher", vb.CIRCUITS)
def test_circuits(pkg, gpu, d, mix, seed, npi, nw, hasher):
    c = Case(pkg, d, mix, seed, npi, nw, hasher)
    rng = np.random.default_rng(d)
    flips = [vb.flip(c.proof, int(p), int(rng.integers(0, 8))) for p in rng.integers(0, len(c.proof), size=6)]
    reports = same_as_host(pkg, c.vd._h, [c.proof] + flips + [vb.flip(c.proof, 1), c.proof])
    assert reports[0][0] == 0 and reports[-1][0] == 0 and all(r[0] == -9 for r in reports[1:-1])


def test_targeted_mutations_in_one_batch(pkg, ecdsa8):
    c = ecdsa8
    lib = pkg.load_library()
    muts = vb.mutations(lib, c.vd._h, c.proof, c.L)
    batch = vb.interleaved(c.proof, muts)
    reports = same_as_host(pkg, c.vd._h, batch)
    assert all(r[0] == 0 for r in reports[0::2]) and all(r[0] == -9 for r in reports[1::2])
    msgs = [r.message for r in c.vd.verify_batch(batch)]
    assert msgs[1::2] == [vb.lone(lib, c.vd._h, m)[1] for _, m in muts]
    for want in vb.SIX:
        assert any(want in m for m in msgs), want


@pytest.mark.parametrize("size", [1, 63, 64, 65, 257])
def test_batch_sizes(pkg, sha6, size):
    c = sha6
    bad = vb.flip(c.proof, c.L.queries_at + 5 * c.L.query_bytes + c.L.init_at[3] + 8)   # a quotient leaf element of query 5
    at = sorted({p for p in (0, 63, 64, size - 1) if p < size})
    batch = [bad if i in at else c.proof for i in range(size)]
    reports = same_as_host(pkg, c.vd._h, batch)
    assert [i for i, r in enumerate(reports) if r[0]] == at
    assert all(reports[i] == (-9, 10, 5, 3) for i in at)


def test_mixed_batch(pkg, ecdsa8):
    """Proofs of different witnesses of one circuit (the last wire column is free in the synthetic circuits), a proof of
    another circuit and wrong lengths, in one batch."""
    c = ecdsa8
    proofs = [c.proof]
    for row in (7, 100, 255):
        w = c.wires.copy()
        w[233, row] = (int(w[233, row]) + 1 + row) % vb.P
        proofs.append(c.cd.prove(w, c.pis).to_bytes())
    assert len(set(proofs)) == 4
    other = Case(pkg, 8, "ecdsa", 4, npi=2)
    batch = proofs[:2] + [other.proof, c.proof[:-1], b""] + proofs[2:] + [c.proof + b"\0"]
    reports = same_as_host(pkg, c.vd._h, batch)
    assert [r[0] for r in reports] == [0, 0, -9, -9, -9, 0, 0, -9]
    assert reports[3][1] == 3 and reports[4][1] == 1


BOUND = 8    # the one public input of memory_ops_inputs.less_or_equal_circuit may be 0 .. BOUND


@pytest.fixture(scope="module")
def bounded(pkg, gpu):
    """One circuit with a public input the prover chooses: (handle, verifier handle, layout, {value: proof})."""
    b, _ = moi.less_or_equal_circuit(pkg, BOUND)
    cd = pkg.CircuitData(b.blob())
    proofs = {}
    for value in range(BOUND + 1):
        bb, tt = moi.less_or_equal_circuit(pkg, BOUND)
        _, wires = bb.build({tt: value})
        proofs[value] = cd.prove(wires, public_inputs=[value]).to_bytes()
    vd = cd.verifier_data()
    return cd, vd, vb.Layout(vd.to_bytes()), proofs


def test_distinct_public_inputs_in_one_batch(pkg, bounded):
    """The lanes of one wave hash different public inputs, start their transcripts from different hashes and check different
    words for canonicity; a public input swapped for another proof's, a non-canonical one and one above the bound's proof sit
    among them, and every verdict stays with its own proof."""
    cd, vd, L, proofs = bounded
    assert L.num_pi == 1 and len(set(proofs.values())) == BOUND + 1
    for v, p in proofs.items():
        assert int.from_bytes(p[L.pis_at:L.pis_at + 8], "little") == v
    good = [proofs[v] for v in (3, 0, 8, 5, 1, 7, 2, 6, 4)]
    swapped = proofs[5][:L.pis_at] + proofs[6][L.pis_at:]              # proof of 5 that claims 6
    big = proofs[2][:L.pis_at] + (vb.P + 2).to_bytes(8, "little")      # 2 + p: the same field element, not a canonical word
    batch = good[:4] + [swapped] + good[4:7] + [big] + good[7:] + [swapped]
    reports = same_as_host(pkg, vd._h, batch)
    assert [r[0] for r in reports] == [0, 0, 0, 0, -9, 0, 0, 0, -9, 0, 0, -9]
    assert reports[4] == reports[11] == (-9, 6, 0xFFFFFFFF, 0xFFFFFFFF)      # another public-input hash: the identity at zeta fails
    assert reports[8] == (-9, 4, 0xFFFFFFFF, 0xFFFFFFFF)
    assert same_as_host(pkg, cd._h, batch) == reports
    # many waves' worth, every lane with its neighbour's public input differing
    many = [proofs[(7 * i) % (BOUND + 1)] for i in range(130)]
    many[77] = swapped
    reports = same_as_host(pkg, vd._h, many)
    assert [i for i, r in enumerate(reports) if r[0]] == [77]


def test_prove_batch_with_verify(pkg, bounded):
    """WitnessPlan.prove_batch(verify=True): a report per proof made, None beside the member the level walk refused."""
    cd, vd, L, proofs = bounded
    bb, tt = moi.less_or_equal_circuit(pkg, BOUND)
    plan = cd.witness_plan(bb.seed_cells(), generators=bb.generators())
    try:
        values = [4, BOUND + 1, 0]
        rows = []
        for v in values:
            b2, t2 = moi.less_or_equal_circuit(pkg, BOUND)
            rows.append(b2.seed_values({t2: v}))
        out, reports = plan.prove_batch(rows, public_inputs=[[v] for v in values], verify=True)
        assert isinstance(out[1], pkg.P2GpuError) and out[1].code == -5 and reports[1] is None
        assert reports[0].ok and reports[2].ok and reports[0].message == "accepted"
        assert [int.from_bytes(o.to_bytes()[L.pis_at:L.pis_at + 8], "little") for o in (out[0], out[2])] == [4, 0]
        assert [r.ok for r in vd.verify_batch([out[0], out[2]], device=False)] == [True, True]
        plain = plan.prove_batch(rows, public_inputs=[[v] for v in values])           # the default is unchanged: a list
        assert isinstance(plain, list) and isinstance(plain[1], pkg.P2GpuError) and plain[0].to_bytes() == out[0].to_bytes()
    finally:
        plan.close()


def test_device_group_is_refused(pkg, sha6):
    """A device group (two ranks sharing the GPU) holds no single device to verify on: P2GPU_E_ARG, no report written."""
    lib = pkg.load_library()
    try:
        pkg.init([0, 0])
        cd = pkg.CircuitData(pkg.make_circuit(6, "sha", 2)[0])
        try:
            for device in (True, False):
                rc, raw, err = vb.raw_batch(lib, cd._h, [sha6.proof], device=device)
                assert rc == -7 and "device group" in err, (device, rc, err)
            with pytest.raises(pkg.P2GpuError) as ei:
                cd.verify_batch([sha6.proof])
            assert ei.value.code == -7
        finally:
            cd.close()
    finally:
        pkg.init([0])
    assert [r.ok for r in sha6.cd.verify_batch([sha6.proof])] == [True]


def test_deep_tree(pkg, gpu):
    c = Case(pkg, 13, "arith", 7)
    bad = vb.flip(c.proof, c.L.queries_at + 27 * c.L.query_bytes + c.L.step_at[1] + 16 * 16 + 1 + 3 * c.L.hb)   # the top sibling of the last query's second fold
    batch = [c.proof] * 3 + [bad] + [c.proof] * 4
    reports = same_as_host(pkg, c.vd._h, batch)
    assert [r[0] for r in reports] == [0, 0, 0, -9, 0, 0, 0, 0] and reports[3] == (-9, 13, 27, 1)


def test_handle_kinds(pkg, ecdsa8):
    c = ecdsa8
    batch = [c.proof, vb.flip(c.proof, c.L.pow_at), c.proof, vb.flip(c.proof, c.L.tail_at - 3)]
    on_prover = same_as_host(pkg, c.cd._h, batch)
    on_verifier = same_as_host(pkg, c.vd._h, batch)
    assert on_prover == on_verifier and [r[0] for r in on_prover] == [0, -9, 0, -9]
    assert [r.ok for r in c.cd.verify_batch(batch)] == [True, False, True, False]
    for h in (c.cd._h, c.vd._h):     # nothing of the circuit's length: every verdict from the shape step, no launch
        assert [r[1] for r in same_as_host(pkg, h, [c.proof[:-1], b"", c.proof + b"\0"])] == [3, 1, 3]
    assert c.cd.prove(c.wires, c.pis).to_bytes() == c.proof       # the prover handle proves the same bytes afterwards


def test_verify_while_another_handle_proves(pkg, ecdsa8, sha6):
    """A verify batch on one handle while another thread proves on a second one: verdicts and proof bytes as they are alone."""
    c, p = ecdsa8, sha6
    batch = [c.proof, vb.flip(c.proof, c.L.open_at + 3), c.proof] * 8
    alone = c.cd.verify_batch(batch)
    proofs, errors = [], []

    def prover():
        try:
            for _ in range(6):
                proofs.append(p.cd.prove(p.wires, p.pis).to_bytes())
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    t = threading.Thread(target=prover)
    t.start()
    together = [c.cd.verify_batch(batch) for _ in range(3)] + [c.vd.verify_batch(batch)]
    t.join(120)
    assert not t.is_alive() and not errors, errors
    assert all(r == alone for r in together) and [r.ok for r in alone] == [True, False, True] * 8
    assert proofs == [p.proof] * 6
