"""p2gpu_prove_batch_dev / p2gpu_prove_seeds_batch on the MI355X (csrc/provebatch.hip): every proof byte against the lone
CircuitData.prove on the same handle -- every circuit shape the batched prover has a path for, distinct witnesses in one batch,
the block, wave and slab edges of the batch size, failing members among good ones, the walk-and-prove call, the refusals on a
prover handle, and a batch beside a lone proof on another handle."""
import random
import threading

import pytest

import memory_ops_inputs as moi
import prove_batch_cases as pbc
import witness_batch_inputs as wbi
import witness_gen_inputs as wgi

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
UNSAT = "witness does not satisfy the circuit"


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    return True


@pytest.fixture(scope="module")
def bounded(pkg, gpu):
    """The less-or-equal circuit: (handle, {value: matrix}, {value: lone proof bytes})."""
    blob, mats = pbc.less_or_equal(pkg)
    cd = pkg.CircuitData(blob)
    lone = {v: cd.prove(w, public_inputs=[v]).to_bytes() for v, w in mats.items()}
    assert len(set(lone.values())) == len(lone)
    yield cd, mats, lone
    cd.close()


def members(bounded, values):
    cd, mats, lone = bounded
    return pbc.stacked([mats[v] for v in values], DEV), [[v] for v in values], [lone[v] for v in values]


@pytest.mark.parametrize("name,d,mix,npi,nw,hasher", pbc.SHAPES, ids=[s[0] for s in pbc.SHAPES])
def test_shapes(pkg, gpu, name, d, mix, npi, nw, hasher):
    blob, wires, pis = pbc.shape(pkg, name, d, mix, npi, nw, hasher)
    cd = pkg.CircuitData(blob)
    try:
        assert cd.degree_bits == d
        lone = cd.prove(wires, pis).to_bytes()
        rc, status, proofs, err = pbc.raw(pkg, cd, pbc.stacked([wires] * 3, DEV), [pis] * 3)
        assert rc == 0 and status == [0, 0, 0], (rc, status, err)
        assert proofs == [lone] * 3
        assert cd.prove(wires, pis).to_bytes() == lone      # the lone path on the same handle is what it was
    finally:
        cd.close()


def test_distinct_public_inputs_in_one_batch(pkg, bounded):
    cd = bounded[0]
    values = list(range(pbc.BOUND + 1))
    random.Random(3).shuffle(values)
    wires, pis, lone = members(bounded, values)
    out = cd.prove_batch(wires, pis)
    got = [o.to_bytes() for o in out]
    assert got == lone and len(set(got)) == len(got)


def test_distinct_bitwise_members(pkg, gpu):
    ks = [0, 5, 1, 7, 3]
    ms = [wbi.bitwise_member(pkg, k) for k in ks]
    cd = pkg.CircuitData(ms[0][0])
    try:
        lone = [cd.prove(m[3]).to_bytes() for m in ms]
        got = [o.to_bytes() for o in cd.prove_batch(pbc.stacked([m[3] for m in ms], DEV))]
        assert got == lone and len(set(got)) == len(ks)
    finally:
        cd.close()


def test_distinct_custom_gate_chains(pkg, gpu):
    kw, cells, _, _ = wgi.custom_gate_chain()
    cd = pkg.CircuitData.build(**kw)
    try:
        mats = [wbi.custom_gate_chain(second)[1] for second in (0x80000000, 5, 0xFFFFFFFF, 0)]
        lone = [cd.prove(m).to_bytes() for m in mats]
        got = [o.to_bytes() for o in cd.prove_batch(pbc.stacked(mats, DEV))]
        assert got == lone and len(set(got)) == len(mats)
    finally:
        cd.close()


@pytest.mark.parametrize("batch", [1, 2, 63, 65, 257])
def test_sizes(pkg, bounded, batch):
    cd = bounded[0]
    values = [(5 * i + 2) % (pbc.BOUND + 1) for i in range(batch)]
    wires, pis, lone = members(bounded, values)
    rc, status, proofs, err = pbc.raw(pkg, cd, wires, pis)
    assert rc == 0 and not any(status), (rc, err)
    assert proofs == lone
    info = cd.prove_batch_info()
    assert info["slab"] == batch and info["launches"] > 0
    test_sizes.launches.add(info["launches"])
    assert len(test_sizes.launches) == 1        # the launches of a slab do not depend on the number of proofs in it


test_sizes.launches = set()


def test_slab_boundary(pkg, bounded):
    cd = bounded[0]
    wires, pis, lone = members(bounded, [3, 0, 8, 5, 1, 7, 2])
    auto = [o.to_bytes() for o in cd.prove_batch(wires, pis)]
    cd.set("prove_batch_slab", 3)
    try:
        slabs = [o.to_bytes() for o in cd.prove_batch(wires, pis)]
        assert cd.prove_batch_info()["slab"] == 1      # 3 + 3 + 1
    finally:
        cd.set("prove_batch_slab", 0)
    assert slabs == auto == lone


def test_failing_members_among_good_ones(pkg, bounded):
    cd, mats, lone = bounded
    vd = cd.verifier_data()
    try:
        values = [4, 1, 6, 2, 7]
        ms = [mats[v].copy() for v in values]
        cells = moi.less_or_equal_circuit(pkg, pbc.BOUND)[0].seed_cells()
        r, c = cells[0]                                          # a cell a gate reads: the public input's own
        ms[1][c, r] = (int(ms[1][c, r]) + 1) % moi.P
        pis = [[v] for v in values]
        pis[3] = [7]                                              # member 3 proves 2 and claims 7
        wires = pbc.stacked(ms, DEV)
        rc, status, proofs, err = pbc.raw(pkg, cd, wires, pis)
        assert status == [0, -5, 0, -5, 0] and rc == -5, (rc, status, err)
        assert err.startswith("witness 1 of the batch: ") and UNSAT in err
        for b in (1, 3):
            with pytest.raises(pkg.P2GpuError) as ei:
                cd.prove(wires[b], pis[b])
            assert ei.value.code == -5 and str(ei.value) == "p2gpu error -5: " + err[len("witness 1 of the batch: "):]
            assert proofs[b] == bytes(len(proofs[b]))
        assert [proofs[b] for b in (0, 2, 4)] == [lone[v] for v in (4, 6, 7)]
        assert [rep.ok for rep in cd.verify_batch([proofs[b] for b in (0, 2, 4)])] == [True, True, True]
        out = cd.prove_batch(wires, pis)
        assert [isinstance(o, pkg.P2GpuError) and o.code for o in out] == [False, -5, False, -5, False] and UNSAT in str(out[1])
        cd.set("self_check", 0)
        try:
            rc0, status0, proofs0, _ = pbc.raw(pkg, cd, wires, pis)
            lone0 = [cd.prove(wires[b], pis[b]).to_bytes() for b in (1, 3)]
        finally:
            cd.set("self_check", 1)
        assert rc0 == 0 and not any(status0)
        assert [proofs0[1], proofs0[3]] == lone0 and [proofs0[b] for b in (0, 2, 4)] == [lone[v] for v in (4, 6, 7)]
        assert [rep.ok for rep in vd.verify_batch(proofs0)] == [True, False, True, False, True]
    finally:
        vd.close()


def test_one_call_walk_and_prove(pkg, bounded):
    cd = bounded[0]
    bb, _ = moi.less_or_equal_circuit(pkg, pbc.BOUND)
    plan = cd.witness_plan(bb.seed_cells(), generators=bb.generators())
    try:
        values = [4, pbc.BOUND + 1, 0]
        rows = []
        for v in values:
            b2, t2 = moi.less_or_equal_circuit(pkg, pbc.BOUND)
            rows.append(b2.seed_values({t2: v}))
        pis = [[v] for v in values]
        loop, loop_reports = plan.prove_batch(rows, public_inputs=pis, verify=True)
        one, one_reports = plan.prove_batch(rows, public_inputs=pis, verify=True, one_call=True)
        assert [o.to_bytes() for o in (one[0], one[2])] == [o.to_bytes() for o in (loop[0], loop[2])] == [bounded[2][4], bounded[2][0]]
        assert isinstance(one[1], pkg.P2GpuError) and one[1].code == loop[1].code == -5 and str(one[1]) == str(loop[1])
        assert one_reports == loop_reports and one_reports[1] is None and one_reports[0].ok and one_reports[2].ok
        _, walk_status, walk_cells = plan.generate_batch(rows)
        res, cells = plan._prove_batch_one_call(rows, pis)
        assert cells == walk_cells and [isinstance(r, pkg.P2GpuError) for r in res] == [bool(s) for s in walk_status]
    finally:
        plan.close()


def test_refusals_on_a_prover_handle(pkg, gpu):
    lib = pkg.load_library()
    blob13, wires13 = pkg.make_circuit(13, "arith", seed=2)
    cd = pkg.CircuitData(blob13)
    try:
        rc, status, proofs, err = pbc.raw(pkg, cd, pbc.stacked([wires13], DEV), [()])
        assert rc == -7 and "P2GPU_PROVE_BATCH_MAX_DEGREE_BITS = 12" in err and "p2gpu_prove_dev" in err and status == [99]
        assert len(cd.prove(wires13)) == cd._bound
    finally:
        cd.close()
    blob, wires = pkg.make_circuit(6, "sha", seed=2)
    stack = pbc.stacked([wires] * 2, DEV)
    try:
        pkg.init([0, 0])
        grp = pkg.CircuitData(blob)
        try:
            rc, status, _, err = pbc.raw(pkg, grp, stack, [(), ()])
            assert rc == -7 and "device group" in err and status == [99, 99]
            lone = grp.prove(wires).to_bytes()
        finally:
            grp.close()
    finally:
        pkg.init([0])
    cd = pkg.CircuitData(blob)
    try:
        cb = pkg.prover._ALLGATHER_FN(lambda ctx, send, recv, nbytes: -1)      # (never called: world = 1)
        assert lib.p2gpu_circuit_set_shard(cd._h, 0, 1, cb, None) == 0
        rc, status, _, err = pbc.raw(pkg, cd, stack, [(), ()])
        assert rc == -7 and "sharding configured" in err and status == [99, 99]
        assert cd.prove(wires).to_bytes() == lone
    finally:
        cd.close()


def test_beside_another_handle(pkg, bounded):
    """The batch call on one handle while another thread proves alone on a handle of another circuit: both as they are alone."""
    cd = bounded[0]
    blob, wires = pkg.make_circuit(6, "sha", seed=2)
    other = pkg.CircuitData(blob)
    try:
        want_other = other.prove(wires).to_bytes()
        stack, pis, lone = members(bounded, [(3 * i) % (pbc.BOUND + 1) for i in range(40)])
        proofs, errors = [], []

        def prover():
            try:
                for _ in range(6):
                    proofs.append(other.prove(wires).to_bytes())
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        t = threading.Thread(target=prover)
        t.start()
        together = [[o.to_bytes() for o in cd.prove_batch(stack, pis)] for _ in range(3)]
        t.join(120)
        assert not t.is_alive() and not errors, errors
        assert all(g == lone for g in together) and proofs == [want_other] * 6
    finally:
        other.close()
