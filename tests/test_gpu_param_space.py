"""GPU proofs of circuits off the reference's shape (K = 2, rate_bits 3, 80 routed wires, arity 16 at every step): the same
parameter space as tests/test_param_space.py, proved by the HIP path and compared byte for byte with the oracle.

Proved on the GPU here (GRID, POSEIDON, the K = 1 / half_gates case and the device groups):
  K 1 and 2; rate_bits 1, 2 and 3 (C = 2, 4, 8 cosets); arity bits 1, 2, 3, 4 in mixed orders, 8 steps of arity 2;
  9, 10, 12 and 16 partial-product chunks; PoW bits 0, 12, 16; 1, 28 and 64 query rounds; KeccakHash<25> and PoseidonHash
  (whose step leaves of 4 elements are hashed lane by lane and those of 8 and 16 elements cooperatively);
  coset sharding over device groups of 2 and 4 ranks at rate 2, 2 ranks at rate 1, 8 ranks at rate 3 with K = 1.
Refused: a device group whose size does not divide the 2^rate_bits cosets.  The loader's refusals are host code
(test_param_space.py).
"""
import sys

import numpy as np
import pytest

from conftest import GOLDEN

sys.path.insert(0, GOLDEN)
import fri_check  # noqa: E402
import param_circuits as pc  # noqa: E402
import proof_stages  # noqa: E402

pytestmark = pytest.mark.gpu

# (name, circuit, patch) as in test_param_space.GRID
GRID = [
    ("arity_1", ("synth", "ecdsa", 9), dict(arity=[1])),
    ("arity_2_3", ("synth", "sha", 10), dict(arity=[2, 3])),
    ("arity_3_1_2", ("synth", "sha", 10), dict(arity=[3, 1, 2])),
    ("arity_1_1_1_1", ("synth", "sha", 10), dict(arity=[1, 1, 1, 1])),
    ("arity_4_1", ("synth", "ecdsa", 9), dict(arity=[4, 1])),
    ("arity_8_steps", ("synth", "sha", 10), dict(arity=[1] * 8)),
    ("K1_arity_1_2", ("synth", "sha", 10), dict(K=1, arity=[1, 2])),
    ("pow0", ("synth", "sha", 10), dict(pow_bits=0)),
    ("queries1", ("synth", "ecdsa", 9), dict(queries=1)),
    ("queries64", ("synth", "sha", 10), dict(queries=64)),
    ("rate2_R64_16chunks", ("arith", 10, 64, 64, 2, 2, 2), {}),
    ("rate2_K1_W135_d14", ("arith", 14, 64, 135, 1, 2, 2), {}),
    ("rate2_R40_cap6", ("arith", 9, 40, 80, 2, 2, 6), {}),
    ("rate2_K1_arity_3_1", ("arith", 12, 48, 96, 1, 2, 3), dict(arity=[3, 1])),
    ("rate3_K1_generated", ("arith", 9, 80, 234, 1, 3, 4), dict(arity=[2, 2], pow_bits=12)),
    ("rate1_R32_16chunks", ("degree1", 10, 32, 32, 2, 1, 1), {}),
    ("rate1_K1_R20_cap5_d13", ("degree1", 13, 20, 40, 1, 1, 5), dict(arity=[3])),
]


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]


def builders(pkg, orc):
    return [pc.build_fn(pkg.load_library().p2gpu_build_blob), pc.build_fn(orc.lib().orc_build_blob)]


def make(pkg, orc, circuit, patch, seed=5, hasher=0):
    if circuit[0] == "synth":
        blob, wires = pkg.make_circuit(circuit[2], circuit[1], seed, hasher=hasher)
    else:
        gen = pc.arith_circuit if circuit[0] == "arith" else pc.degree1_circuit
        blob, wires = gen(*circuit[1:], seed=seed, builders=builders(pkg, orc))
    return (pc.with_params(blob, **patch) if patch else blob), wires


def sparse_split(wires):
    """(ncols, row) for prove_sparse: the columns from ncols on are zero in every row but `row`."""
    nz = wires != 0
    multi = np.nonzero(nz.sum(axis=1) > 1)[0]
    ncols = int(multi[-1]) + 1 if len(multi) else 0
    rows = np.nonzero(nz[ncols:].any(axis=0))[0]
    assert len(rows) <= 1
    return ncols, int(rows[0]) if len(rows) else 0


def prove_every_way(pkg, cd, wires, want):
    """Host matrix (twice on the handle), resident torch tensor, prove_sparse: every proof equals `want`."""
    import torch

    for _ in range(2):
        assert cd.prove(wires).to_bytes() == want
    wd = torch.from_numpy(wires.view(np.int64)).cuda()
    assert cd.prove(wd).to_bytes() == want
    ncols, row = sparse_split(wires)
    assert cd.prove_sparse(wires, ncols, row).to_bytes() == want
    assert cd.prove(wd).to_bytes() == want


def fri_checked(blob, proof, cd):
    c = proof_stages.header(blob)
    capb = cd.constants_sigmas_cap()
    fri_check.check(c, proof, cd.circuit_digest(), [capb[i:i + 25] for i in range(0, len(capb), 25)],
                    pow_bits=int(blob[:256].view(np.uint32)[11]))


@pytest.mark.parametrize("name,circuit,patch", GRID, ids=[g[0] for g in GRID])
def test_gpu_proofs_across_the_parameter_space(pkg, orc, gpu, name, circuit, patch):
    blob, wires = make(pkg, orc, circuit, patch)
    oc = orc.OracleCircuit(blob)
    want, _ = oc.prove(wires)
    cd = pkg.CircuitData(blob)
    assert cd.constants_sigmas_cap() == oc.cap()
    prove_every_way(pkg, cd, wires, want)
    cd.verify(want)
    c = proof_stages.header(blob)
    if any(a != 4 for a in c["arity"]) or c["rate_bits"] != 3 or c["K"] != 2:
        fri_checked(blob, want, cd)
    cd.close()
    oc.close()


@pytest.mark.parametrize("d", [10, 15])
def test_k1_challenge_with_half_domain_gates(pkg, orc, gpu, d):
    """K = 1 on the heavy mix: the opening order, the zs / partial-product column counts and the half-domain gate sums'
    slot count (half_slots * K) all shrink; knob half_gates 0 / 1 / 2 keeps every byte."""
    blob, wires = make(pkg, orc, ("synth", "ecdsa", d), dict(K=1))
    want = orc.OracleCircuit(blob).prove(wires)[0]
    cd = pkg.CircuitData(blob)
    for hg in (0, 1, 2):
        cd.set("half_gates", hg)
        prove_every_way(pkg, cd, wires, want)
    cd.close()


POSEIDON = [("sha", 9, dict(arity=[1, 2])), ("ecdsa", 10, dict(arity=[3])), ("sha", 10, dict(K=1, arity=[2, 1, 1]))]


@pytest.mark.parametrize("mix,d,patch", POSEIDON)
def test_poseidon_step_leaves_of_every_size(pkg, orc, gpu, mix, d, patch):
    """PoseidonHash step trees: arity 2 leaves (4 elements) take hash_or_noop's no-hash branch and the lane-per-leaf kernel;
    arity 4 and 8 leaves (8, 16 elements) the cooperative twelve-lane kernel."""
    blob, wires = make(pkg, orc, ("synth", mix, d), patch, hasher=1)
    oc = orc.OracleCircuit(blob)
    want, _ = oc.prove(wires)
    assert oc.verify(want)
    cd = pkg.CircuitData(blob)
    assert cd.hash_bytes() == 32
    prove_every_way(pkg, cd, wires, want)
    cd.close()
    oc.close()


# ---- coset sharding at C = 2, 4, 8 ---------------------------------------------------------------------------------------
def _group_case(pkg, orc, world, blob, wires, knobs=((0, 0, 0),)):
    want = orc.OracleCircuit(blob).prove(wires)[0]
    try:
        pkg.init([0] * world)
        cd = pkg.CircuitData(blob)
        for intt, zs, red in knobs:
            cd.set("shard_intt", intt)
            cd.set("shard_zs", zs)
            cd.set("shard_reduce", red)
            prove_every_way(pkg, cd, wires, want)
        cd.close()
    finally:
        pkg.init([0])


@pytest.mark.parametrize("world,circuit", [(2, ("arith", 10, 64, 64, 2, 2, 2)), (4, ("arith", 11, 64, 135, 1, 2, 2)),
                                           (2, ("degree1", 10, 32, 32, 2, 1, 1))])
def test_device_group_at_rate_1_and_2(pkg, orc, gpu, world, circuit):
    """A single-process device group (ranks sharing the one GPU) over C = 4 and C = 2 cosets, every exchange on."""
    blob, wires = make(pkg, orc, circuit, {})
    _group_case(pkg, orc, world, blob, wires, knobs=((0, 0, 0), (1, 1, 1)))


def test_k1_eight_ranks_overflowed_the_old_exchange_buffer(pkg, orc, gpu):
    """K = 1, rate 3, 8 ranks, d = 14: the shard_reduce all-gather writes 2 G n words into the exchange buffer, more than
    max(G * gather_cap, K * C * n) + 64 -- what the buffer held before it was sized for this exchange too."""
    blob, wires = make(pkg, orc, ("synth", "ecdsa", 14), dict(K=1))
    old, need = pc.xchg_words(blob, 8, new=False)
    new, _ = pc.xchg_words(blob, 8, new=True)
    assert old < need <= new, (old, need, new)
    _group_case(pkg, orc, 8, blob, wires, knobs=((0, 0, 0), (1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)))


def test_group_size_must_divide_the_cosets(pkg, orc, gpu):
    blob, _ = make(pkg, orc, ("arith", 8, 64, 64, 2, 2, 2), {})
    try:
        pkg.init([0] * 8)
        with pytest.raises(pkg.P2GpuError):
            pkg.CircuitData(blob)
    finally:
        pkg.init([0])
