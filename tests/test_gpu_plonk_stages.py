"""Z, the partial products and the quotient on the MI355X (`CircuitData.plonk_stages`: prover phases 1-3 on challenges the
test chooses) against tests/plonk_stage_model.py, word for word, no tolerance.

Whole-proof parity takes beta, gamma and alpha from the transcript: a congruent word >= p in the wrong operand position shows
about once in 2^32 operations, values such as beta = 0 or a zero numerator are unreachable, and a mismatch names a cap, not a
row.  Here the challenges, the wires and (through zp_in) the committed Z / partial products are chosen (plonk_stage_cases.py;
tests/test_plonk_stage_model.py shows without a GPU that every family places what it claims), and a mismatch names the output,
challenge, column or coset, and row.

Shapes (n rows): 8, 32 (64-lane blocks), 64 (first size of the four-wave split of the quotient and gate-sum kernels), 128, 256 (one
256-lane block), 512 (two blocks: the scan's block prefix).  Circuits: ArithmeticGate rows with R = 80 / K = 2 / rate 3, R = 64 /
rate 2 (16 chunks), R = 40 / rate 2, R = 44 / rate 3 (a ragged last chunk), K = 1; degree-1 gates at rate 1; the sha and ecdsa
mixes with public inputs (PoseidonGate) with the half-domain gate sums off and forced.
Families: 1 the real path (trace challenges, satisfying witness, the caps are the proof's); 2 challenge edges; 3 targeted
factors (zero numerators in the first / a middle / the last chunk, at row 0, row n - 1 and the block boundary of n = 512: Z
holds runs of zeros); 4 a pinned coset (edge words as the LDE words of Z, the partial products and the routed wires on an even and
an odd coset); 5 steered raw words (products whose congruent raw word is >= p by the model's account).
"""
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

import plonk_stage_cases as cases
import plonk_stage_model as psm

pytestmark = pytest.mark.gpu
_handles = {}


@pytest.fixture(scope="module")
def gpu(pkg):
    import torch

    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert "gfx950" in pkg.device_info()["name"]
    yield True
    _handles.clear()


def handle(pkg, orc, name, **knobs):
    key = (name,) + tuple(sorted(knobs.items()))
    if key not in _handles:
        cd = pkg.CircuitData(cases.circuit(pkg, orc, name).blob)
        for k, v in knobs.items():
            cd.set(k, v)
        _handles[key] = cd
    return _handles[key]


def first_difference(what, got, want):
    got, want = np.asarray(got), np.asarray(want, dtype=np.uint64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    if len(bad):
        at = tuple(int(x) for x in bad[0])
        pytest.fail("%s: %d of %d words differ; first at %s: device %#x, model %#x" % (what, len(bad), got.size, at, int(got[at]), int(want[at])))


def keccak_cap(orc, cir, vals):
    orc.lib().orc_set_hasher(0)
    return orc.commit_values(np.ascontiguousarray(vals, dtype=np.uint64), cir.rate_bits, cir.cap_h)


def check_case(pkg, orc, case, got=None, **knobs):
    """Every word of zp [column][row], qvals [challenge][coset][index], quot [chunk][coefficient] and the three caps."""
    b = cases.circuit(pkg, orc, case.circuit)
    if got is None:
        got = handle(pkg, orc, case.circuit, **knobs).plonk_stages(*case.args())
    want = psm.stages(orc, b.cir, case.wires, case.pih, case.betas, case.gammas, case.alphas, case.zp_in)
    first_difference(case.name + " zp_out [column][row]", got["zp"], want["zp"])
    first_difference(case.name + " qvals_out [challenge][coset][index]", got["qvals"], want["qvals"])
    first_difference(case.name + " quot_out [chunk][coefficient]", got["quot"], want["quot"])
    caps = case.caps or (keccak_cap(orc, b.cir, case.wires), keccak_cap(orc, b.cir, want["zp"] if case.zp_in is None else case.zp_in),
                         keccak_cap(orc, b.cir, np.stack([orc.ntt(col) for col in want["quot"]])))
    for name, g, w in zip(("wires", "zs", "quotient"), got["caps"], caps):
        assert g == w, "%s: the %s cap differs" % (case.name, name)
    return got


def digest(out):
    h = hashlib.sha256()
    for k in ("zp", "qvals", "quot"):
        h.update(np.ascontiguousarray(out[k]).tobytes())
    for c in out["caps"]:
        h.update(c)
    return h.hexdigest()


# ---- 1. the real path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", cases.REAL)
def test_real_path_gives_the_proofs_caps(pkg, orc, gpu, name):
    case = cases.real_case(pkg, orc, name)
    check_case(pkg, orc, case)
    # a proof on the handle afterwards is the oracle's
    assert handle(pkg, orc, name).prove(case.wires, cases.circuit(pkg, orc, name).pis).to_bytes() == case.proof


@pytest.mark.parametrize("name", ["sha64", "ecdsa64"])
def test_knobs_give_the_same_words(pkg, orc, gpu, name):
    """half_gates 0 and 2 against the model; zero_columns / virtual_columns off: the same words as with them on."""
    case = cases.real_case(pkg, orc, name)
    a = check_case(pkg, orc, case, half_gates=0)
    b = check_case(pkg, orc, case, half_gates=2)
    c = handle(pkg, orc, name, zero_columns=0, virtual_columns=0).plonk_stages(*case.args())
    assert digest(a) == digest(b) == digest(c)
    # the half-domain sums on wires that do NOT satisfy the circuit and an edge alpha
    rng = np.random.default_rng(40)
    cir = cases.circuit(pkg, orc, name).cir
    rnd = cases.Case("random-" + name, name, cases.rand_words(rng, (cir.W, cir.n)), cases.rand_list(rng, 4), cases.rand_list(rng, 2),
                     cases.rand_list(rng, 2), [psm.P - 1, 1 << 32])
    assert psm.denominators_nonzero(cir, rnd.wires, rnd.betas, rnd.gammas)
    assert digest(check_case(pkg, orc, rnd, half_gates=2)) == digest(handle(pkg, orc, name, half_gates=0).plonk_stages(*rnd.args()))


# ---- 2 - 5. the chosen inputs ---------------------------------------------------------------------------------------------------
def family_ids(fam, count):
    return ["%s-%d" % (fam, i) for i in range(count)]


@pytest.mark.parametrize("i", range(13), ids=family_ids("edges", 13))
def test_challenge_edges(pkg, orc, gpu, i):
    fam = cases.family(pkg, orc, "edges")
    assert len(fam) == 13
    check_case(pkg, orc, fam[i])


@pytest.mark.parametrize("i", range(5), ids=family_ids("targets", 5))
def test_targeted_factors(pkg, orc, gpu, i):
    fam = cases.family(pkg, orc, "targets")
    assert len(fam) == 5
    check_case(pkg, orc, fam[i])


@pytest.mark.parametrize("i", range(4), ids=family_ids("pinned", 4))
def test_pinned_coset(pkg, orc, gpu, i):
    fam = cases.family(pkg, orc, "pinned")
    assert len(fam) == 4
    check_case(pkg, orc, fam[i])


@pytest.mark.parametrize("i", range(4), ids=family_ids("steered", 4))
def test_steered_raw_words(pkg, orc, gpu, i):
    fam = cases.family(pkg, orc, "steered")
    assert len(fam) == 4
    check_case(pkg, orc, fam[i])


# ---- further checks ------------------------------------------------------------------------------------------------------------
GROUP_CHILD = r"""
import sys, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as ge
pkg, orc = ge.load_package(), ge.load_oracle()
import plonk_stage_cases as cases
pkg.init(devices=(0, 0))
b = cases.circuit(pkg, orc, "arith64_R64")
cd = pkg.CircuitData(b.blob)
try:
    cd.plonk_stages(b.wires, [0] * 4, [1, 2], [3, 4], [5, 6])
    print("ACCEPTED")
except pkg.P2GpuError as e:
    print("REFUSED", e.code)
"""


def test_refusals(pkg, orc, gpu):
    """P2GPU_E_ARG before any device call: a null pointer, a verifier-only handle, a sharded handle, a word >= p."""
    import ctypes

    case = cases.real_case(pkg, orc, "arith32")
    cd = handle(pkg, orc, "arith32")
    P = psm.P
    for field, bad in (("wires", None), ("pih", [P, 0, 0, 0]), ("betas", [P, 1]), ("gammas", [1, (1 << 64) - 1]), ("alphas", [P + 1, 0])):
        args = dict(wires=case.wires, pih=case.pih, betas=case.betas, gammas=case.gammas, alphas=case.alphas)
        if bad is None:
            bad = np.array(case.wires, copy=True)
            bad[79, 31] = P
        args[field] = bad
        with pytest.raises(pkg.P2GpuError) as e:
            cd.plonk_stages(args["wires"], args["pih"], args["betas"], args["gammas"], args["alphas"])
        assert e.value.code == -7, (field, e.value)
    zp = psm.zs(cases.circuit(pkg, orc, "arith32").cir, case.wires, case.betas, case.gammas)
    zp[3, 5] = P
    with pytest.raises(pkg.P2GpuError) as e:
        cd.plonk_stages(*case.args()[:5], zp_in=zp)
    assert e.value.code == -7
    lib = pkg.load_library()
    w = np.ascontiguousarray(case.wires)
    ch = np.zeros(4, dtype=np.uint64)
    out = np.zeros(1 << 20, dtype=np.uint64)
    ok = [cd._h, w.ctypes.data, ch.ctypes.data, ch.ctypes.data, ch.ctypes.data, ch.ctypes.data, None] + [out.ctypes.data] * 4
    for null in (0, 1, 2, 3, 4, 5, 7, 8, 9, 10):
        a = list(ok)
        a[null] = None
        assert lib.p2gpu_plonk_stages(*a) == -7, null
    vk = pkg.VerifierCircuitData(cd.verifier_blob())
    a = list(ok)
    a[0] = vk._h
    assert lib.p2gpu_plonk_stages(*a) == -7
    # a device group (two ranks sharing the one GPU), in a process of its own: the device list is per process
    tests = os.path.dirname(os.path.abspath(__file__))
    r = subprocess.run([sys.executable, "-c", GROUP_CHILD.format(root=os.path.dirname(tests), tests=tests)], capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0 and "REFUSED -7" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    # the handle is none the worse for the refusals
    check_case(pkg, orc, case)


CHILD = r"""
import sys, hashlib, numpy as np, torch
sys.path.insert(0, {root!r}); sys.path.insert(0, {tests!r})
import __graft_entry__ as ge
pkg, orc = ge.load_package(), ge.load_oracle()
import plonk_stage_cases as cases
from test_gpu_plonk_stages import digest
case = cases.real_case(pkg, orc, "ecdsa64")
for hg in (0, 2):
    cd = pkg.CircuitData(cases.circuit(pkg, orc, "ecdsa64").blob)
    cd.set("half_gates", hg)
    cd.set("profile", 2)
    print("WORDS", digest(cd.plonk_stages(*case.args())))
    print("KERNELS", "|".join(sorted(cd.kernel_stats())))
"""


def test_gate_groups_and_launch_forms(pkg, orc, gpu):
    """P2GPU_GATE_GROUPS (and its two companions) 1 and 4, each in a process of its own, half_gates 0 and 2: the words the model
    confirms in this process; and across them every launch form of the quotient ran (profile = 2 kernel statistics)."""
    case = cases.real_case(pkg, orc, "ecdsa64")
    want = digest(check_case(pkg, orc, case, half_gates=0))
    tests = os.path.dirname(os.path.abspath(__file__))
    code = CHILD.format(root=os.path.dirname(tests), tests=tests)
    kernels = set()
    for g in ("1", "4"):
        env = dict(os.environ, P2GPU_GATE_GROUPS=g, P2GPU_GATE_GROUPS_HALF=g, P2GPU_SUMS_GROUPS=g)
        r = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, (g, r.stderr[-2000:])
        lines = r.stdout.splitlines()
        assert [ln.split()[1] for ln in lines if ln.startswith("WORDS")] == [want, want], g
        for ln in lines:
            if ln.startswith("KERNELS"):
                kernels |= set(ln.split(" ", 1)[1].split("|"))
    for k in ("quotient_kernel<false, 1>", "quotient_kernel<false, 4>", "gate_sums_cross_kernel", "poseidon_gate_kernel"):
        assert k in kernels, (k, sorted(kernels))
    assert any(k.startswith("gate_sums_kernel<1") for k in kernels) and any(k.startswith("gate_sums_kernel<4") for k in kernels), sorted(kernels)
