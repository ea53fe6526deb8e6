"""The circuits and the chosen inputs of tests/test_gpu_plonk_stages.py (test infrastructure), built without a GPU so that
tests/test_plonk_stage_model.py can check -- by the model's own account -- that every family puts a case where it says it does.

A case is the argument list of `CircuitData.plonk_stages` plus `account`: what the model says about the words the case was built
to produce (targets hit, zeros in Z, raw words >= p by plonk_stage_model.raw_nc).  The account never decides a comparison.
"""
import sys

import numpy as np

import plonk_stage_model as psm
from conftest import GOLDEN
from plonk_stage_model import EDGE, P

sys.path.insert(0, GOLDEN)
import param_circuits as pc  # noqa: E402

# (the loader wants cap_height >= rate_bits)
# name -> ("arith" | "degree1", d, R, W, K, rate_bits, cap_height) or ("synth", mix): n = 8 ... 512, see the GPU test's docstring
CIRCUITS = {
    "arith32": ("arith", 5, 80, 80, 2, 3, 3),
    "arith64_R64": ("arith", 6, 64, 64, 2, 2, 2),         # 16 chunks
    "arith128_R40": ("arith", 7, 40, 80, 2, 2, 2),        # 10 chunks of 4
    "arith256_K1": ("arith", 8, 80, 100, 1, 3, 3),
    "arith512": ("arith", 9, 80, 80, 2, 3, 3),            # two 256-row blocks: the scan's block prefix
    "arith8_R44": ("arith", 3, 44, 44, 2, 3, 3),          # 6 chunks, the last of 4 columns: a ragged last chunk
    "degree1_32": ("degree1", 5, 16, 16, 2, 1, 1),
    # the same circuits with sigma replaced by a random permutation of all routed cells: no cell is its own image, so a numerator
    # can be zero (or any word) in ANY row without the denominator following it -- only for inputs that need not satisfy the circuit
    "arith32_perm": ("perm", "arith32"),
    "arith512_perm": ("perm", "arith512"),
    "sha64": ("synth", "sha"),
    "ecdsa64": ("synth", "ecdsa"),
}
_cache = {}


class Bundle:
    pass


def circuit(pkg, orc, name):
    """blob, satisfying wires, public inputs, model tables, the LDE of the constants / sigmas"""
    if name in _cache:
        return _cache[name]
    spec = CIRCUITS[name]
    b = Bundle()
    b.name, b.pis = name, ()
    if spec[0] == "perm":
        base = circuit(pkg, orc, spec[1])
        ids = np.array([[k * x % P for x in base.cir.sub] for k in base.cir.k_is], dtype=np.uint64)
        perm = np.random.default_rng(21).permutation(ids.size)
        b.blob, b.wires = np.array(base.blob, copy=True), None
        b.blob[base.cir.sigma_off:base.cir.sigma_off + 8 * ids.size] = ids.reshape(-1)[perm].view(np.uint8)
    elif spec[0] == "synth":
        b.blob, b.wires, b.pis = pkg.make_circuit(6, spec[1], 3, num_public_inputs=4)
    else:
        gen = pc.arith_circuit if spec[0] == "arith" else pc.degree1_circuit
        builders = [pc.build_fn(pkg.load_library().p2gpu_build_blob), pc.build_fn(orc.lib().orc_build_blob)]
        b.blob, b.wires = gen(*spec[1:], seed=11, builders=builders)
    b.cir = psm.Circuit(b.blob)
    b.cs_lde = psm.lde(orc, b.cir, np.concatenate([b.cir.constants, b.cir.sigmas]))
    _cache[name] = b
    return b


class Case:
    def __init__(self, name, circuit, wires, pih, betas, gammas, alphas, zp_in=None, account=None, caps=None):
        self.name, self.circuit, self.wires, self.pih = name, circuit, wires, [int(x) for x in pih]
        self.betas, self.gammas, self.alphas = ([int(x) for x in v] for v in (betas, gammas, alphas))
        self.zp_in, self.account, self.caps = zp_in, account or {}, caps

    def args(self):
        return (self.wires, self.pih, self.betas, self.gammas, self.alphas, self.zp_in)


def rand_words(rng, shape):
    return rng.integers(0, P, size=shape, dtype=np.uint64)


def rand_list(rng, k):
    return [int(x) for x in rand_words(rng, k)]


# ---- 1. the real path ----------------------------------------------------------------------------------------------------------
REAL = ["arith8_R44", "arith32", "arith128_R40", "arith256_K1", "degree1_32", "sha64", "ecdsa64"]


def real_case(pkg, orc, name):
    b = circuit(pkg, orc, name)
    proof, tr = orc.OracleCircuit(b.blob).prove(b.wires, b.pis)
    K, cap = b.cir.K, 25 << b.cir.cap_h
    c = Case("real-" + name, name, b.wires, tr.pi_hash, tr.betas[:K], tr.gammas[:K], tr.alphas[:K],
             caps=tuple(proof[i * cap:(i + 1) * cap] for i in range(3)))
    c.proof = proof
    return c


# ---- 2. challenge edges --------------------------------------------------------------------------------------------------------
M32 = psm.M32
EDGE_CHALLENGES = {   # K -> (betas, gammas, alphas): every word of EDGE appears; beta = 0, gamma = 0, alpha = 0, alpha = 1, a repeated pair
    2: [((0, P - 1), (1, 1 << 32), (0, 1)),
        ((2, M32), (0, P - (1 << 32)), (P - 1, 2)),
        ((P - 2, P - 2), (M32, M32), (1 << 32, P - (1 << 32))),
        ((1, 1 << 32), (P - 1, P - 2), (1, 0)),
        ((P - (1 << 32), 0), (2, 0), (M32, P - 2))],
    1: [((0,), (2,), (1,)), ((P - (1 << 32),), (0,), (0,)), ((M32,), (P - 1,), (P - 2,))],
}
EDGE_CIRCUITS = ["arith32", "arith64_R64", "arith256_K1"]


def edge_cases(pkg, orc, name):
    b = circuit(pkg, orc, name)
    out = []
    for q, (be, ga, al) in enumerate(EDGE_CHALLENGES[b.cir.K]):
        seed = 100 + q
        while True:
            rng = np.random.default_rng(seed)
            wires = rand_words(rng, (b.cir.W, b.cir.n))
            if psm.denominators_nonzero(b.cir, wires, be, ga):
                break
            seed += 1000
        words = set(be) | set(ga) | set(al)
        out.append(Case("edges-%s-%d" % (name, q), name, wires, rand_list(rng, 4), be, ga, al,
                        account={"words": words, "beta0": 0 in be, "gamma0": 0 in ga, "alpha0": 0 in al, "alpha1": 1 in al,
                                 "repeat": len(be) == 2 and be[0] == be[1] and ga[0] == ga[1], "K1": b.cir.K == 1}))
    return out


# ---- 3. targeted factors -------------------------------------------------------------------------------------------------------
# circuit -> cases; a case: zero numerators [(challenge, row, chunk position)], rows whose factors take the edge words
TARGETS = {
    "arith32_perm": [dict(zeros=[(0, 0, "first"), (1, 0, "middle")], edge_rows=[0, 1]),
                dict(zeros=[(0, 31, "last"), (1, 31, "first")], edge_rows=[30, 31]),
                dict(zeros=[(0, 0, "last"), (1, 31, "middle")], edge_rows=[0, 31])],
    "arith512_perm": [dict(zeros=[(0, 255, "last"), (1, 256, "first")], edge_rows=[255, 256]),
                 dict(zeros=[(0, 256, "middle"), (1, 511, "last")], edge_rows=[254, 257, 511])],
}


def placement(n, row):
    return "row0" if row == 0 else "last_row" if row == n - 1 else "block_boundary" if n > 256 and row in (255, 256) else "other"


def target_cases(pkg, orc, name):
    b = circuit(pkg, orc, name)
    cir, out = b.cir, []
    chunk_of = {"first": 0, "middle": cir.nchunks // 2, "last": cir.nchunks - 1}
    for q, spec in enumerate(TARGETS[name]):
        seed = 300 + q
        while True:
            rng = np.random.default_rng(seed)
            wires = rand_words(rng, (cir.W, cir.n))
            be, ga, al = (rand_list(rng, cir.K) for _ in range(3))
            used, want = set(), []
            for c, row, pos in spec["zeros"]:
                m = chunk_of[pos]
                j = min((m + 1) * cir.QF, cir.R) - 1 - c                      # a column of that chunk, one per challenge
                psm.target_factor(cir, wires, j, row, 0, be[c], ga[c], "num")
                used.add((j, row))
                want.append((c, j, row, "num", 0))
            for row in spec["edge_rows"]:
                for idx, t in enumerate(EDGE):
                    for which in ("num", "den"):
                        if t == 0:                                            # (zero numerators: `zeros`; a zero denominator is undefined)
                            continue
                        j = int(rng.integers(0, cir.R))
                        while (j, row) in used:
                            j = (j + 1) % cir.R
                        c = idx % cir.K
                        psm.target_factor(cir, wires, j, row, t, be[c], ga[c], which)
                        used.add((j, row))
                        want.append((c, j, row, which, t))
            if psm.denominators_nonzero(cir, wires, be, ga):
                break
            seed += 1000
        fac = [psm.factors(cir, wires, be[c], ga[c]) for c in range(cir.K)]
        for c, j, row, which, t in want:
            assert int(fac[c][0 if which == "num" else 1][j, row]) == t
        zp = psm.zs(cir, wires, be, ga)
        acct = {"zeros": [(placement(cir.n, row), pos) for _, row, pos in spec["zeros"]], "edge_factors": len(want),
                "zero_words_in_zp": int((zp == 0).sum()), "z0": [int(zp[c, 0]) for c in range(cir.K)]}
        for c, row, pos in spec["zeros"]:                                   # Z_c is zero from the next row on, never in row 0
            assert (zp[c, row + 1:] == 0).all() and (zp[c, :row + 1] != 0).all() and int(zp[c, 0]) == 1
        out.append(Case("targets-%s-%d" % (name, q), name, wires, rand_list(rng, 4), be, ga, al, account=acct))
    return out


# ---- 4. a pinned coset ---------------------------------------------------------------------------------------------------------
PINNED = {"arith32": (2, 5), "arith64_R64": (2, 3)}     # circuit -> one even and one odd coset


def pinned_cases(pkg, orc, name):
    b = circuit(pkg, orc, name)
    cir, out = b.cir, []
    for r in PINNED[name]:
        seed = 500 + r
        while True:
            rng = np.random.default_rng(seed)
            wires = rand_words(rng, (cir.W, cir.n))
            for j in range(cir.R):
                wires[j] = psm.pin_coset(orc, cir, r, [EDGE[i] for i in rng.integers(0, len(EDGE), size=cir.n)])
            zp_in = np.stack([psm.pin_coset(orc, cir, r, [EDGE[i] for i in rng.integers(0, len(EDGE), size=cir.n)]) for _ in range(cir.nzp)])
            be, al = rand_list(rng, cir.K), rand_list(rng, cir.K)
            ga = [P - 1, 1 << 32][:cir.K]
            if psm.denominators_nonzero(cir, wires, be, ga):
                break
            seed += 1000
        wl = psm.lde(orc, cir, wires[:cir.R])[:, r::cir.C]
        zl = psm.lde(orc, cir, zp_in)[:, r::cir.C]
        edge = np.array(EDGE, dtype=np.uint64)
        assert np.isin(wl, edge).all() and np.isin(zl, edge).all()
        acct = {"coset": r, "parity": r & 1, "wire_words": int(wl.size), "zp_words": int(zl.size),
                "z_minus_1_wraps": int((zl[:cir.K] == 0).sum()),                                    # Z - 1 on Z = 0
                "wv_plus_gamma_wraps": int(sum(((wl.astype(object) + g) >= P).sum() for g in ga))}   # wv + gamma >= p
        out.append(Case("pinned-%s-coset%d" % (name, r), name, wires, rand_list(rng, 4), be, ga, al, zp_in=zp_in, account=acct))
    return out


# ---- 5. steered raw words ------------------------------------------------------------------------------------------------------
STEERED = {"arith32": 3, "arith64_R64": 1}              # circuit -> the coset that is pinned


def zs_raw_products(cir, wires, i, beta, gamma, m):
    """By psm.raw_nc, the raw running products of chunk m in subgroup row i as the comment in zs_chunk_kernel has them: they
    start at 1 and take the chunk's factors in column order; canonical once per chunk."""
    bx = beta * cir.sub[i] % P
    rn = rd = 1
    for j in range(m * cir.QF, min((m + 1) * cir.QF, cir.R)):
        wg = (int(wires[j, i]) + gamma) % P
        rn = psm.raw_mul(rn, psm.raw_mul_add(bx, cir.k_is[j], wg))
        rd = psm.raw_mul(rd, psm.raw_mul_add(beta, int(cir.sigmas[j, i]), wg))
    return rn, rd


def steered_zs_case(pkg, orc, name):
    """Subgroup rows whose chunk products are raw words >= p at the point zs_chunk_kernel makes them canonical."""
    b = circuit(pkg, orc, name)
    cir = b.cir
    rng = np.random.default_rng(700)
    wires = rand_words(rng, (cir.W, cir.n))
    be, ga, al = (rand_list(rng, cir.K) for _ in range(3))
    hits = {"num": 0, "den": 0}
    for row, m, which in ((1, 0, "num"), (2, cir.nchunks - 1, "den"), (cir.n - 1, 1, "num"), (cir.n // 2, 0, "den")):
        cols = list(range(m * cir.QF, min((m + 1) * cir.QF, cir.R)))
        num, den = psm.factors(cir, wires, be[0], ga[0])
        rest = 1
        for j in cols[:-1]:
            rest = rest * int((num if which == "num" else den)[j, row]) % P
        for v in range(1, 64):                                              # product = v < 2^32: the raw word is v or v + p
            psm.target_factor(cir, wires, cols[-1], row, v * psm.inv(rest) % P, be[0], ga[0], which)
            raw = zs_raw_products(cir, wires, row, be[0], ga[0], m)[0 if which == "num" else 1]
            assert raw % P == v
            if raw >= P:
                hits[which] += 1
                break
    assert psm.denominators_nonzero(cir, wires, be, ga)
    return Case("steered-zs-" + name, name, wires, rand_list(rng, 4), be, ga, al, account={"raw_canonicalised": hits})


def steered_quotient_case(pkg, orc, name):
    """One pinned coset on which, at chosen indices and for challenge 0, the model's account of prev * n, of next * d (with
    prev = 0, so that the difference borrows) and of filter * sum for the ArithmeticGate is a raw word >= p."""
    b = circuit(pkg, orc, name)
    cir, r = b.cir, STEERED[name]
    assert cir.W == cir.R, "every wire of the row is pinned"
    rng = np.random.default_rng(800)
    be, ga, al = (rand_list(rng, cir.K) for _ in range(3))
    pih = rand_list(rng, 4)
    tw = [[int(x) for x in rand_words(rng, cir.n)] for _ in range(cir.R)]          # the LDE words on coset r: wires ...
    tz = [[int(x) for x in rand_words(rng, cir.n)] for _ in range(cir.nzp)]        # ... and Z / partial products
    pts = [cir.pts[cir.C * k + r] for k in range(cir.n)]
    sg = b.cs_lde[cir.NC:, r::cir.C]
    K, k1, k2, k3, k4 = cir.K, 3, 9, 17, 22
    acct = {"prev_n": 0, "next_d": 0, "next_d_last_chunk": 0, "f_sum": 0}

    def steer_chunk(k, m, which, other):
        """make (other * chunk product) a small value whose raw word, by the account, is >= p"""
        cols = list(range(m * cir.QF, min((m + 1) * cir.QF, cir.R)))
        j = cols[-1]
        wl = [tw[c][k] for c in range(cir.R)]
        rest = other
        for c in cols[:-1]:
            side = cir.k_is[c] * pts[k] if which == "num" else int(sg[c, k])
            rest = rest * ((wl[c] + be[0] * side + ga[0]) % P) % P
        side = cir.k_is[j] * pts[k] if which == "num" else int(sg[j, k])
        for v in range(1, 64):
            tw[j][k] = (v * psm.inv(rest) - be[0] * side - ga[0]) % P
            wl[j] = tw[j][k]
            raw = psm.chunk_raw_products(cir, wl, sg[:, k], pts[k], be[0], ga[0], m)[0 if which == "num" else 1]
            if psm.raw_mul(other, raw) >= P:
                assert psm.raw_mul(other, raw) % P == v
                return 1
        return 0

    acct["prev_n"] = steer_chunk(k1, 0, "num", tz[0][k1])                          # prev of chunk 0: Z_0
    tz[0][k2] = 0                                                                  # prev * n = 0 < next * d: the difference wraps
    acct["next_d"] = steer_chunk(k2, 0, "den", tz[K][k2])                          # next of chunk 0: the first partial product
    tz[K + cir.PP - 1][k4] = 0                                                     # last chunk: prev is the last partial product,
    acct["next_d_last_chunk"] = steer_chunk(k4, cir.nchunks - 1, "den", tz[0][(k4 + 1) % cir.n])   # next is Z_0 of the NEXT index
    # filter * sum of the ArithmeticGate at index k3: move the output wire of operation 0 until the folded sum is v / filter
    gi = next(i for i, g in enumerate(cir.gates) if g["kind"] == 3)
    g = cir.gates[gi]
    f = int(psm.gate_filter(cir, gi, psm.obj(b.cs_lde[g["sel"], r::cir.C][k3:k3 + 1]))[0])
    consts = [int(x) for x in b.cs_lde[cir.num_selectors:cir.NC, r::cir.C][:, k3]]
    tg = K + K * cir.nchunks

    def folded(row):
        cons = orc.gate_eval(g["kind"], g["params"], np.array(row, dtype=np.uint64), consts=consts, pi_hash=pih)
        return sum(pow(al[0], tg + t, P) * int(c) for t, c in enumerate(cons)) % P

    row = [tw[c][k3] for c in range(cir.R)]
    s0 = folded(row)
    row[3] = (row[3] + 1) % P
    slope = (folded(row) - s0) % P                                                 # the sum is affine in the output wire
    assert f and slope
    for v in range(1, 64):
        row[3] = (tw[3][k3] + (v * psm.inv(f) - s0) * psm.inv(slope)) % P
        s = folded(row)
        assert f * s % P == v
        if psm.raw_mul(f, s) >= P:
            tw[3][k3] = row[3]
            acct["f_sum"] = 1
            break
    wires = np.stack([psm.pin_coset(orc, cir, r, col) for col in tw])
    zp_in = np.stack([psm.pin_coset(orc, cir, r, col) for col in tz])
    assert psm.denominators_nonzero(cir, wires, be, ga)
    assert np.array_equal(psm.lde(orc, cir, wires)[:, r::cir.C], np.array(tw, dtype=np.uint64))
    return Case("steered-quotient-%s-coset%d" % (name, r), name, wires, pih, be, ga, al, zp_in=zp_in, account=acct)


FAMILIES = {
    "edges": lambda pkg, orc: [c for n in EDGE_CIRCUITS for c in edge_cases(pkg, orc, n)],
    "targets": lambda pkg, orc: [c for n in TARGETS for c in target_cases(pkg, orc, n)],
    "pinned": lambda pkg, orc: [c for n in PINNED for c in pinned_cases(pkg, orc, n)],
    "steered": lambda pkg, orc: [f(pkg, orc, n) for n in STEERED for f in (steered_zs_case, steered_quotient_case)],
}
_cases = {}


def family(pkg, orc, name):
    if name not in _cases:
        _cases[name] = FAMILIES[name](pkg, orc)
    return _cases[name]
