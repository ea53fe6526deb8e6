"""Prover phases 2 and 3 in Python integers (test infrastructure): what `CircuitData.plonk_stages` must return, word for word.

Written from oracle/prover.c and SURVEY.md C.5 / C.7, for ANY wire matrix, challenges and Z / partial-product override:

  * `zs`: for each row the QF-sized chunks of (beta x k_j + w + gamma) / (beta sigma_j + w + gamma), then the running product
    (Z_c, then the partial products of every challenge); sigmas and k_is come from the blob;
  * `quotient_values`: at every LDE point x = g w_N^i the terms L_0(x) (Z_c - 1), the chunk checks
    prev prod(num) - next prod(den), the selector-filtered gate constraints (oracle/pyoracle.py gate_eval on the row's LDE
    words; the filter restated here), folded by each alpha, divided by x^n - 1;
  * `quotient_chunks`: the size-N coset interpolation of those values cut into 2^rate_bits chunks of n coefficients -- well
    defined whether or not the wires satisfy the circuit.

Column LDEs are the oracle's (orc.ntt, orc.coset_lde); all field arithmetic on top of them is Python integers (numpy object
arrays where a whole column is handled at once).  The input builders at the end choose wires and overrides that put edge words
where the kernels of csrc/plonk.hip could go wrong; `raw_nc` restates ONE formula of the device code (the comment of
gl_reduce_words_nc in csrc/gl.hpp) and serves only to choose inputs, never to decide pass or fail.
"""
import numpy as np

P = 0xFFFFFFFF00000001
GEN = 14293326489335486720      # plonky2's coset shift
ROOT32 = 7277203076849721926     # generator of the subgroup of order 2^32
M32, M64 = (1 << 32) - 1, (1 << 64) - 1
EDGE = [0, 1, 2, M32, 1 << 32, P - (1 << 32), P - 2, P - 1]


def inv(a):
    assert a % P, "inverse of zero"
    return pow(a, P - 2, P)


def root(lg):
    return pow(ROOT32, 1 << (32 - lg), P)


def obj(a):
    """uint64 array -> array of Python integers"""
    return np.asarray(a).astype(object)


def u64(a):
    return np.array(a, dtype=np.uint64)


class Circuit:
    """The tables of a circuit blob (include/p2gpu.h) that phases 2 and 3 read."""

    def __init__(self, blob):
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        h = blob[:256].view(np.uint32)
        assert h[0] == 0x43473250
        self.d, self.W, self.R, self.NC, self.num_selectors, self.K, self.QF, self.rate_bits, self.cap_h = (int(h[i]) for i in range(2, 11))
        self.num_gates, self.flags, self.PP = int(h[23]), int(h[25]), int(h[26])
        self.n, self.C = 1 << self.d, 1 << self.rate_bits
        self.N = self.n * self.C
        assert self.QF == self.C
        self.nchunks = -(-self.R // self.QF)
        assert self.PP == self.nchunks - 1
        off = 256
        g = blob[off:off + 48 * self.num_gates].view(np.uint32).reshape(self.num_gates, 12)
        self.gates = [dict(kind=int(r[0]), params=[int(x) for x in r[1:5]], sel=int(r[5]), gs=int(r[6]), ge=int(r[7]), nc=int(r[8]),
                           nconst=int(r[10])) for r in g]
        off += 48 * self.num_gates
        if self.flags & 2:
            off += 32 << self.cap_h
        self.k_is = [int(x) for x in blob[off:off + 8 * self.R].view(np.uint64)]
        off += 8 * self.R
        self.constants = blob[off:off + 8 * self.NC * self.n].view(np.uint64).reshape(self.NC, self.n).copy()
        off += 8 * self.NC * self.n
        self.sigma_off = off
        self.sigmas = blob[off:off + 8 * self.R * self.n].view(np.uint64).reshape(self.R, self.n).copy()
        self.NGC = max(g["nc"] for g in self.gates)
        self.nzp = self.K * (1 + self.PP)
        self.omega = root(self.d)
        self.sub = [pow(self.omega, i, P) for i in range(self.n)]            # the subgroup, row i -> w^i
        wN = root(self.d + self.rate_bits)
        self.pts = [GEN * pow(wN, i, P) % P for i in range(self.N)]           # the LDE points, natural order

    def coset_shift(self, r):
        return self.pts[r]                                                     # g w_N^r: coset r is pts[r::C]


# ---- phase 2 ---------------------------------------------------------------------------------------------------------------
def factors(cir, wires, beta, gamma):
    """(num, den) [R][n], Python integers: beta k_j w^i + w + gamma and beta sigma_j[i] + w + gamma."""
    w = obj(wires[:cir.R])
    x = np.array(cir.sub, dtype=object)
    num = np.empty((cir.R, cir.n), dtype=object)
    den = np.empty((cir.R, cir.n), dtype=object)
    for j in range(cir.R):
        num[j] = (w[j] + beta * (cir.k_is[j] * x % P) + gamma) % P
        den[j] = (w[j] + beta * obj(cir.sigmas[j]) + gamma) % P
    return num, den


def denominators_nonzero(cir, wires, betas, gammas):
    return all((factors(cir, wires, b, g)[1] != 0).all() for b, g in zip(betas, gammas))


def zs(cir, wires, betas, gammas):
    """[K (1 + PP)][n] uint64: Z of every challenge, then the partial products (oracle/prover.c step 3)."""
    out = np.zeros((cir.nzp, cir.n), dtype=np.uint64)
    for c in range(cir.K):
        num, den = factors(cir, wires, betas[c], gammas[c])
        assert (den != 0).all(), "a zero denominator: the oracle does not define this case"
        z = 1
        for i in range(cir.n):
            out[c, i] = z
            acc = z
            for m in range(cir.nchunks):
                q = 1
                for j in range(m * cir.QF, min((m + 1) * cir.QF, cir.R)):
                    q = q * int(num[j, i]) % P * inv(int(den[j, i])) % P
                acc = acc * q % P
                if m < cir.PP:
                    out[cir.K + c * cir.PP + m, i] = acc
            z = acc
    return out


# ---- phase 3 ---------------------------------------------------------------------------------------------------------------
def lde(orc, cir, vals):
    """[cols][n] values over the subgroup -> [cols][N] on the coset g <w_N>, natural order"""
    return np.stack([orc.coset_lde(orc.ntt(col, inverse=True), cir.rate_bits) for col in np.asarray(vals, dtype=np.uint64)])


def gate_filter(cir, gi, s):
    """gates/selectors.rs compute_filter on a column of selector words (Python integers)"""
    g = cir.gates[gi]
    f = np.full(s.shape, 1, dtype=object)
    for i in range(g["gs"], g["ge"]):
        if i != gi:
            f = f * ((i - s) % P) % P
    if cir.num_selectors > 1:
        f = f * ((M32 - s) % P) % P
    return f


def gate_terms(orc, cir, cs_lde, w_lde, pi_hash):
    """[NGC][N] Python integers: sum over the gates of filter * constraint, at every LDE point"""
    lib = orc.lib()
    rows = np.ascontiguousarray(w_lde.T)                                            # [N][W]
    ngc = cir.NC - cir.num_selectors
    consts = np.zeros((cir.N, ngc + 8), dtype=np.uint64)
    consts[:, :ngc] = cs_lde[cir.num_selectors:cir.NC].T
    pih = u64([int(x) for x in pi_hash])
    out = np.zeros(4096, dtype=np.uint64)
    tot = np.full((cir.NGC, cir.N), 0, dtype=object)
    for gi, g in enumerate(cir.gates):
        if not g["nc"]:
            continue
        p = np.array(g["params"], dtype=np.uint32)
        cons = np.zeros((cir.N, g["nc"]), dtype=np.uint64)
        for i in range(cir.N):
            k = lib.orc_gate_eval(g["kind"], p.ctypes.data, rows[i].ctypes.data, consts[i].ctypes.data, pih.ctypes.data, out.ctypes.data)
            assert k == g["nc"]
            cons[i] = out[:k]
        f = gate_filter(cir, gi, obj(cs_lde[g["sel"]]))
        tot[:g["nc"]] = (tot[:g["nc"]] + obj(cons.T) * f) % P
    return tot


def quotient_terms(orc, cir, wires, zp, betas, gammas, pi_hash):
    """The unfolded terms [c] -> [K + K nchunks + NGC][N] in the oracle's order (the gate terms are shared by the challenges)."""
    n, N, C, K = cir.n, cir.N, cir.C, cir.K
    cs_lde = lde(orc, cir, np.concatenate([cir.constants, cir.sigmas]))
    w_lde = lde(orc, cir, wires)
    z_lde = obj(lde(orc, cir, zp))
    x = np.array(cir.pts, dtype=object)
    gn = pow(GEN, n, P)
    wC = root(cir.rate_bits)
    zh = [(gn * pow(wC, r, P) - 1) % P for r in range(C)]
    zh_pt = np.array([zh[i % C] for i in range(N)], dtype=object)
    l0 = np.array([zh[i % C] * inv(n * (cir.pts[i] - 1) % P) % P for i in range(N)], dtype=object)
    nxt = (np.arange(N) + C) % N                                                     # Z(g x): the same coset, index k + 1
    terms = [l0 * ((z_lde[c] - 1) % P) % P for c in range(K)]
    wl, sg = obj(w_lde[:cir.R]), obj(cs_lde[cir.NC:])
    for c in range(K):
        for m in range(cir.nchunks):
            prev = z_lde[c] if m == 0 else z_lde[K + c * cir.PP + m - 1]
            nx = z_lde[c][nxt] if m == cir.nchunks - 1 else z_lde[K + c * cir.PP + m]
            np_, dp = 1, 1
            for j in range(m * cir.QF, min((m + 1) * cir.QF, cir.R)):
                np_ = np_ * ((wl[j] + betas[c] * (cir.k_is[j] * x % P) + gammas[c]) % P) % P
                dp = dp * ((wl[j] + betas[c] * sg[j] + gammas[c]) % P) % P
            terms.append((prev * np_ - nx * dp) % P)
    terms.extend(gate_terms(orc, cir, cs_lde, w_lde, pi_hash))
    return terms, zh_pt


def quotient_values(orc, cir, wires, zp, betas, gammas, alphas, pi_hash):
    """[K][N] uint64, natural LDE order"""
    terms, zh_pt = quotient_terms(orc, cir, wires, zp, betas, gammas, pi_hash)
    zhi = np.array([inv(int(v)) for v in zh_pt[:cir.C]] * cir.n, dtype=object)
    out = np.zeros((cir.K, cir.N), dtype=np.uint64)
    for c in range(cir.K):
        acc = np.full(cir.N, 0, dtype=object)
        for t in reversed(terms):
            acc = (acc * alphas[c] + t) % P
        out[c] = u64(list(acc * zhi % P))
    return out


def by_coset(cir, qv):
    """[K][N] natural order -> [K][C][n]: coset r, index k is LDE row C k + r"""
    return np.ascontiguousarray(qv.reshape(cir.K, cir.n, cir.C).transpose(0, 2, 1))


def quotient_chunks(orc, cir, qv):
    """[K C][n] uint64: natural-order coefficients of the chunk polynomials"""
    gi = inv(GEN)
    sc = np.array([pow(gi, e, P) for e in range(cir.N)], dtype=object)
    out = np.zeros((cir.K * cir.C, cir.n), dtype=np.uint64)
    for c in range(cir.K):
        co = u64(list(obj(orc.ntt(qv[c], inverse=True)) * sc % P))
        out[c * cir.C:(c + 1) * cir.C] = co.reshape(cir.C, cir.n)
    return out


def stages(orc, cir, wires, pi_hash, betas, gammas, alphas, zp_in=None):
    """What CircuitData.plonk_stages returns: zp, qvals [K][C][n], quot (no caps: those are the hash code's business)"""
    zp = zs(cir, wires, betas, gammas)
    used = zp if zp_in is None else np.asarray(zp_in, dtype=np.uint64)
    qv = quotient_values(orc, cir, wires, used, betas, gammas, alphas, pi_hash)
    return {"zp": zp, "qvals": by_coset(cir, qv), "quot": quotient_chunks(orc, cir, qv), "qv_natural": qv}


# ---- the quadratic extension (x^2 = 7), for evaluating at zeta ----------------------------------------------------------------
def ext_mul(a, b):
    return ((a[0] * b[0] + 7 * a[1] * b[1]) % P, (a[0] * b[1] + a[1] * b[0]) % P)


def eval_values_at(orc, vals, z):
    """The interpolant of `vals` (over the subgroup) at the extension point z"""
    co = [int(v) for v in orc.ntt(u64(vals), inverse=True)]
    return eval_coeffs_at(co, z)


def eval_coeffs_at(co, z):
    acc = (0, 0)
    for a in reversed(co):
        acc = ext_mul(acc, z)
        acc = ((acc[0] + int(a)) % P, acc[1])
    return acc


# ---- input builders ------------------------------------------------------------------------------------------------------------
def target_factor(cir, wires, j, i, t, beta, gamma, which):
    """(a) the wire word that makes the numerator ("num") or the denominator ("den") of cell (column j, row i) equal t"""
    other = cir.k_is[j] * cir.sub[i] % P if which == "num" else int(cir.sigmas[j, i])
    wires[j, i] = (t - beta * other - gamma) % P


def pin_coset(orc, cir, r, targets):
    """(b) the values over the subgroup of the polynomial of degree < n whose LDE words on coset r (points g w_N^r w^k) are
    `targets` [n]: a_e = intt(targets)[e] s_r^-e, values = ntt(a)"""
    si = inv(cir.coset_shift(r))
    co = obj(orc.ntt(u64([int(t) % P for t in targets]), inverse=True))
    sc = np.array([pow(si, e, P) for e in range(cir.n)], dtype=object)
    return orc.ntt(u64(list(co * sc % P)))


def raw_nc(x):
    """(c) the raw u64 of gl_reduce_words_nc for the 128-bit integer x = (w3 w2 w1 w0): with c = carry(w1 + w2),
    ((w1 + w2 + c) : w0) - (w2 + w3 + c), one wrap at most (then + p).  May be >= p."""
    assert 0 <= x < 1 << 128
    w0, w1, w2, w3 = (x >> s & M32 for s in (0, 32, 64, 96))
    c = (w1 + w2) >> 32
    r = ((((w1 + w2 + c) & M32) << 32) | w0) - (w2 + w3 + c)
    if r < 0:
        r += P
    assert 0 <= r <= M64 and r % P == x % P
    return r


def raw_mul(a, b):
    return raw_nc(a * b)


def raw_mul_add(a, b, c):
    return raw_nc(a * b + c)


def raw_pair(t=0, a=2):
    """Canonical (a, b) whose product's raw word is p + t' >= p for the smallest t' >= t that a divides: a * b = p + t' < 2^64,
    so the raw word of the product is the integer product itself."""
    while (P + t) % a:
        t += 1
    b = (P + t) // a
    assert b < P and P <= a * b <= M64 and raw_mul(a, b) == a * b
    return a, b


def chunk_raw_products(cir, wl, sg, x, beta, gamma, m):
    """By `raw_nc`, the raw running products (n, d) of chunk m at one LDE point, formed as the quotient kernel's comment says:
    they start at the chunk's first factor and are multiplied by each further factor of the chunk in column order."""
    bx = beta * x % P
    rn = rd = None
    for j in range(m * cir.QF, min((m + 1) * cir.QF, cir.R)):
        wg = (int(wl[j]) + gamma) % P
        fn, fd = raw_mul_add(bx, cir.k_is[j], wg), raw_mul_add(beta, int(sg[j]), wg)
        rn, rd = (fn, fd) if rn is None else (raw_mul(rn, fn), raw_mul(rd, fd))
    return rn, rd
