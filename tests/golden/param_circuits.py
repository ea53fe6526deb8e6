"""Circuits across the parameter space the circuit blob loader accepts (test infrastructure).

The synthetic workload generator (csrc/synth.cpp) and mini_builder.py both fix the reference's shape: K = 2 challenges,
rate_bits = 3 (QF = 8), 80 routed wires, an all-4 FRI arity schedule.  This module makes circuits off that shape:

  * ``arith_circuit``: ArithmeticGate rows (num_ops = R / 4, every wire routed) whose witness satisfies
    out = c0 * m0 * m1 + c1 * addend, copy chains from earlier outputs and from Constant cells into later inputs, one
    PublicInputGate row, Constant rows, Noop padding.  Fits rate_bits 2 and 3 (ArithmeticGate has degree 3).
  * ``degree1_circuit``: Constant, PublicInput and Noop rows only (degree 1), copy chains between Constant cells of equal
    value and between free cells of Noop rows -- what fits max_degree 3 at rate_bits 1 (QF = 2).
  * ``with_params``: a header patch of a synth blob for the four parameters that appear in no blob table (K, the FRI
    arity schedule, PoW bits, query count).

The circuits come as the inputs of ``builder.build()`` (gate declarations, row -> gate, gate constants, copy pairs); the
caller passes the build functions to run them through (the product's p2gpu_build_blob and the oracle's orc_build_blob), and
every one of them must return the same bytes.  Pure Python/numpy: uses neither oracle/ nor the product.
"""
import ctypes

import numpy as np

P = 0xFFFFFFFF00000001
G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC = 0, 1, 2, 3
_FLAGS_WORD = 25


class BuildParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("degree_bits", "num_wires", "num_routed_wires", "num_challenges", "quotient_degree_factor",
                                                "rate_bits", "cap_height", "proof_of_work_bits", "num_query_rounds", "num_public_inputs")]


class GateDecl(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("p", ctypes.c_uint32 * 4), ("degree", ctypes.c_uint32), ("num_constants", ctypes.c_uint32)]


def build_fn(fn):
    """Give a ctypes build function (p2gpu_build_blob / orc_build_blob) its argument types."""
    fn.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p,
                   ctypes.c_size_t, ctypes.c_void_p, ctypes.POINTER(ctypes.c_size_t)]
    return fn


def _run_build(fn, params, decl, row_gate, consts, copies):
    gates = (GateDecl * len(decl))()
    for i, (kind, p0, deg, nk) in enumerate(decl):
        gates[i].kind, gates[i].degree, gates[i].num_constants = kind, deg, nk
        gates[i].p[0] = p0
    rg = np.ascontiguousarray(row_gate, dtype=np.uint32)
    gc = np.ascontiguousarray(consts, dtype=np.uint64)
    cp = np.ascontiguousarray(copies, dtype=np.uint32).reshape(-1, 4)
    ln = ctypes.c_size_t(0)
    args = [ctypes.byref(params), gates, len(decl), rg.ctypes.data_as(ctypes.c_void_p), gc.ctypes.data_as(ctypes.c_void_p),
            cp.ctypes.data_as(ctypes.c_void_p) if cp.size else None, ctypes.c_size_t(len(cp))]
    rc = fn(*args, None, ctypes.byref(ln))
    assert rc == 0, f"build probe failed: {rc}"
    out = np.zeros(ln.value, dtype=np.uint8)
    rc = fn(*args, out.ctypes.data_as(ctypes.c_void_p), ctypes.byref(ln))
    assert rc == 0, f"build failed: {rc}"
    return out[:ln.value]


def _build_all(builders, params, decl, row_gate, consts, copies):
    """Run every build function; all must agree byte for byte (as tests/test_build.py asks of synth blobs)."""
    blobs = [_run_build(fn, params, decl, row_gate, consts, copies) for fn in builders]
    assert blobs, "at least one build function is needed"
    for b in blobs[1:]:
        assert b.tobytes() == blobs[0].tobytes(), "the build functions disagree"
    return blobs[0]


def arith_circuit(d, R, W, K, rate_bits, cap_h, seed, builders, pow_bits=16, queries=28):
    """A satisfiable circuit of ArithmeticGate rows with R routed wires (R a multiple of 4, num_ops = R / 4), W wires in all,
    K challenges, QF = 2^rate_bits.  builders: the build functions to run (see module doc).  Returns (blob, wires)."""
    assert R % 4 == 0 and W >= R and d >= 3 and rate_bits >= 2, "ArithmeticGate (degree 3) needs QF >= 4"
    rng = np.random.default_rng(seed)
    n, ops = 1 << d, R // 4
    n_const = 2
    n_arith = n - 1 - n_const - max(1, n // 8)         # leave Noop rows at the end
    pi_row = n_arith
    c_rows = [pi_row + 1 + i for i in range(n_const)]
    wires = np.zeros((W, n), dtype=np.uint64)
    consts = np.zeros((2, n), dtype=np.uint64)
    copies = []
    # Constant rows: two constants each, wire j holds constant j
    const_cells = []
    for r in c_rows:
        for j in range(2):
            v = int(rng.integers(0, P, dtype=np.uint64))
            consts[j, r] = v
            wires[j, r] = v
            const_cells.append((r, j))
    # ArithmeticGate rows: per-row (c0, c1), random inputs, some inputs copied from earlier outputs or Constant cells
    outs = []
    for r in range(n_arith):
        c0, c1 = (int(x) for x in rng.integers(0, P, size=2, dtype=np.uint64))
        consts[0, r], consts[1, r] = c0, c1
        for i in range(ops):
            m0, m1, ad = (int(x) for x in rng.integers(0, P, size=3, dtype=np.uint64))
            col = 4 * i
            if outs and rng.random() < 0.5:            # chain: m0 is an earlier output
                sr, sc = outs[int(rng.integers(0, len(outs)))]
                m0 = int(wires[sc, sr])
                copies.append((sr, sc, r, col))
            if rng.random() < 0.2:                     # chain: the addend is a Constant cell
                sr, sc = const_cells[int(rng.integers(0, len(const_cells)))]
                ad = int(wires[sc, sr])
                copies.append((sr, sc, r, col + 2))
            out = (c0 * m0 % P * m1 + c1 * ad) % P
            wires[col:col + 4, r] = (m0, m1, ad, out)
            outs.append((r, col + 3))
    # PublicInputGate row: the hash of zero public inputs is four zeros; plonky2 randomises every other wire of the row
    wires[4:, pi_row] = rng.integers(0, P, size=W - 4, dtype=np.uint64)
    decl = [(G_NOOP, 0, 0, 0), (G_CONSTANT, 2, 1, 2), (G_PUBLIC_INPUT, 0, 1, 0), (G_ARITHMETIC, ops, 3, 2)]
    row_gate = np.zeros(n, dtype=np.uint32)
    row_gate[:n_arith] = 3
    row_gate[pi_row] = 2
    row_gate[c_rows] = 1
    params = BuildParams(d, W, R, K, 1 << rate_bits, rate_bits, cap_h, pow_bits, queries, 0)
    blob = _build_all(builders, params, decl, row_gate, consts, np.array(copies, dtype=np.uint32).reshape(-1, 4))
    return blob, wires


def degree1_circuit(d, R, W, K, rate_bits, cap_h, seed, builders, pow_bits=16, queries=28):
    """A satisfiable circuit of degree-1 gates only (Constant, PublicInput, Noop): fits rate_bits 1 (max_degree 3).
    Copy chains tie Constant cells of equal value together and free cells of Noop rows to each other."""
    assert W >= R >= 4 and d >= 3
    rng = np.random.default_rng(seed)
    n = 1 << d
    n_const = n // 4
    pi_row = 0
    c_rows = list(range(1, 1 + n_const))
    noop_rows = list(range(1 + n_const, n))
    wires = np.zeros((W, n), dtype=np.uint64)
    consts = np.zeros((2, n), dtype=np.uint64)
    copies = []
    pool = [int(x) for x in rng.integers(0, P, size=5, dtype=np.uint64)]   # few distinct values: chains of equal constants
    last_cell = {}
    for r in c_rows:
        for j in range(2):
            v = pool[int(rng.integers(0, len(pool)))]
            consts[j, r] = v
            wires[j, r] = v
            if v in last_cell:
                copies.append(last_cell[v] + (r, j))
            last_cell[v] = (r, j)
    for r in noop_rows:
        wires[:, r] = rng.integers(0, P, size=W, dtype=np.uint64)
    prev = None
    for r in noop_rows[: len(noop_rows) // 2]:        # a long cycle through routed cells of Noop rows
        col = int(rng.integers(0, R))
        if prev is not None:
            wires[col, r] = wires[prev[1], prev[0]]
            copies.append(prev + (r, col))
        prev = (r, col)
    wires[4:, pi_row] = rng.integers(0, P, size=W - 4, dtype=np.uint64)
    decl = [(G_NOOP, 0, 0, 0), (G_CONSTANT, 2, 1, 2), (G_PUBLIC_INPUT, 0, 1, 0)]
    row_gate = np.zeros(n, dtype=np.uint32)
    row_gate[pi_row] = 2
    row_gate[c_rows] = 1
    params = BuildParams(d, W, R, K, 1 << rate_bits, rate_bits, cap_h, pow_bits, queries, 0)
    blob = _build_all(builders, params, decl, row_gate, consts, np.array(copies, dtype=np.uint32).reshape(-1, 4))
    return blob, wires


def with_params(blob, K=None, arity=None, pow_bits=None, queries=None):
    """A copy of a circuit blob with other num_challenges / FRI arity bits / PoW bits / query rounds.  None of the four is
    part of a blob table, and a blob with flags 0 carries no digest (the digest is derived at create), so patching the header
    is all it takes."""
    b = np.array(blob, dtype=np.uint8, copy=True)
    h = b[:256].view(np.uint32)
    assert h[0] == 0x43473250 and int(h[_FLAGS_WORD]) == 0, "only blobs without a stored cap or digest can be patched"
    if K is not None:
        h[7] = K
    if arity is not None:
        h[13] = len(arity)
        h[14:22] = 0
        for i, a in enumerate(arity):
            h[14 + i] = a
    if pow_bits is not None:
        h[11] = pow_bits
    if queries is not None:
        h[12] = queries
    return b


def patch_header(blob, **words):
    """A copy of a blob with raw header words replaced: {"w<index>": value} (for the refusal tests)."""
    b = np.array(blob, dtype=np.uint8, copy=True)
    h = b[:256].view(np.uint32)
    for k, v in words.items():
        h[int(k[1:])] = v
    return b


def xchg_words(blob, world, new=True):
    """Words of the sharded exchange buffer for this circuit (handle.hip shard_layout), by the formula before the fix of the
    FRI batch reduction's all-gather (new=False: max(G * gather_cap, K * C * n) + 64) or after it (also 2 * G * n), and the
    words the shard_reduce all-gather writes there: 2 * G * n."""
    h = np.frombuffer(bytes(blob[:256]), dtype=np.uint32)
    d, W, R, NC, K, QF, rate, cap_h, queries = (int(h[i]) for i in (2, 3, 4, 5, 7, 8, 9, 10, 12))
    arity = [int(x) for x in h[14:14 + int(h[13])]]
    PP = int(h[26])
    n, C = 1 << d, 1 << rate
    nall = NC + R + W + K * (1 + PP) + K * QF
    gw, ds = 0, d
    for ab in arity:
        gw += (2 << ab) + 4 * (ds + rate)
        ds -= ab
    gw += nall + 16 * (d + rate)
    gather_cap = gw * queries + 64
    terms = [world * gather_cap, K * C * n] + ([2 * world * n] if new else [])
    return max(terms) + 64, 2 * world * n
