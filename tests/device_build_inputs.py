"""Inputs of build() for the device-build tests (test infrastructure): a circuit blob taken apart into gate declarations,
row -> gate, gate constants and copy pairs, vectorised so that 2^17-row circuits take seconds (tests/test_build.py's
``decompose`` is a Python loop over every routed cell), and hand-made copy sets that stress the union-find."""
import ctypes

import numpy as np

G_NOOP = 0


def header_kwargs(blob):
    h = np.frombuffer(bytes(blob[:256]), dtype=np.uint32)
    return dict(degree_bits=int(h[2]), num_wires=int(h[3]), num_routed_wires=int(h[4]), num_challenges=int(h[7]),
                quotient_degree_factor=int(h[8]), rate_bits=int(h[9]), cap_height=int(h[10]), proof_of_work_bits=int(h[11]),
                num_query_rounds=int(h[12]), num_public_inputs=int(h[24]))


def decompose(pkg, blob):
    """blob -> keyword arguments of ``pkg.build_blob`` / ``pkg.CircuitData.build``.  The copy pairs are the edges
    x -> sigma(x) of every cycle: sigma is inverted by sorting the identity permutation's values (the sigma table
    p2gpu_build_blob gives for the same circuit without copy pairs) and looking every sigma value up in them."""
    blob = np.ascontiguousarray(blob)
    kw = header_kwargs(blob)
    h = blob[:256].view(np.uint32)
    d, R, NC, nsel, ng = kw["degree_bits"], kw["num_routed_wires"], int(h[5]), int(h[6]), int(h[23])
    n = 1 << d
    assert int(h[25]) == 0, "a blob with a stored cap / digest has another layout"
    gt = blob[256:256 + 48 * ng].view(np.uint32).reshape(ng, 12)
    gates = [(int(g[0]), tuple(int(x) for x in g[1:5]), int(g[9]), int(g[10])) for g in gt]
    off = 256 + 48 * ng + 8 * R
    consts = blob[off:off + 8 * NC * n].view(np.uint64).reshape(NC, n)
    off += 8 * NC * n
    sig = blob[off:off + 8 * R * n].view(np.uint64).reshape(-1)
    sel = consts[:nsel]
    if nsel == 1:
        row_gate = sel[0].astype(np.uint32)
    else:
        used = sel != 0xFFFFFFFF
        assert (used.sum(axis=0) == 1).all()
        row_gate = np.where(used, sel, 0).sum(axis=0).astype(np.uint32)
    row_constants = np.ascontiguousarray(consts[nsel:])
    kw.update(gates=gates, row_gate=row_gate, row_constants=row_constants)
    ident_blob = pkg.build_blob(copies=np.zeros((0, 4), dtype=np.uint32), **kw)
    ident = ident_blob[off:off + 8 * R * n].view(np.uint64)
    order = np.argsort(ident, kind="stable")
    at = np.searchsorted(ident[order], sig)
    assert (ident[order][at] == sig).all()
    target = order[at]                               # flat index col * n + row of sigma(x)
    x = np.nonzero(target != np.arange(R * n))[0]
    y = target[x]
    copies = np.stack([x % n, x // n, y % n, y // n], axis=1).astype(np.uint32)
    kw["copies"] = np.ascontiguousarray(copies)
    return kw


def with_hasher(blob, hasher):
    b = np.array(blob, dtype=np.uint8, copy=True)
    b[:256].view(np.uint32)[22] = hasher
    return b


def noop_circuit(d, copies, R=80, W=234):
    """2^d NoopGate rows, no constants: nothing but the copy pairs decides the sigma table."""
    n = 1 << d
    return dict(degree_bits=d, gates=[(G_NOOP, (), 0, 0)], row_gate=np.zeros(n, dtype=np.uint32),
                row_constants=np.zeros((0, n), dtype=np.uint64), copies=np.ascontiguousarray(copies, dtype=np.uint32).reshape(-1, 4),
                num_wires=W, num_routed_wires=R)


def _cells(rng, d, R, count):
    """`count` distinct routed cells as (row, col) rows."""
    n = 1 << d
    flat = rng.choice(R * n, size=count, replace=False)
    return np.stack([flat // R, flat % R], axis=1).astype(np.uint32)


def _pairs(a, b):
    return np.concatenate([a, b], axis=1).astype(np.uint32)


def stress_copy_sets(R=80):
    """name -> (d, copies[m][4]): the copy sets the union-find has to get right whatever order its atomics land in."""
    rng = np.random.default_rng(2024)
    out = {}
    # random small classes, every pair listed twice
    c = _cells(rng, 10, R, 4000)
    base = _pairs(c[:-1], c[1:])[np.arange(3999) % 4 != 3]
    out["every_pair_twice"] = (10, np.concatenate([base, base]))
    # pairs (a, a) only, and mixed in between real ones
    out["self_pairs_only"] = (10, _pairs(c[:500], c[:500]))
    mixed = np.concatenate([base[:1000], _pairs(c[:500], c[:500]), base[1000:]])
    out["self_pairs_mixed"] = (10, mixed)
    # shuffled order, ends swapped at random
    sh = base[rng.permutation(len(base))].copy()
    swap = rng.random(len(sh)) < 0.5
    sh[swap] = sh[swap][:, [2, 3, 0, 1]]
    out["shuffled_and_swapped"] = (11, sh)
    # one chain through a whole column, given last row first
    n = 1 << 14
    rows = np.arange(n - 1, 0, -1, dtype=np.uint32)
    col = np.full(n - 1, 7, dtype=np.uint32)
    out["column_chain_last_row_first"] = (14, np.stack([rows, col, rows - 1, col], axis=1))
    # the same chain first row first: every pair finds a long tail behind it
    out["column_chain_first_row_first"] = (14, np.stack([rows[::-1] - 1, col, rows[::-1], col], axis=1))
    # a star: 2^15 cells copied to one hub, the hub's key above / below its leaves
    cells = _cells(rng, 12, R, (1 << 15) + 1)
    key = cells[:, 0].astype(np.int64) * R + cells[:, 1]
    srt = cells[np.argsort(key)]
    for name, hub, leaves in (("star_hub_last", srt[-1:], srt[:-1]), ("star_hub_first", srt[:1], srt[1:]),
                              ("star_hub_middle", srt[1000:1001], np.concatenate([srt[:1000], srt[1001:]]))):
        leaves = leaves[rng.permutation(len(leaves))]
        out[name] = (12, _pairs(np.repeat(hub, len(leaves), axis=0), leaves))
    # two stars joined by their last pair
    a, b = srt[:5000], srt[5000:10000]
    sa = _pairs(np.repeat(a[-1:], 4999, axis=0), a[:-1])
    sb = _pairs(np.repeat(b[:1], 4999, axis=0), b[1:])
    out["two_stars_joined_last"] = (12, np.concatenate([sa, sb, _pairs(a[17:18], b[4000:4001])]))
    # every routed cell in one class: a random spanning tree over all R * n cells
    d = 10
    tot = R << d
    perm = rng.permutation(tot)
    par = perm[(rng.random(tot - 1) * np.arange(1, tot)).astype(np.int64)]    # node i + 1 hangs under a random earlier node
    ch = perm[1:]
    tree = np.stack([ch // R, ch % R, par // R, par % R], axis=1).astype(np.uint32)
    out["all_cells_one_class"] = (d, tree[rng.permutation(len(tree))])
    out["no_copies"] = (10, np.zeros((0, 4), dtype=np.uint32))
    return out


class BuildParams(ctypes.Structure):
    _fields_ = [(k, ctypes.c_uint32) for k in ("degree_bits", "num_wires", "num_routed_wires", "num_challenges", "quotient_degree_factor",
                                                "rate_bits", "cap_height", "proof_of_work_bits", "num_query_rounds", "num_public_inputs")]


class GateDecl(ctypes.Structure):
    _fields_ = [("kind", ctypes.c_uint32), ("p", ctypes.c_uint32 * 4), ("degree", ctypes.c_uint32), ("num_constants", ctypes.c_uint32)]


def raw_build_args(kw):
    """The ctypes arguments of p2gpu_circuit_build (without hasher and out) for a keyword set with every parameter given."""
    bp = BuildParams(*[kw[k] for k, _ in BuildParams._fields_])
    gd = (GateDecl * len(kw["gates"]))()
    for i, (kind, ps, deg, nk) in enumerate(kw["gates"]):
        gd[i].kind, gd[i].degree, gd[i].num_constants = kind, deg, nk
        for j, v in enumerate(tuple(ps) + (0,) * (4 - len(ps))):
            gd[i].p[j] = v
    return bp, gd
