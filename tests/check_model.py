"""The expected report of the witness check (test infrastructure): what `CircuitData.check_witness` must say about a wire matrix,
computed from the circuit's BUILD KEYWORDS (gates, row -> gate, gate constants, copy pairs) -- never from the blob or the handle.

  * gate constraints: oracle/pyoracle.py's `gate_eval`, the oracle's independently written evaluator, on every row, with the
    oracle's Poseidon hash of the public inputs;
  * copy classes: a union-find over the copy pairs;
  * canonicity: the words >= p of the whole matrix; the two checks above see such a word reduced once (v - p).

The model predicts `gate_rows_failed`, `row_status`, the first gate finding and everything about canonicity exactly.  The order
of sigma's cycle inside a copy class is build()'s business, so for copies it promises only what does not depend on it
(`assert_report` (a)-(c); the tests add (d) and (e) where their corruption has that shape):
  (a) the count is zero if and only if every class is constant;
  (b) every flagged cell lies in a non-constant class, and every non-constant class holds a flagged cell;
  (c) `copy_cells_failed` is the popcount of `cell_flags`; the first finding is the lowest flagged key col << d | row, its partner
      lies in the same class, and both reported values are the matrix's.
"""
import contextlib
import sys
from collections import defaultdict

import numpy as np

P = 0xFFFFFFFF00000001
NONE = 0xFFFF


def poseidon_hash(orc, values):
    v = np.ascontiguousarray(np.array([int(x) for x in values], dtype=np.uint64))
    out = np.zeros(4, dtype=np.uint64)
    orc.lib().orc_poseidon_hash_no_pad(v.ctypes.data if v.size else None, v.size, out.ctypes.data)
    return [int(x) for x in out]


class Model:
    """The expected report of one matrix."""

    def __init__(self, orc, kw, wires, public_inputs=()):
        d = kw["degree_bits"]
        n = 1 << d
        gates, row_gate = kw["gates"], [int(g) for g in kw["row_gate"]]
        rc = np.asarray(kw["row_constants"], dtype=np.uint64).reshape(-1, n)
        self.d, self.n, self.R = d, n, kw.get("num_routed_wires", 80)
        self.raw = np.ascontiguousarray(wires, dtype=np.uint64)
        assert self.raw.shape == (kw.get("num_wires", 234), n)
        big = self.raw >= np.uint64(P)
        self.reduced = np.where(big, self.raw - np.uint64(P), self.raw)
        # ---- canonicity ----
        self.noncanonical_cells = int(big.sum())
        cols, rows = np.nonzero(big)                      # (column-major: the first hit is the lowest key col << d | row)
        self.first_noncanonical = (int(rows[0]), int(cols[0])) if self.noncanonical_cells else None
        # ---- gates ----
        pih = poseidon_hash(orc, public_inputs)
        self.row_status = np.full(n, NONE, dtype=np.uint16)
        self.first_gate = None
        for r in range(n):
            kind, params, _, nconst = gates[row_gate[r]]
            out = orc.gate_eval(kind, params, self.reduced[:, r], consts=[int(x) for x in rc[:nconst, r]], pi_hash=pih)
            nz = np.nonzero(out)[0]
            if nz.size:
                self.row_status[r] = int(nz[0])
                if self.first_gate is None:
                    self.first_gate = (r, row_gate[r], int(kind), int(nz[0]), int(out[nz[0]]))
        self.gate_rows_failed = int((self.row_status != NONE).sum())
        # ---- copy classes ----
        parent = {}

        def find(x):
            parent.setdefault(x, x)
            while parent[x] != x:
                parent[x] = parent[parent[x]]
                x = parent[x]
            return x

        for ra, ca, rb, cb in np.asarray(kw["copies"], dtype=np.int64).reshape(-1, 4):
            a, b = find((int(ra), int(ca))), find((int(rb), int(cb)))
            if a != b:
                parent[max(a, b)] = min(a, b)
        classes = defaultdict(list)
        for cell in list(parent):
            classes[find(cell)].append(cell)
        self.classes = [sorted(cl) for cl in classes.values() if len(cl) > 1]
        self.class_of = {cell: i for i, cl in enumerate(self.classes) for cell in cl}
        self.nonconstant = [i for i, cl in enumerate(self.classes) if len({int(self.reduced[c, r]) for r, c in cl}) > 1]

    @property
    def ok(self):
        return not (self.gate_rows_failed or self.nonconstant or self.noncanonical_cells)

    def assert_report(self, rep):
        """`rep`: a WitnessReport taken with details=True."""
        assert rep.gate_rows_failed == self.gate_rows_failed
        assert np.array_equal(rep.row_status, self.row_status), (np.nonzero(rep.row_status != self.row_status)[0][:8], rep.row_status, self.row_status)
        assert rep.first_gate == self.first_gate, (rep.first_gate, self.first_gate)
        assert rep.noncanonical_cells == self.noncanonical_cells
        assert rep.first_noncanonical == self.first_noncanonical
        flags = rep.cell_flags
        assert flags.shape == (self.R, self.n) and set(np.unique(flags)) <= {0, 1}
        flagged = [(int(r), int(c)) for c, r in zip(*np.nonzero(flags))]            # by ascending key
        assert (rep.copy_cells_failed == 0) == (not self.nonconstant)                # (a)
        hit = set()
        for cell in flagged:                                                         # (b)
            assert cell in self.class_of and self.class_of[cell] in self.nonconstant, cell
            hit.add(self.class_of[cell])
        assert hit == set(self.nonconstant)
        assert rep.copy_cells_failed == len(flagged)                                 # (c)
        if flagged:
            cell, partner, values = rep.first_copy
            assert cell == flagged[0]
            assert self.class_of[partner] == self.class_of[cell] and partner != cell
            assert values == (int(self.raw[cell[1], cell[0]]), int(self.raw[partner[1], partner[0]]))
            assert values[0] % P != values[1] % P
        else:
            assert rep.first_copy is None
        assert rep.ok == self.ok
        return flagged


@contextlib.contextmanager
def recorded_build(pkg):
    """The build keywords of every circuit a builder lays out inside the block: builder.build_blob's arguments, recorded in the
    list this yields, as `Model` and `CircuitData.build` take them."""
    builder, seen = sys.modules[pkg.__name__ + ".builder"], []
    real = builder.build_blob

    def record(degree_bits, gates, row_gate, row_constants, copies, num_public_inputs=0, num_wires=234, **kw):
        seen.append(dict(degree_bits=degree_bits, gates=list(gates), row_gate=np.array(row_gate), row_constants=np.array(row_constants),
                         copies=np.array(copies), num_public_inputs=num_public_inputs, num_wires=num_wires, num_routed_wires=80))
        return real(degree_bits, gates, row_gate, row_constants, copies, num_public_inputs=num_public_inputs, num_wires=num_wires, **kw)

    builder.build_blob = record
    try:
        yield seen
    finally:
        builder.build_blob = real


def corrupt(wires, row, col, delta=1):
    w = np.array(wires, dtype=np.uint64, copy=True)
    w[col, row] = (int(w[col, row]) + delta) % P
    return w

