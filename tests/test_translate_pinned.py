"""The translator's outputs, pinned: SHA-256 digests of the blob, the wire matrix, the seed cells, the seed values, the generator
list and the public-input values of a small corpus of circuits, against tests/golden/translate_pinned.json.  The corpus goes
through public methods only (`translate_circuit`, `build`, `witness_seeds`, `witness_generators`, `public_inputs`; on a bare
CircuitBuilder the gadget methods, `build`, `seed_cells`, `seed_values`, `generators`), so the same file records and checks:
    python tests/test_translate_pinned.py        # rewrites the JSON from the tree it runs in
The JSON in the tree was recorded so at commit 673fc51, before the translator was split into builder.py and the gadget modules:
a change of the translator's structure leaves every digest as it is.  CPU only."""
import hashlib
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import biguint_inputs as bui  # noqa: E402
import memory_ops_inputs as moi  # noqa: E402
import nonnative_inputs as nni  # noqa: E402

PINNED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "translate_pinned.json")
KEYS = ("blob", "wires", "seed_cells", "seed_values", "generators", "public_inputs")
SHA256_IV = [0x6a09e667, 0xbb67ae85, 0x3c6ef372, 0xa54ff53a, 0x510e527f, 0x9b05688c, 0x1f83d9ab, 0x5be0cd19]


def _digest(x):
    data = x.tobytes() if hasattr(x, "tobytes") else json.dumps(x, default=int).encode()
    return hashlib.sha256(data).hexdigest()


def _digests(*six):
    return {k: _digest(v) for k, v in zip(KEYS, six)}


def program(pkg, ops, witness, public=(), private=(), num_wires=234):
    cb = pkg.translate.CircuitBuilderFromAcirToPlonky2(num_wires=num_wires)
    cb.translate_circuit(ops, public_parameters=public, private_parameters=private)
    blob, wires = cb.build(witness)
    cells, values = cb.witness_seeds(witness)
    return _digests(blob, wires, cells, values, cb.witness_generators(), cb.public_inputs())


def bare(b, witness):
    blob, wires = b.build(witness)
    return _digests(blob, wires, b.seed_cells(), b.seed_values(witness), b.generators(), b.public_input_values)


# -- the corpus: name -> function of pkg that returns the six digests -------------------------------------------------------
CORPUS = {}


def case(name):
    def add(fn):
        assert name not in CORPUS
        CORPUS[name] = fn
        return fn
    return add


@case("sha256_compression_234")
def _sha256(pkg):
    wit = dict(enumerate([1 << 31] + [0] * 15 + SHA256_IV))
    return program(pkg, [("sha256_compression", list(range(16)), list(range(16, 24)), list(range(24, 32)))], wit)


for _bits in (8, 32):
    @case("range_and_xor_%d" % _bits)
    def _bitwise(pkg, bits=_bits):
        ops = [("range", 0, bits), ("range", 1, bits), ("and", 0, 1, 2, bits), ("xor", 0, 1, 3, bits)]
        return program(pkg, ops, {0: 0xF0F0F0F0 >> (32 - bits), 1: 0xFF00FF35 >> (32 - bits)}, private=[0, 1])

# a block of 8: one write, then the written position and another are read
LENGTH_8 = dict(ops=[moi.init(0, list(range(8))), moi.write(0, 8, 9), moi.read(0, 10, 11), moi.read(0, 12, 13)],
                public=list(range(11)) + [12])
MEMORY = [(name, prog, wit) for name, prog, wit, _ in moi.CASES]
MEMORY.append(("block_of_length_8", LENGTH_8, {**{i: 50 + i for i in range(8)}, 8: 6, 9: 77, 10: 6, 12: 7}))
for _name, _prog, _wit in MEMORY:
    for _nw in (234, 135):
        @case("memory_%s_%d" % (_name, _nw))
        def _memory(pkg, prog=_prog, wit=_wit, nw=_nw):
            return program(pkg, prog["ops"], wit, public=prog["public"], num_wires=nw)

# w11 = w0 + ... + w10, the eleven summands public (two PoseidonGate rows) or not (none)
SUM_OPS = [("assert_zero", [], [(1, i) for i in range(11)] + [(moi.P - 1, 11)], 0)]
SUM_WITNESS = {**{i: 1000 + 7 * i for i in range(11)}, 11: sum(1000 + 7 * i for i in range(11))}


@case("public_parameters_11")
def _public_11(pkg):
    return program(pkg, SUM_OPS, SUM_WITNESS, public=list(range(11)), private=[11])


@case("public_parameters_none")
def _public_none(pkg):
    return program(pkg, SUM_OPS, SUM_WITNESS, private=list(range(12)))


def _add_many(pkg, count, num_wires):
    b, w = bui.builder(pkg, num_wires), {}
    ts = b.add_virtual_u32_targets(count)
    b.range_check_u32(ts)
    b.add_many_u32(ts)
    for i, t in enumerate(ts):
        w[t] = 0xFFFFFFFF - 3 * i
    return b, w


def _div_rem(pkg, la, lb, num_wires, then_equal=False):
    c = bui.div_rem_virtual(pkg, la, lb, num_wires)
    if then_equal:
        c[0].is_equal(c[3][0], c[4][0])
    return c[0], bui.operands(c, bui.X128 >> (32 * (4 - la)), bui.Y128 >> (32 * (4 - lb)))


for _nw in (135, 234):
    for _name, _fn in bui.REFERENCE_CASES[:4]:
        @case("biguint_%s_%d" % (_name, _nw))
        def _biguint(pkg, fn=_fn, nw=_nw):
            return bare(*fn(pkg, num_wires=nw))

    for _count in (3, 4):
        @case("add_many_u32_%d_%d" % (_count, _nw))
        def _add_many_case(pkg, count=_count, nw=_nw):
            return bare(*_add_many(pkg, count, nw))

    for _la, _lb in ((4, 2), (1, 1), (1, 3)):
        @case("div_rem_%d_%d_%d" % (_la, _lb, _nw))
        def _div_rem_case(pkg, la=_la, lb=_lb, nw=_nw):
            return bare(*_div_rem(pkg, la, lb, nw))

    @case("div_rem_then_is_equal_%d" % _nw)
    def _div_rem_equal(pkg, nw=_nw):
        return bare(*_div_rem(pkg, 4, 2, nw, then_equal=True))


def _conditional_neg(pkg, field):
    b = nni.builder(pkg)
    x = nni._inputs(b, nni.L)
    flag = b.add_virtual_bool_target_safe()
    b.nonnative_conditional_neg(x, flag, field)
    w = {flag: 1}
    nni.set_biguint(w, x, nni.X256)
    return b, w


def _reduce(pkg, field):
    b = nni.builder(pkg)
    x = nni._inputs(b, 10)
    b.reduce_nonnative(x, field)
    w = {}
    nni.set_biguint(w, x, (nni.X256 << 64) + nni.Y256)
    return b, w


for _field in nni.FIELDS:
    for _kind, _la, _lb in (("add", 8, 8), ("sub", 8, 8), ("mul", 8, 8), ("inv", 8, 0), ("neg", 0, 8), ("mul", 4, 4)):
        @case("nonnative_%s_%d_%d_%s" % (_kind, _la, _lb, _field))
        def _nonnative(pkg, kind=_kind, la=_la, lb=_lb, field=_field):
            c = nni.virtual(pkg, kind, field, la, lb)
            return bare(c[0], nni.operands(c, nni.X256 >> (32 * (8 - la)) if la else 0, nni.Y256 >> (32 * (8 - lb)) if lb else 0))

    @case("nonnative_conditional_neg_%s" % _field)
    def _nn_conditional_neg(pkg, field=_field):
        return bare(*_conditional_neg(pkg, field))

    @case("reduce_nonnative_%s" % _field)
    def _nn_reduce(pkg, field=_field):
        return bare(*_reduce(pkg, field))

    @case("nonnative_chain_%s" % _field)
    def _nn_chain(pkg, field=_field):
        c = nni.chain(pkg, field)
        return bare(c[0], nni.chain_operands(c, nni.X256, nni.Y256, nni.Z256, nni.V256))


@pytest.fixture(scope="module")
def pinned():
    with open(PINNED) as f:
        return json.load(f)


def test_corpus_is_the_recorded_one(pinned):
    assert sorted(pinned) == sorted(CORPUS)


@pytest.mark.parametrize("name", list(CORPUS))
def test_pinned(pkg, pinned, name):
    got = CORPUS[name](pkg)
    assert set(got) == set(KEYS)
    for k in KEYS:
        assert got[k] == pinned[name][k], "%s: the %s differ from the recorded ones" % (name, k)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import __graft_entry__ as entry
    entry.build()
    package = entry.load_package()
    with open(PINNED, "w") as f:
        json.dump({name: fn(package) for name, fn in CORPUS.items()}, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded %d circuits in %s" % (len(CORPUS), PINNED))
