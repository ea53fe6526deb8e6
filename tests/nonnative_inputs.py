"""The circuits of the reference's nonnative gadget tests (plonky2_ecdsa/biguint/gadgets/nonnative.rs:739-908: add, sub, mul, neg,
inv) with fixed values in place of FF::rand(), over both fields the reference instantiates; "virtual" forms whose operands are
seeds, range-checked first as biguint_inputs.div_rem_virtual's are; a chain with the dependency shape of curve_add's slope and
x-coordinate; and edge operands per kind with the values Python expects.  Shared by tests/test_reference_nonnative_tests.py
(oracle), tests/test_witness_plan_nonnative.py (host plan compiler), tests/test_nonnative_host.py (the arithmetic under g++) and
tests/test_gpu_nonnative.py (MI355X).  All circuits have 234 wires (wide_ecc_config, what the reference builds with): a
U32RangeCheckGate row over the eight limbs of a field element needs 136."""
from biguint_inputs import M, digits, set_biguint  # noqa: F401

BASE, SCALAR = "secp256k1_base", "secp256k1_scalar"
FIELDS = (BASE, SCALAR)
FIELD_IDS = {BASE: 0, SCALAR: 1}
ORDER = {BASE: 2**256 - 2**32 - 977, SCALAR: 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141}
KINDS = {"nonnative_add": 2, "nonnative_sub": 3, "nonnative_mul": 4, "nonnative_inv": 5}
OP_CODES = {"nonnative_add": 15, "nonnative_sub": 16, "nonnative_mul": 17, "nonnative_inv": 18}
L = 8
NUM_WIRES = 234
# the "random" field elements (below both orders: their top word is not all ones)
X256 = 0xC6EF372F_E94F82BE_3B9AC9FF_54A0B1D7_9E3779B9_7F4A7C15_F39CC060_5CEDC834
Y256 = 0xA54FF53A_5F1D36F1_510E527F_ADE682D1_9B05688C_2B3E6C1F_1F83D9AB_FB41BD6B
Z256 = 0x3C6EF372_FE94F82B_E3B9AC9F_F54A0B1D_79E3779B_97F4A7C1_5F39CC06_05CEDC83
V256 = 0x72BE5D74_F27B896F_3956C25B_F59F111F_1923F82A_4AF194F9_B5C0FBCF_E9B5DBA5
assert all(v < min(ORDER.values()) for v in (X256, Y256, Z256, V256))


def builder(pkg):
    return pkg.translate.CircuitBuilder(num_wires=NUM_WIRES)


def expected(kind, field, a, b=0):
    """What the generator of `kind` sets for the integers a and b (any size: reduced first), as (first, second)."""
    m = ORDER[field]
    a, b = a % m, b % m
    if kind == "add":
        return (a + b - m, 1) if a + b > m else (a + b, 0)
    if kind in ("sub", "neg"):
        return (a - b, 0) if a >= b else (m + a - b, 1)
    if kind == "mul":
        q, r = divmod(a * b, m)
        return r, q
    inv = pow(a, -1, m)
    return inv, a * inv // m


# -- the reference's five tests: constants in, the result connected to the expected constant ----------------------------
def _binary(pkg, kind, field, x, y, claimed):
    b = builder(pkg)
    z = getattr(b, kind + "_nonnative")(b.constant_nonnative(x, field), b.constant_nonnative(y, field), field)
    b.connect_nonnative(z, b.constant_nonnative(expected(kind, field, x, y)[0] if claimed is None else claimed, field), field)
    return b, {}


def add_case(pkg, field=BASE, claimed=None):
    """nonnative.rs:739-764 test_nonnative_add (the sum wraps: x + y > M for both fields)"""
    return _binary(pkg, "add", field, X256, Y256, claimed)


def sub_case(pkg, field=BASE, claimed=None):
    """nonnative.rs:806-834 test_nonnative_sub: x >= y"""
    return _binary(pkg, "sub", field, X256, Y256, claimed)


def mul_case(pkg, field=BASE, claimed=None):
    """nonnative.rs:836-860 test_nonnative_mul"""
    return _binary(pkg, "mul", field, X256, Y256, claimed)


def neg_case(pkg, field=BASE, claimed=None):
    """nonnative.rs:862-884 test_nonnative_neg"""
    b = builder(pkg)
    z = b.neg_nonnative(b.constant_nonnative(X256, field), field)
    b.connect_nonnative(z, b.constant_nonnative(ORDER[field] - X256 if claimed is None else claimed, field), field)
    return b, {}


def inv_case(pkg, field=BASE, claimed=None):
    """nonnative.rs:886-908 test_nonnative_inv"""
    b = builder(pkg)
    z = b.inv_nonnative(b.constant_nonnative(X256, field), field)
    b.connect_nonnative(z, b.constant_nonnative(pow(X256, -1, ORDER[field]) if claimed is None else claimed, field), field)
    return b, {}


REFERENCE_CASES = [("add", add_case), ("sub", sub_case), ("mul", mul_case), ("neg", neg_case), ("inv", inv_case)]


# -- virtual operands ------------------------------------------------------------------------------------------------------
def _inputs(b, count):
    """A virtual target of `count` limbs, range-checked (13 limbs per U32RangeCheckGate row at most at 234 wires): the first
    cell of a limb's copy class, the cell its seed names, is a gate input (biguint_inputs.div_rem_virtual says why)."""
    t = b.add_virtual_biguint_target(count)
    for i in range(0, count, 13):
        b.range_check_u32(t[i:i + 13])
    return t


def virtual(pkg, kind, field=BASE, la=L, lb=L):
    """One operation over virtual operands of la and lb limbs (inv: la; neg: the operand has lb limbs, `a` none).
    (builder, a limbs, b limbs, the first target's limbs, the second target's limbs)"""
    b = builder(pkg)
    if kind == "inv":
        ta, tb = _inputs(b, la), []
        b.inv_nonnative(ta, field)
    elif kind == "neg":
        ta, tb = [], _inputs(b, lb)
        b.neg_nonnative(tb, field)
    else:
        ta, tb = _inputs(b, la), _inputs(b, lb)
        getattr(b, kind + "_nonnative")(ta, tb, field)
    (ev,) = [e for e in b.events if e.kind in pkg.translate.NONNATIVE_EVENTS]
    a, b_, first, second = ev.groups
    assert list(a) == ta and list(b_) == tb
    return b, ta, tb, list(first), list(second)


def operands(c, x, y=0):
    """The witness of virtual()'s circuit for a = x, b = y."""
    w = {}
    set_biguint(w, c[1], x), set_biguint(w, c[2], y)
    return w


# -- the chain: curve_add's slope and x-coordinate -----------------------------------------------------------------------
def chain(pkg, field=BASE):
    """u = y2 - y1, v = x2 - x1, s = u * inv(v), x3 = s * s - x1 - x2: seven generators, the six from v on each feeding the next.
    (builder, [x1, y1, x2, y2] limb lists, x3 limbs)"""
    b = builder(pkg)
    x1, y1, x2, y2 = (_inputs(b, L) for _ in range(4))
    u = b.sub_nonnative(y2, y1, field)
    v = b.sub_nonnative(x2, x1, field)
    s = b.mul_nonnative(u, b.inv_nonnative(v, field), field)
    x3 = b.sub_nonnative(b.sub_nonnative(b.mul_nonnative(s, s, field), x1, field), x2, field)
    return b, [x1, y1, x2, y2], x3


CHAIN_KINDS = ["nonnative_sub", "nonnative_sub", "nonnative_inv", "nonnative_mul", "nonnative_mul", "nonnative_sub", "nonnative_sub"]


def chain_operands(c, x1, y1, x2, y2):
    w = {}
    for t, v in zip(c[1], (x1, y1, x2, y2)):
        set_biguint(w, t, v)
    return w


def chain_x3(field, x1, y1, x2, y2):
    m = ORDER[field]
    s = (y2 - y1) * pow(x2 - x1, -1, m) % m
    return (s * s - x1 - x2) % m


# -- edge operands: (name, kind, la, lb, a(field), b(field)); what Python expects comes from expected() -------------------------
def _zero_top_inverse(field):
    """A value whose inverse has a zero top digit: the inverse of a seven-digit number."""
    m = ORDER[field]
    inv = 0x1F83D9AB_FB41BD6B_9B05688C_2B3E6C1F_510E527F_ADE682D1_5F1D36F1      # 7 digits
    return pow(inv, -1, m)


EDGES = [
    ("add_below_m", "add", L, L, lambda f: X256 >> 1, lambda f: Y256 >> 1),
    ("add_equals_m", "add", L, L, lambda f: X256, lambda f: ORDER[f] - X256),                 # sum = M itself, overflow 0
    ("add_m_plus_one", "add", L, L, lambda f: X256 + 1, lambda f: ORDER[f] - X256),
    ("add_both_m_minus_one", "add", L, L, lambda f: ORDER[f] - 1, lambda f: ORDER[f] - 1),
    ("add_one_limb_b", "add", L, 1, lambda f: X256, lambda f: 1),                              # bool_to_nonnative's shape
    ("sub_equal", "sub", L, L, lambda f: X256, lambda f: X256),
    ("sub_below_by_one", "sub", L, L, lambda f: Y256, lambda f: Y256 + 1),
    ("sub_neg_shape", "neg", 0, L, lambda f: 0, lambda f: X256),                               # la = 0
    ("sub_b_zero", "sub", L, L, lambda f: X256, lambda f: 0),
    ("mul_a_zero", "mul", L, L, lambda f: 0, lambda f: Y256),
    ("mul_both_m_minus_one", "mul", L, L, lambda f: ORDER[f] - 1, lambda f: ORDER[f] - 1),
    ("mul_below_m", "mul", L, L, lambda f: X256 >> 130, lambda f: Y256 >> 130),
    ("mul_four_by_four", "mul", 4, 4, lambda f: X256 >> 128, lambda f: Y256 >> 128),           # the overflow has no limbs
    ("mul_all_ones_below_m", "mul", L, L, lambda f: 2**224 - 1, lambda f: ORDER[f] - 2**224),  # limbs of 2^32 - 1 below the modulus
    ("inv_one", "inv", L, 0, lambda f: 1, lambda f: 0),
    ("inv_two", "inv", L, 0, lambda f: 2, lambda f: 0),
    ("inv_m_minus_one", "inv", L, 0, lambda f: ORDER[f] - 1, lambda f: 0),
    ("inv_zero_top_digit", "inv", L, 0, _zero_top_inverse, lambda f: 0),
]
for _f in FIELDS:
    assert expected("add", _f, X256, ORDER[_f] - X256) == (ORDER[_f], 0)
    assert expected("inv", _f, _zero_top_inverse(_f))[0] >> 224 == 0
    assert (2**224 - 1) < ORDER[_f] and ORDER[_f] - 2**224 < ORDER[_f]
