"""The circuits of the reference's curve gadget tests (plonky2_ecdsa/curve/gadgets/curve.rs:330-545: the live test_curve_mul and
the ones it keeps commented) with fixed values, the circuits the device tests run (virtual operands, range-checked first as
nonnative_inputs.virtual's are), the scalars of the GLV decomposition tests, and an integer model: plain functions on Python
integers that follow the gadgets' formulas and know nothing of the builder.  Shared by tests/test_reference_curve_tests.py
(oracle), tests/test_glv_host.py (the arithmetic under g++), tests/test_witness_plan_glv.py (host plan compiler),
tests/test_translate_ecdsa.py and tests/test_gpu_curve.py (MI355X).  All circuits have 234 wires."""
import json
import os
import random

from nonnative_inputs import BASE, L, NUM_WIRES, ORDER, SCALAR, _inputs, builder, digits, set_biguint  # noqa: F401

GOLDILOCKS = 0xFFFFFFFF00000001
P, N = ORDER[BASE], ORDER[SCALAR]
HALF = (N - 1) // 2
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
GX = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
GY = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8
G = (GX, GY)
KIND, OP_CODE = 8, 19                   # P2GPU_GEN_GLV_DECOMPOSE, OP_GLV_DECOMPOSE


# -- the integer model ---------------------------------------------------------------------------------------------------------
GLV_BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
GLV_S = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
A1 = B2 = 0x3086D221A7D46BCDE86C90E49284EB15
MINUS_B1 = 0xE4437ED6010E88286F547FA90ABFE4C3
A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
RANDO = (0xA86C70FE28EB2CB4E881AA81971AE5121389F53E8B82771E5435099CAAACA00F, 0x3C20A74F2CC59D7DF8BE94B58EE35F088885C02B6E16821DABDD5C2B0901B91B)
TO_ADD = (0x04F07480028E1A4379E40FAC7D38B237DCB21FC25AA8287F3BC10079ECB2821D, 0xC3144A41D7A799C9EB6EE728CF791E371210CD8AA94214FD31362398F775F69B)


def on_curve(pt):
    return (pt[1] * pt[1] - pt[0] ** 3 - 7) % P == 0


def neg(pt):
    return pt[0], (P - pt[1]) % P


def add(p1, p2):
    """curve_add's formula: the slope through two points of different x (the inverse of zero has no value)"""
    (x1, y1), (x2, y2) = p1, p2
    if (x2 - x1) % P == 0:
        raise ZeroDivisionError("curve_add of two points with one x")
    s = (y2 - y1) * pow(x2 - x1, -1, P) % P
    x3 = (s * s - x1 - x2) % P
    return x3, (s * (x1 - x3) - y1) % P


def double(pt):
    x, y = pt
    lam = 3 * x * x * pow(2 * y, -1, P) % P
    x3 = (lam * lam - 2 * x) % P
    return x3, (lam * (x - x3) - y) % P


def mul(k, pt):
    """k * pt by double-and-add over complete arithmetic (None is the zero point): the yardstick for msm and glv"""
    acc, cur = None, pt
    while k:
        if k & 1:
            acc = cur if acc is None else (double(acc) if acc == cur else (None if acc == neg(cur) else add(acc, cur)))
        cur = double(cur)
        k >>= 1
    return acc


def msm(p, q, n, m, limbs):
    """curve_msm_circuit's window walk: n p + m q for scalars of `limbs` 32-bit limbs, two bits per window from the top, the
    table i p + j q built from RANDO as the gadget builds it, the fixed correction TO_ADD at the end (which is minus the
    multiple of RANDO the walk accumulates over 4 limbs = 64 windows: for other limb counts the result keeps an offset)."""
    table = [p] * 16
    cur_p = cur_q = RANDO
    for i in range(4):
        table[i], table[4 * i] = cur_p, cur_q
        cur_p, cur_q = add(cur_p, p), add(cur_q, q)
    for i in range(1, 4):
        table[i], table[4 * i] = add(table[i], neg(RANDO)), add(table[4 * i], neg(RANDO))
    for i in range(1, 4):
        for j in range(1, 4):
            table[i + 4 * j] = add(table[i], table[4 * j])
    result = RANDO
    for w in reversed(range(16 * limbs)):
        result = double(double(result))
        index = ((n >> (2 * w)) & 3) + 4 * ((m >> (2 * w)) & 3)
        if index:
            result = add(result, table[index])
    return add(result, TO_ADD)


def decompose(k):
    """decompose_secp256k1_scalar on an integer k in [0, N): (|k1|, |k2|, k1 < 0, k2 < 0); the rounding by exact halves"""
    def rounded(a):
        q, r = divmod(a, N)
        return q + (1 if 2 * r > N else 0)
    c1, c2 = rounded(B2 * k), rounded(MINUS_B1 * k)
    k1, k2 = (k - c1 * A1 - c2 * A2) % N, (c1 * MINUS_B1 - c2 * B2) % N
    n1, n2 = k1 > HALF, k2 > HALF
    return (N - k1 if n1 else k1), (N - k2 if n2 else k2), n1, n2


def glv(pt, k):
    """glv_mul: k1 (+-pt) + k2 (+-(beta x, y)) through the window walk with four-limb scalars"""
    k1, k2, n1, n2 = decompose(k % N)
    sp = (GLV_BETA * pt[0] % P, pt[1])
    return msm(neg(pt) if n1 else pt, neg(sp) if n2 else sp, k1, k2, 4)


def fold(limbs):
    return sum(v << (32 * i) for i, v in enumerate(limbs))


def ecdsa_reading(b):
    """A 32-byte string as the reference's translator reads it: limb i = b[4i] + 2^8 b[4i+1] + 2^16 b[4i+2] + 2^24 b[4i+3], limb 0
    the least significant -- the little-endian integer of the string."""
    return int.from_bytes(bytes(b), "little")


def ecdsa_model(pkx, pky, signature, hashed_message, reading=ecdsa_reading):
    """The translated circuit on integers: R = (h / s) G + (r / s) Q through glv(), then (r, R, r <= R.x).  The formulas never
    ask whether Q lies on the curve, and neither does this."""
    q = (reading(pkx), reading(pky))
    r, s, h = reading(signature[:32]), reading(signature[32:]), reading(hashed_message)
    assert max(r, s, h) < N and max(q) < P, "a reading of the order or above: the nonnative constraints would not hold"
    s1 = pow(s, -1, N)
    big_r = add(glv(G, h * s1 % N), glv(q, r * s1 % N))
    return r, big_r, int(r <= big_r[0])


PLAN_KINDS = {"equality": 0, "biguint_divrem": 1, "nonnative_add": 2, "nonnative_sub": 3, "nonnative_mul": 4, "nonnative_inv": 5, "glv_decompose": KIND}
FIELD_IDS = {BASE: 0, SCALAR: 1}


def records(generators):
    """builder.generators() -> (p2gpu_generator_v records [kind word, shape[4]], flat (row, col) list), as numpy would take them"""
    recs, cells = [], []
    for gen in generators:
        groups = [[c] for c in gen[1]] if gen[0] == "equality" else [list(grp) for grp in gen[1]]
        recs.append([PLAN_KINDS[gen[0]] | (FIELD_IDS[gen[2]] << 8 if len(gen) > 2 else 0)] + [len(grp) for grp in groups])
        cells += [tuple(c) for grp in groups for c in grp]
    return recs, cells


# -- fixtures: recorded values of the reference -----------------------------------------------------------------------------------
def curve_mul_vector():
    """the reference's test_curve_mul (curve.rs:482-518): (scalar, expected x, expected y)"""
    with open(os.path.join(GOLDEN, "reference", "curve_mul.json")) as f:
        v = json.load(f)
    return int(v["scalar"], 16), int(v["x"], 16), int(v["y"], 16)


def prover_toml_bytes():
    """the 160 input bytes of the reference's ecdsa_secp256k1/Prover.toml: {name: [bytes]}"""
    with open(os.path.join(GOLDEN, "reference", "ecdsa_secp256k1_prover.json")) as f:
        return {k: list(v) for k, v in json.load(f).items()}


# -- the scalars of the decomposition tests ----------------------------------------------------------------------------------------
def _sign_pairs():
    """one scalar per sign pair, by a seeded search: {(k1_neg, k2_neg): k}"""
    rng, out = random.Random(20261019), {}
    while len(out) < 4:
        k = rng.randrange(N)
        out.setdefault(decompose(k)[2:], k)
    return out


SIGN_PAIRS = _sign_pairs()
assert {s: decompose(k)[2:] for s, k in SIGN_PAIRS.items()} == {s: s for s in [(False, False), (False, True), (True, False), (True, True)]}
# the four rounding edges: B2 k = t and MINUS_B1 k = t (mod N) for t either side of N / 2
ROUNDING_EDGES = [t * pow(c, -1, N) % N for c in (B2, MINUS_B1) for t in (HALF, HALF + 1)]
for _c, _ks in ((B2, ROUNDING_EDGES[:2]), (MINUS_B1, ROUNDING_EDGES[2:])):
    assert [2 * (_c * _k % N) - N for _k in _ks] == [-1, 1]          # the remainders: half a unit below and above the tie
SCALARS = [0, 1, N - 1, N - 5, GLV_S, N - GLV_S] + ROUNDING_EDGES + [SIGN_PAIRS[s] for s in sorted(SIGN_PAIRS)]
# limb lists that exercise fold and reduce: sixteen limbs of an integer >= N, and eight limbs one of which is >= 2^32
LIMB_LISTS = [digits((N + 12345) << 200 | 0xDEADBEEF, 16), [0xFFFFFFFF00000000, 7, (1 << 32) + 5, 0, 0xFFFFFFFF, 1 << 40, 3, 0x7FFFFFFF]]
assert fold(LIMB_LISTS[0]) >= N and any(v >> 32 for v in LIMB_LISTS[1])
assert max(max(decompose(k % N)[:2]).bit_length() for k in SCALARS + [fold(x) for x in LIMB_LISTS]) == 128
for _k in SCALARS:
    _k1, _k2, _n1, _n2 = decompose(_k)
    assert ((-_k1 if _n1 else _k1) + GLV_S * (-_k2 if _n2 else _k2)) % N == _k and _k1 < 1 << 128 and _k2 < 1 << 128


# -- the reference's tests ------------------------------------------------------------------------------------------------------
def point_is_valid(pkg, bad=False):
    """curve.rs:330-380 test_curve_point_is_valid / _is_not_valid (G.y + 1)"""
    b = builder(pkg)
    if bad:
        b.curve_assert_valid(b.constant_affine_point(GX, GY + 1))
    else:
        g = b.curve_generator_constant()
        b.curve_assert_valid(g)
        b.curve_assert_valid(b.curve_neg(g))
    return b, {}


def double_case(pkg):
    """curve.rs:382-417 test_curve_double: 2 G and 2 (-G)"""
    b = builder(pkg)
    g = b.curve_generator_constant()
    neg_g = b.curve_neg(g)
    e1, e2 = b.constant_affine_point(*double(G)), b.constant_affine_point(*double(neg(G)))
    b.curve_assert_valid(e1)
    b.curve_assert_valid(e2)
    a1, a2 = b.curve_double(g), b.curve_double(neg_g)
    b.curve_assert_valid(a1)
    b.curve_assert_valid(a2)
    b.connect_affine_point(e1, a1)
    b.connect_affine_point(e2, a2)
    return b, {}


def add_case(pkg):
    """curve.rs:419-447 test_curve_add: G + 2 G"""
    b = builder(pkg)
    expected = b.constant_affine_point(*add(G, double(G)))
    b.curve_assert_valid(expected)
    g = b.curve_generator_constant()
    actual = b.curve_add(g, b.curve_double(g))
    b.curve_assert_valid(actual)
    b.connect_affine_point(expected, actual)
    return b, {}


def conditional_add_case(pkg):
    """curve.rs:449-479 test_curve_conditional_add: with true and with false"""
    b = builder(pkg)
    expected = b.constant_affine_point(*add(G, double(G)))
    g = b.curve_generator_constant()
    two_g = b.curve_double(g)
    b.connect_affine_point(expected, b.curve_conditional_add(g, two_g, b.constant_bool(True)))
    b.connect_affine_point(g, b.curve_conditional_add(g, two_g, b.constant_bool(False)))
    return b, {}


MUL2_POINT = mul(0xC0FFEE, G)


def scalar_mul_two_case(pkg):
    """curve.rs:520-545 test_curve_random, the point fixed: curve_scalar_mul(P, 2) == curve_double(P)"""
    b = builder(pkg)
    pt = b.constant_affine_point(*MUL2_POINT)
    b.connect_affine_point(b.curve_double(pt), b.curve_scalar_mul(pt, b.constant_nonnative(2, SCALAR)))
    return b, {}


def glv_mul_case(pkg):
    """curve.rs:482-518 test_curve_mul: glv_mul(G, k) connected to the recorded point; the scalar is virtual (and, here,
    range-checked: its limbs are the seeds of the device witness).  (builder, scalar limbs)"""
    _, x, y = curve_mul_vector()
    b = builder(pkg)
    g = b.constant_affine_point(GX, GY)
    scalar = _inputs(b, L)
    b.connect_affine_point(b.glv_mul(g, scalar), b.constant_affine_point(x, y))
    return b, scalar


# -- circuits with virtual operands, for the device witness -----------------------------------------------------------------------
def decomposition(pkg, lk=L):
    """decompose_secp256k1_scalar on a virtual, range-checked scalar of lk limbs.  (builder, k limbs, k1, k2, k1_neg, k2_neg)"""
    b = builder(pkg)
    k = _inputs(b, lk)
    return (b, k) + tuple(b.decompose_secp256k1_scalar(k))


def generator_only(pkg, lk):
    """The GLV decomposition generator without the gadget's check, over lk limbs that nothing range-checks (each is squared, to
    lie in a gate row): what fold and reduce do with sixteen limbs and with limbs of 2^32 and above.  Same tuple as above."""
    b = builder(pkg)
    k = b.add_virtual_biguint_target(lk)
    for t in k:
        b.mul(t, t)
    k1, k2 = b.add_virtual_biguint_target(4), b.add_virtual_biguint_target(4)
    k1_neg, k2_neg = b.add_virtual_bool_target_safe(), b.add_virtual_bool_target_safe()
    b._listed_generator("glvdec", k, (), k1 + k2, (k1_neg, k2_neg))
    b.range_check_u32(k1 + k2)
    return b, k, k1, k2, k1_neg, k2_neg


def scalar_witness(c, limbs):
    return {t: v for t, v in zip(c[1], limbs)}


def _point(b):
    return _inputs(b, L), _inputs(b, L)


def set_point(w, target, pt):
    set_biguint(w, target[0], pt[0]), set_biguint(w, target[1], pt[1])


def point_of(b, target):
    return fold([b.value_of(t) for t in target[0]]), fold([b.value_of(t) for t in target[1]])


def curve_op(pkg, op):
    """One curve operation over virtual points ("add", "double", "conditional_add", "assert_valid").
    (builder, [point targets], bit target or None, result point or None)"""
    b = builder(pkg)
    if op == "add":
        pts = [_point(b), _point(b)]
        return b, pts, None, b.curve_add(*pts)
    if op == "double":
        pts = [_point(b)]
        return b, pts, None, b.curve_double(pts[0])
    if op == "conditional_add":
        pts = [_point(b), _point(b)]
        bit = b.add_virtual_bool_target_safe()
        return b, pts, bit, b.curve_conditional_add(pts[0], pts[1], bit)
    assert op == "assert_valid"
    pts = [_point(b)]
    b.curve_assert_valid(pts[0])
    return b, pts, None, None


def curve_op_witness(c, points, bit=None):
    w = {}
    for t, pt in zip(c[1], points):
        set_point(w, t, pt)
    if c[2] is not None:
        w[c[2]] = int(bit)
    return w


TABLE = [mul(3 + 2 * i, G) for i in range(16)]        # sixteen points for random_access_curve_points


def random_access(pkg):
    """random_access_curve_points over sixteen constant points, the index virtual (and bounded by a four-bit split).
    (builder, index target, result point)"""
    b = builder(pkg)
    index = b.add_virtual_target()
    b.split_le(index, 4)
    return b, index, b.random_access_curve_points(index, [b.constant_affine_point(*pt) for pt in TABLE])


ECDSA_OUTPUT = 160                      # the witnesses of ecdsa_program(): hashed_message 0 .. 31, pub_key_x, pub_key_y, signature, then the output


def ecdsa_program():
    """The reference's test program (noir_circuits_for_testing/ecdsa_secp256k1/src/main.nr) as the circuit nargo would compile it
    to: one EcdsaSecp256k1 call over the 160 byte parameters and the `assert` on its output.  (circuit dict for
    acir.serialize_program, {witness: value} of Prover.toml without the output)"""
    w = list(range(160))
    fi = [(i, 8) for i in w]
    call = {"name": "EcdsaSecp256k1", "public_key_x": fi[32:64], "public_key_y": fi[64:96], "signature": fi[96:160], "hashed_message": fi[0:32],
            "output": ECDSA_OUTPUT}
    check = {"mul_terms": [], "linear_combinations": [(1, ECDSA_OUTPUT)], "q_c": GOLDILOCKS - 1}
    circuit = {"current_witness_index": ECDSA_OUTPUT, "opcodes": [("BlackBoxFuncCall", call), ("AssertZero", check)], "private_parameters": w}
    v = prover_toml_bytes()
    return circuit, dict(enumerate(v["hashed_message"] + v["pub_key_x"] + v["pub_key_y"] + v["signature"]))


MSM_P, MSM_Q = mul(5, G), mul(11, G)
MSM_SCALARS = [(0x2D, 0), (0, 0xC0000001), (0xFFFFFFFF, 0x1B)]


def msm_one_limb(pkg):
    """curve_msm_circuit on two constant points with one-limb virtual scalars (sixteen windows).  (builder, n, m, result)"""
    b = builder(pkg)
    n, m = _inputs(b, 1), _inputs(b, 1)
    return b, n, m, b.curve_msm_circuit(b.constant_affine_point(*MSM_P), b.constant_affine_point(*MSM_Q), n, m)
