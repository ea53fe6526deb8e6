"""The circuits of the reference's biguint / u32 gadget tests (plonky2_ecdsa/biguint/biguint.rs:374-521, gadgets/arithmetic_u32.rs
:363-394, gadgets/multiple_comparison.rs:93-151) with fixed values in place of OsRng, and the div-rem shapes added beyond them;
shared by tests/test_reference_biguint_tests.py (oracle), tests/test_witness_plan_divrem.py (host plan compiler) and
tests/test_gpu_biguint.py (MI355X).  Every case is (builder, witness {target: value}); expected values are Python integers."""
M = 0xFFFFFFFF
X128 = 0xF3A1_9C04_5D2E_77B1_0C3F_E2A9_8B64_D015      # the "random" 128-bit operands
Y128 = 0x8E5B_21F7_A0C3_4D96_E718_3B5A_F2C4_6D09
SECP256K1_P = 2**256 - 2**32 - 977                    # the base-field prime `nonnative` reduces by


def digits(v, count=None):
    """`to_u32_digits` (zero has none), or exactly `count` 32-bit digits."""
    out = []
    while v:
        out.append(v & M)
        v >>= 32
    if count is not None:
        assert len(out) <= count
        out += [0] * (count - len(out))
    return out


def set_biguint(witness, target, value):
    """witness.set_biguint_target (biguint.rs:291-298)"""
    for t, v in zip(target, digits(value, len(target))):
        witness[t] = v


def builder(pkg, num_wires=135):
    return pkg.translate.CircuitBuilder(num_wires=num_wires)


def add_case(pkg, x=X128, y=Y128, claimed=None, num_wires=135):
    """biguint.rs:374-402 test_biguint_add: virtual x, y and expected_z, all assigned."""
    b, w = builder(pkg, num_wires), {}
    z = x + y if claimed is None else claimed
    tx, ty = b.add_virtual_biguint_target(len(digits(x))), b.add_virtual_biguint_target(len(digits(y)))
    tz = b.add_biguint(tx, ty)
    te = b.add_virtual_biguint_target(len(digits(z)))
    b.connect_biguint(tz, te)
    set_biguint(w, tx, x), set_biguint(w, ty, y), set_biguint(w, te, z)
    return b, w


def sub_case(pkg, x=X128, y=Y128, claimed=None, num_wires=135):
    """biguint.rs:404-432 test_biguint_sub: constants, x >= y."""
    b = builder(pkg, num_wires)
    if y > x:
        x, y = y, x
    z = b.sub_biguint(b.constant_biguint(x), b.constant_biguint(y))
    b.connect_biguint(z, b.constant_biguint(x - y if claimed is None else claimed))
    return b, {}


def mul_case(pkg, x=X128, y=Y128, claimed=None, num_wires=135):
    """biguint.rs:434-462 test_biguint_mul: virtual x, y and expected_z, all assigned."""
    b, w = builder(pkg, num_wires), {}
    z = x * y if claimed is None else claimed
    tx, ty = b.add_virtual_biguint_target(len(digits(x))), b.add_virtual_biguint_target(len(digits(y)))
    tz = b.mul_biguint(tx, ty)
    te = b.add_virtual_biguint_target(len(digits(z)))
    b.connect_biguint(tz, te)
    set_biguint(w, tx, x), set_biguint(w, ty, y), set_biguint(w, te, z)
    return b, w


def cmp_case(pkg, x=X128, y=Y128, claimed=None, num_wires=135):
    """biguint.rs:464-488 test_biguint_cmp: constants."""
    b = builder(pkg, num_wires)
    cmp = b.cmp_biguint(b.constant_biguint(x), b.constant_biguint(y))
    b.connect(cmp, b.constant_bool((x <= y) if claimed is None else claimed))
    return b, {}


def div_rem_case(pkg, x=X128, y=Y128, claimed=None, num_wires=135):
    """biguint.rs:490-521 test_biguint_div_rem: constants, x >= y; div and rem connected to the expected constants."""
    b = builder(pkg, num_wires)
    if y > x:
        x, y = y, x
    q, r = divmod(x, y) if claimed is None else claimed
    div, rem = b.div_rem_biguint(b.constant_biguint(x), b.constant_biguint(y))
    b.connect_biguint(div, b.constant_biguint(q))
    b.connect_biguint(rem, b.constant_biguint(r))
    return b, {}


def div_rem_virtual(pkg, la, lb, num_wires=135):
    """div_rem_biguint over virtual operands of la and lb limbs, the operands the witness's choice, range-checked first as a
    caller's inputs are (seven limbs per U32RangeCheckGate row at most: 17 wires each).  So the first cell of an operand
    limb's copy class -- the cell its seed names -- is a gate INPUT: the U32AddMany result that div_rem_biguint connects `a`
    to afterwards compares with the seed's value in the level walk, it does not share a writer bit with it.
    (builder, a limbs, b limbs, div limbs, rem limbs)"""
    b = builder(pkg, num_wires)
    ta, tb = b.add_virtual_biguint_target(la), b.add_virtual_biguint_target(lb)
    for t in (ta, tb):
        for i in range(0, len(t), 7):
            b.range_check_u32(t[i:i + 7])
    div, rem = b.div_rem_biguint(ta, tb)
    return b, ta, tb, div, rem


def operands(b_ta_tb, x, y):
    """The witness of div_rem_virtual's circuit for a = x, b = y."""
    _, ta, tb = b_ta_tb[:3]
    w = {}
    set_biguint(w, ta, x), set_biguint(w, tb, y)
    return w


def add_many_case(pkg, claimed=None, num_wires=135):
    """arithmetic_u32.rs:363-394 test_add_many_u32s: fifteen constant addends through add_u32s_with_carry."""
    b = builder(pkg, num_wires)
    xs = [(0x9E3779B9 * (i + 1) ^ 0x5BD1E995 * (i + 7)) & M for i in range(15)]
    total = sum(xs) if claimed is None else claimed
    low, high = b.add_u32s_with_carry([b.constant_u32(x) for x in xs], b.zero_u32())
    b.connect_u32(low, b.constant_u32(total & M))
    b.connect_u32(high, b.constant_u32(total >> 32))
    return b, {}


def list_le_case(pkg, size, num_bits, claimed=None, num_wires=135):
    """multiple_comparison.rs:93-140 test_list_le: two lists of `size` constants below 2^num_bits."""
    b = builder(pkg, num_wires)
    l1 = [(0x9E3779B97F4A7C15 * (i + 3)) % (1 << num_bits) for i in range(size)]
    l2 = [(0xC2B2AE3D27D4EB4F * (i + 5)) % (1 << num_bits) for i in range(size)]
    l2[-1] = l1[-1]                                       # (the top limbs equal: the comparison goes on below them)
    va = sum(v << (64 * i) for i, v in enumerate(l1))
    vb = sum(v << (64 * i) for i, v in enumerate(l2))
    res = b.list_le([b.constant(v) for v in l1], [b.constant(v) for v in l2], num_bits)
    b.connect(res, b.constant_bool((va <= vb) if claimed is None else not (va <= vb)))      # (claimed: the wrong answer)
    return b, {}


# the reference's five biguint tests
REFERENCE_CASES = [("add", add_case), ("sub", sub_case), ("mul", mul_case), ("cmp", cmp_case), ("div_rem", div_rem_case)]

# div-rem operands beyond the reference: (name, la, lb, a, b)
ADD_BACK_A, ADD_BACK_B = 3 + (0x80000000 << 64), 1 + (0x20000000 << 64)   # q = 3 (the estimate 4 is one too many: add-back), r = 0x20000000 * 2^64
DIV_REM_EDGES = [
    ("a_zero", 4, 4, 0, Y128),
    ("all_ones", 4, 4, 2**128 - 1, 2**128 - 1),
    ("a_below_b", 4, 4, Y128, X128),
    ("a_equals_b", 4, 4, X128, X128),
    ("b_one_limb", 4, 1, X128, 0xFFFFFFFB),
    ("b_zero_top_limb", 4, 4, (Y128 >> 40) * 0xFFFF1234 + 77, Y128 >> 40),
    ("quotient_words_all_ones", 4, 3, 2**128 - 1, 2**64 + 1),
    ("add_back", 3, 3, ADD_BACK_A, ADD_BACK_B),
    ("div_without_limbs", 1, 3, 0xDEADBEEF, (7 << 64) + 5),     # lb > la + 1: mul_biguint places U32AddManyGate { num_addends: 0 }
]
