"""plonky2_ecdsa/biguint/gadgets/split_nonnative.rs:28-60 `CircuitBuilderSplit` and plonky2_ecdsa/curve/gadgets/curve.rs:98-262
`CircuitBuilderCurve` as mixins of builder.CircuitBuilder, above gadgets_nonnative's.  An AffinePointTarget is the pair (x, y) of
two NonNativeTarget<Secp256K1Base>, each the list of its limbs; the arithmetic is incomplete as upstream's is (no zero point, no
doubling through `curve_add`).  Every gadget keeps the order of upstream's nonnative calls: that order fixes the rows.
The one deviation: `curve_scalar_mul` draws its starting point from the builder's seeded generator, upstream from the thread's."""
BASE, SCALAR = "secp256k1_base", "secp256k1_scalar"
SECP256K1_A, SECP256K1_B = 0, 7                                   # curve.rs:13-14
# curve.rs:17-30
SECP256K1_GENERATOR_X = 0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798
SECP256K1_GENERATOR_Y = 0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8


class CircuitBuilderSplit:
    def split_u32_to_4_bit_limbs(self, val):
        """split_nonnative.rs:28-38: sixteen base-4 limbs, paired as b * 4 + a"""
        two_bit_limbs = self.split_le_base(val, 16, 4)
        four = self.constant(4)
        return [self.mul_add(b, four, a) for a, b in zip(two_bit_limbs[0::2], two_bit_limbs[1::2])]

    def split_nonnative_to_4_bit_limbs(self, val, field):
        """split_nonnative.rs:40-49"""
        return [t for limb in val for t in self.split_u32_to_4_bit_limbs(limb)]

    def split_nonnative_to_2_bit_limbs(self, val, field):
        """split_nonnative.rs:51-60: one BaseSumGate<4>{16} row per limb"""
        return [t for limb in val for t in self.split_le_base(limb, 16, 4)]


class CircuitBuilderCurve:
    def generate_random_point(self):
        """curve.rs:32-43, from the builder's seeded generator (upstream: Secp256K1Base::rand(), the thread's): an x whose
        x^3 + 7 is a square, and y = (x^3 + 7)^((P + 1) / 4), a root since P = 3 mod 4.  Integers, as upstream returns them."""
        p = self.nonnative_order(BASE)
        while True:
            x = sum(int(w) << (64 * i) for i, w in enumerate(self.rng.integers(0, 1 << 64, size=4, dtype="uint64"))) % p
            c = (x * x * x + SECP256K1_B) % p
            y = pow(c, (p + 1) // 4, p)
            if x and y and y * y % p == c:
                return x, y

    def constant_affine_point(self, x, y):
        """curve.rs:98-104: x, y integers below the base field's order, neither zero"""
        assert x and y
        return self.constant_nonnative(x, BASE), self.constant_nonnative(y, BASE)

    def connect_affine_point(self, lhs, rhs):
        """curve.rs:106-109"""
        self.connect_nonnative(lhs[0], rhs[0], BASE)
        self.connect_nonnative(lhs[1], rhs[1], BASE)

    def add_virtual_affine_point_target(self):
        """curve.rs:111-116"""
        x = self.add_virtual_nonnative_target(BASE)
        y = self.add_virtual_nonnative_target(BASE)
        return x, y

    def curve_assert_valid(self, p):
        """curve.rs:118-130: y^2 == x^3 + a x + b (a = 0: the constant without limbs)"""
        px, py = p
        a = self.constant_nonnative(SECP256K1_A, BASE)
        b = self.constant_nonnative(SECP256K1_B, BASE)
        y_squared = self.mul_nonnative(py, py, BASE)
        x_squared = self.mul_nonnative(px, px, BASE)
        x_cubed = self.mul_nonnative(x_squared, px, BASE)
        a_x = self.mul_nonnative(a, px, BASE)
        a_x_plus_b = self.add_nonnative(a_x, b, BASE)
        rhs = self.add_nonnative(x_cubed, a_x_plus_b, BASE)
        self.connect_nonnative(y_squared, rhs, BASE)

    def curve_neg(self, p):
        """curve.rs:132-138"""
        return p[0], self.neg_nonnative(p[1], BASE)

    def curve_conditional_neg(self, p, b):
        """curve.rs:140-145"""
        return p[0], self.nonnative_conditional_neg(p[1], b, BASE)

    def curve_double(self, p):
        """curve.rs:147-169"""
        x, y = p
        double_y = self.add_nonnative(y, y, BASE)
        inv_double_y = self.inv_nonnative(double_y, BASE)
        x_squared = self.mul_nonnative(x, x, BASE)
        double_x_squared = self.add_nonnative(x_squared, x_squared, BASE)
        triple_x_squared = self.add_nonnative(double_x_squared, x_squared, BASE)
        a = self.constant_nonnative(SECP256K1_A, BASE)
        triple_xx_a = self.add_nonnative(triple_x_squared, a, BASE)
        lam = self.mul_nonnative(triple_xx_a, inv_double_y, BASE)
        lambda_squared = self.mul_nonnative(lam, lam, BASE)
        x_double = self.add_nonnative(x, x, BASE)
        x3 = self.sub_nonnative(lambda_squared, x_double, BASE)
        x_diff = self.sub_nonnative(x, x3, BASE)
        lambda_x_diff = self.mul_nonnative(lam, x_diff, BASE)
        y3 = self.sub_nonnative(lambda_x_diff, y, BASE)
        return x3, y3

    def curve_repeated_double(self, p, n):
        """curve.rs:171-179"""
        for _ in range(n):
            p = self.curve_double(p)
        return p

    def curve_add(self, p1, p2):
        """curve.rs:181-197: the points are assumed to differ in x (the inverse of zero is unsatisfiable)"""
        (x1, y1), (x2, y2) = p1, p2
        u = self.sub_nonnative(y2, y1, BASE)
        v = self.sub_nonnative(x2, x1, BASE)
        v_inv = self.inv_nonnative(v, BASE)
        s = self.mul_nonnative(u, v_inv, BASE)
        s_squared = self.mul_nonnative(s, s, BASE)
        x_sum = self.add_nonnative(x2, x1, BASE)
        x3 = self.sub_nonnative(s_squared, x_sum, BASE)
        x_diff = self.sub_nonnative(x1, x3, BASE)
        prod = self.mul_nonnative(s, x_diff, BASE)
        y3 = self.sub_nonnative(prod, y1, BASE)
        return x3, y3

    def curve_conditional_add(self, p1, p2, b):
        """curve.rs:199-216: p1 + p2 when b, else p1; the sum is computed either way"""
        not_b = self.not_(b)
        total = self.curve_add(p1, p2)
        x_if_true = self.mul_nonnative_by_bool(total[0], b, BASE)
        y_if_true = self.mul_nonnative_by_bool(total[1], b, BASE)
        x_if_false = self.mul_nonnative_by_bool(p1[0], not_b, BASE)
        y_if_false = self.mul_nonnative_by_bool(p1[1], not_b, BASE)
        x = self.add_nonnative(x_if_true, x_if_false, BASE)
        y = self.add_nonnative(y_if_true, y_if_false, BASE)
        return x, y

    def curve_scalar_mul(self, p, n):
        """curve.rs:218-258: double-and-add over the bits of n (a NonNativeTarget<Secp256K1Scalar>), from a random point that is
        subtracted at the end (see generate_random_point for where it comes from here)."""
        bits = self.split_nonnative_to_bits(n, SCALAR)
        randot = self.constant_affine_point(*self.generate_random_point())
        result = self.add_virtual_affine_point_target()
        self.connect_affine_point(randot, result)
        two_i_times_p = self.add_virtual_affine_point_target()
        self.connect_affine_point(p, two_i_times_p)
        for bit in bits:
            not_bit = self.not_(bit)
            result_plus_2_i_p = self.curve_add(result, two_i_times_p)
            new_x_if_bit = self.mul_nonnative_by_bool(result_plus_2_i_p[0], bit, BASE)
            new_x_if_not_bit = self.mul_nonnative_by_bool(result[0], not_bit, BASE)
            new_y_if_bit = self.mul_nonnative_by_bool(result_plus_2_i_p[1], bit, BASE)
            new_y_if_not_bit = self.mul_nonnative_by_bool(result[1], not_bit, BASE)
            new_x = self.add_nonnative(new_x_if_bit, new_x_if_not_bit, BASE)
            new_y = self.add_nonnative(new_y_if_bit, new_y_if_not_bit, BASE)
            result = (new_x, new_y)
            two_i_times_p = self.curve_double(two_i_times_p)
        neg_r = self.curve_neg(randot)
        return self.curve_add(result, neg_r)

    def curve_generator_constant(self):
        """curve.rs:260-262"""
        return self.constant_affine_point(SECP256K1_GENERATOR_X, SECP256K1_GENERATOR_Y)
