"""plonky2_ecdsa/biguint/gadgets/nonnative.rs:131-443 `CircuitBuilderNonNative` as a mixin of builder.CircuitBuilder, above
gadgets_biguint's: a NonNativeTarget<FF> is the list of its limbs, as a BigUintTarget is; FF is the `field` argument, a name of
NONNATIVE_FIELDS.  Its four generators belong to no gate: they are the generators "nnadd", "nnsub", "nnmul", "nninv", which the
witness plan lists as "nonnative_*".  `add_many_nonnative` is left out (nothing on the ECDSA path calls it)."""
from .builder import GENERATORS, GeneratorKind
from .gadgets_biguint import digits, integer
from .prover import WitnessPlan

# the two `FF` the reference instantiates (plonky2_ecdsa/curve/secp256k1.rs, glv.rs): name -> (p2gpu.h P2GPU_FIELD_*, order)
_ORDERS = {"secp256k1_base": 2**256 - 2**32 - 977, "secp256k1_scalar": 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141}
NONNATIVE_FIELDS = {name: (number, _ORDERS[name]) for name, number in WitnessPlan.NONNATIVE_FIELDS.items()}
NONNATIVE_EVENTS = {"nnadd": "nonnative_add", "nnsub": "nonnative_sub", "nnmul": "nonnative_mul", "nninv": "nonnative_inv"}


def _inverse(a, b, m):
    if a == 0:
        raise ValueError("unsatisfiable: inv_nonnative inverts zero")
    inv = pow(a, -1, m)
    return inv, a * inv // m


# the four generators' run_once (nonnative.rs:469-484, :589-604, :645-658, :691-703): (a, b, order) -> (first, second)
_RUN_ONCE = {"nnadd": lambda a, b, m: (a + b - m, 1) if a + b > m else (a + b, 0),          # (strictly: a + b == m leaves sum = m)
             "nnsub": lambda a, b, m: (a - b, 0) if a >= b else (m + a - b, 1),
             "nnmul": lambda a, b, m: divmod(a * b, m)[::-1],
             "nninv": _inverse}


class CircuitBuilderNonNative:
    @staticmethod
    def nonnative_order(field):
        """FF::order()"""
        return NONNATIVE_FIELDS[field][1]

    @staticmethod
    def num_nonnative_limbs(field):
        """nonnative.rs:127-129: ceil_div_usize(FF::BITS, 32)"""
        return -(-NONNATIVE_FIELDS[field][1].bit_length() // 32)

    def biguint_to_nonnative(self, x, field):
        """nonnative.rs:131-136"""
        return list(x)

    nonnative_to_canonical_biguint = biguint_to_nonnative      # nonnative.rs:138-143

    def constant_nonnative(self, x, field):
        """nonnative.rs:145-148: `x` an element of the field, as a Python integer"""
        assert 0 <= x < self.nonnative_order(field)
        return self.biguint_to_nonnative(self.constant_biguint(x), field)

    def zero_nonnative(self, field):
        """nonnative.rs:150-152"""
        return self.constant_nonnative(0, field)

    def connect_nonnative(self, lhs, rhs, field):
        """nonnative.rs:155-161: both assumed to be in reduced form"""
        self.connect_biguint(lhs, rhs)

    def add_virtual_nonnative_target(self, field):
        """nonnative.rs:163-171"""
        return self.add_virtual_biguint_target(self.num_nonnative_limbs(field))

    def add_virtual_nonnative_target_sized(self, num_limbs, field):
        """nonnative.rs:173-183"""
        return self.add_virtual_biguint_target(num_limbs)

    def add_nonnative(self, a, b, field):
        """nonnative.rs:185-215: (sum, overflow) from the NonNativeAdditionGenerator (event "nnadd": no gate's own), then
        a + b == sum + overflow * modulus and sum <= modulus (`cmp_biguint` is <=: sum = modulus passes, as upstream)."""
        a, b = list(a), list(b)
        total = self.add_virtual_nonnative_target(field)
        overflow = self.add_virtual_bool_target_unsafe()
        self._listed_generator("nnadd", a, b, total, (overflow,), field)
        sum_expected = self.add_biguint(a, b)
        modulus = self.constant_biguint(self.nonnative_order(field))
        mod_times_overflow = self.mul_biguint_by_bool(modulus, overflow)
        sum_actual = self.add_biguint(total, mod_times_overflow)
        self.connect_biguint(sum_expected, sum_actual)
        self.connect(self.cmp_biguint(total, modulus), self.one())
        return total

    def mul_nonnative_by_bool(self, a, b, field):
        """nonnative.rs:217-226"""
        return self.mul_biguint_by_bool(a, b)

    def if_nonnative(self, b, x, y, field):
        """nonnative.rs:228-238"""
        not_b = self.not_(b)
        maybe_x = self.mul_nonnative_by_bool(x, b, field)
        maybe_y = self.mul_nonnative_by_bool(y, not_b, field)
        return self.add_nonnative(maybe_x, maybe_y, field)

    def sub_nonnative(self, a, b, field):
        """nonnative.rs:284-310: (diff, overflow) from the NonNativeSubtractionGenerator (event "nnsub"), diff's limbs range-checked
        in one U32RangeCheckGate row, overflow a bit, then a == diff + b - overflow * modulus."""
        a, b = list(a), list(b)
        diff = self.add_virtual_nonnative_target(field)
        overflow = self.add_virtual_bool_target_unsafe()
        self._listed_generator("nnsub", a, b, diff, (overflow,), field)
        self.range_check_u32(diff)
        self.assert_bool(overflow)
        diff_plus_b = self.add_biguint(diff, b)
        modulus = self.constant_biguint(self.nonnative_order(field))
        mod_times_overflow = self.mul_biguint_by_bool(modulus, overflow)
        diff_plus_b_reduced = self.sub_biguint(diff_plus_b, mod_times_overflow)
        self.connect_biguint(a, diff_plus_b_reduced)
        return diff

    def mul_nonnative(self, a, b, field):
        """nonnative.rs:312-341: (prod, overflow) from the NonNativeMultiplicationGenerator (event "nnmul"), both range-checked,
        then a * b == prod + modulus * overflow.  overflow has len(a) + len(b) - 8 limbs (fewer than 8 operand limbs in all
        underflow upstream: ValueError).  A range check over no limbs (len(a) + len(b) == 8) places no row here: upstream's
        U32RangeCheckGate { num_input_limbs: 0 } constrains nothing and the gate table takes 1 limb at least."""
        a, b = list(a), list(b)
        prod = self.add_virtual_nonnative_target(field)
        modulus = self.constant_biguint(self.nonnative_order(field))
        if len(a) + len(b) < len(modulus):
            raise ValueError("mul_nonnative: %d + %d operand limbs are fewer than the modulus has" % (len(a), len(b)))
        overflow = self.add_virtual_biguint_target(len(a) + len(b) - len(modulus))
        self._listed_generator("nnmul", a, b, prod, overflow, field)
        self.range_check_u32(prod)
        if overflow:
            self.range_check_u32(overflow)
        prod_expected = self.mul_biguint(a, b)
        mod_times_overflow = self.mul_biguint(modulus, overflow)
        prod_actual = self.add_biguint(prod, mod_times_overflow)
        self.connect_biguint(prod_expected, prod_actual)
        return prod

    def mul_many_nonnative(self, to_mul, field):
        """nonnative.rs:343-356"""
        to_mul = list(to_mul)
        if len(to_mul) == 1:
            return to_mul[0]
        acc = self.mul_nonnative(to_mul[0], to_mul[1], field)
        for t in to_mul[2:]:
            acc = self.mul_nonnative(acc, t, field)
        return acc

    def neg_nonnative(self, x, field):
        """nonnative.rs:358-363: zero minus x, the zero a target without limbs"""
        zero_ff = self.biguint_to_nonnative(self.constant_biguint(0), field)
        return self.sub_nonnative(zero_ff, x, field)

    def inv_nonnative(self, x, field):
        """nonnative.rs:365-389: (inv, div) from the NonNativeInverseGenerator (event "nninv"), both with x's limbs, then
        x * inv == modulus * div + 1."""
        x = list(x)
        inv = self.add_virtual_biguint_target(len(x))
        div = self.add_virtual_biguint_target(len(x))
        self._listed_generator("nninv", x, (), inv, div, field)
        product = self.mul_biguint(x, inv)
        modulus = self.constant_biguint(self.nonnative_order(field))
        mod_times_div = self.mul_biguint(modulus, div)
        expected_product = self.add_biguint(mod_times_div, self.constant_biguint(1))
        self.connect_biguint(product, expected_product)
        return inv

    def reduce(self, x, field):
        """nonnative.rs:391-401: x % |FF| through `rem_biguint`"""
        return self.rem_biguint(x, self.constant_biguint(self.nonnative_order(field)))

    def reduce_nonnative(self, x, field):
        """nonnative.rs:403-406"""
        return self.reduce(self.nonnative_to_canonical_biguint(x, field), field)

    def bool_to_nonnative(self, b, field):
        """nonnative.rs:408-416: one limb"""
        return [b]

    def split_nonnative_to_bits(self, x, field):
        """nonnative.rs:418-430: 32 bits per limb, least significant first"""
        return [bit for limb in x for bit in self.split_le(limb, 32)]

    def nonnative_conditional_neg(self, x, b, field):
        """nonnative.rs:432-443"""
        not_b = self.not_(b)
        neg = self.neg_nonnative(x, field)
        x_if_true = self.mul_nonnative_by_bool(neg, b, field)
        x_if_false = self.mul_nonnative_by_bool(x, not_b, field)
        return self.add_nonnative(x_if_true, x_if_false, field)

    @staticmethod
    def nonnative_values(event, field, a_limbs, b_limbs, first_limbs, second_limbs):
        """A generator's run_once on limb values: A and B are the operands' integers (`get_biguint_target`) reduced modulo the
        order (FF::from_noncanonical_biguint).  Returns the two targets' 32-bit digits.  ValueError where upstream panics: the
        inverse of zero, or more digits than limbs (`set_biguint_target`)."""
        m = NONNATIVE_FIELDS[field][1]
        first, second = _RUN_ONCE[event](integer(a_limbs) % m, integer(b_limbs) % m, m)
        if first >> (32 * first_limbs) or second >> (32 * second_limbs):
            raise ValueError("unsatisfiable: a nonnative generator's value has more digits than its target has limbs")
        return digits(first, first_limbs), digits(second, second_limbs)


def _body(ev, vs):
    a, _, first, second = ev.groups
    x, y = CircuitBuilderNonNative.nonnative_values(ev.kind, ev.field, vs[:len(a)], vs[len(a):], len(first), len(second))
    return x + y


GENERATORS.update({event: GeneratorKind(_body, plan, plan + ": a limb of the generator", given=True) for event, plan in NONNATIVE_EVENTS.items()})
