"""plonky2_ecdsa/biguint/biguint.rs `CircuitBuilderBiguint` as a mixin of builder.CircuitBuilder, above gadgets_u32's: a
BigUintTarget is the list of its U32Target limbs, least significant first.  `div_rem_biguint`'s BigUintDivRemGenerator belongs to
no gate: it is the generator "divrem", which the witness plan lists as "biguint_divrem"."""
from .builder import GENERATORS, Generator, GeneratorKind
from .gadgets_u32 import U32_MAX


def digits(v, count):                                # `count` 32-bit digits of v, least significant first
    return [(v >> (32 * i)) & U32_MAX for i in range(count)]


def integer(limbs):                                  # `get_biguint_target`: sum limb_i 2^(32 i) (a limb >= 2^32 carries into the next)
    return sum(v << (32 * i) for i, v in enumerate(limbs))


class CircuitBuilderBiguint:
    def constant_biguint(self, value):
        """biguint.rs:81-86 (`to_u32_digits`: zero has no limbs)"""
        limbs = []
        while value:
            limbs.append(self.constant_u32(value & U32_MAX))
            value >>= 32
        return limbs

    def zero_biguint(self):
        """biguint.rs:88-90"""
        return self.constant_biguint(0)

    def connect_biguint(self, lhs, rhs):
        """biguint.rs:92-104: the common limbs are connected, the others are zero."""
        m = min(len(lhs), len(rhs))
        for x, y in zip(lhs[:m], rhs[:m]):
            self.connect_u32(x, y)
        for x in lhs[m:] + rhs[m:]:
            self.assert_zero_u32(x)

    def pad_biguints(self, a, b):
        """biguint.rs:106-126"""
        n = max(len(a), len(b))
        return list(a) + [self.zero_u32()] * (n - len(a)), list(b) + [self.zero_u32()] * (n - len(b))

    def cmp_biguint(self, a, b):
        """biguint.rs:128-132: a <= b"""
        a, b = self.pad_biguints(a, b)
        return self.list_le_u32(a, b)

    def add_virtual_biguint_target(self, num_limbs):
        """biguint.rs:134-138"""
        return self.add_virtual_u32_targets(num_limbs)

    def add_biguint(self, a, b):
        """biguint.rs:140-162: max(len) + 1 limbs"""
        out, carry = [], self.zero_u32()
        for i in range(max(len(a), len(b))):
            x = a[i] if i < len(a) else self.zero_u32()
            y = b[i] if i < len(b) else self.zero_u32()
            limb, carry = self.add_many_u32([carry, x, y])
            out.append(limb)
        return out + [carry]

    def sub_biguint(self, a, b):
        """biguint.rs:164-181: a - b for a >= b (the last borrow is not constrained, as upstream)"""
        a, b = self.pad_biguints(a, b)
        out, borrow = [], self.zero_u32()
        for x, y in zip(a, b):
            limb, borrow = self.sub_u32(x, y, borrow)
            out.append(limb)
        return out

    def mul_biguint(self, a, b):
        """biguint.rs:183-207: len(a) + len(b) + 1 limbs"""
        to_add = [[] for _ in range(len(a) + len(b))]
        for i, x in enumerate(a):
            for j, y in enumerate(b):
                product, carry = self.mul_u32(x, y)
                to_add[i + j].append(product)
                to_add[i + j + 1].append(carry)
        out, carry = [], self.zero_u32()
        for summands in to_add:
            limb, carry = self.add_u32s_with_carry(summands, carry)
            out.append(limb)
        return out + [carry]

    def mul_biguint_by_bool(self, a, b):
        """biguint.rs:209-219"""
        return [self.mul(l, b) for l in a]

    def mul_add_biguint(self, x, y, z):
        """biguint.rs:221-229"""
        return self.add_biguint(self.mul_biguint(x, y), z)

    def _listed_generator(self, kind, a, b, first, second, field=None):
        """Records a generator the witness plan lists: it reads the limbs of a and b and sets those of `first` and `second`."""
        groups = (tuple(a), tuple(b), tuple(first), tuple(second))
        self.events.append(Generator(kind, groups[0] + groups[1], groups[2] + groups[3], groups=groups, field=field))

    def div_rem_biguint(self, a, b):
        """biguint.rs:231-262: (div, rem) from the BigUintDivRemGenerator (event "divrem": no gate's own), then
        a == div * b + rem and rem <= b as upstream states it."""
        a, b = list(a), list(b)
        div = self.add_virtual_biguint_target(0 if len(b) > len(a) + 1 else len(a) - len(b) + 1)
        rem = self.add_virtual_biguint_target(len(b))
        self._listed_generator("divrem", a, b, div, rem)
        div_b_plus_rem = self.add_biguint(self.mul_biguint(div, b), rem)
        self.connect_biguint(a, div_b_plus_rem)
        self.assert_one(self.cmp_biguint(rem, b))
        return div, rem

    def div_biguint(self, a, b):
        """biguint.rs:264-267"""
        return self.div_rem_biguint(a, b)[0]

    def rem_biguint(self, a, b):
        """biguint.rs:269-272"""
        return self.div_rem_biguint(a, b)[1]

    @staticmethod
    def divrem_values(a_limbs, b_limbs, div_limbs, rem_limbs):
        """BigUintDivRemGenerator::run_once (biguint.rs:337-344) on limb values: (div, rem) = divmod(a, b) of the operands'
        integers, as `div_limbs` and `rem_limbs` 32-bit digits.  ValueError where upstream panics: b = 0, or more digits than
        limbs."""
        a, b = integer(a_limbs), integer(b_limbs)
        if b == 0:
            raise ValueError("unsatisfiable: div_rem_biguint divides by zero")
        q, r = divmod(a, b)
        if q >> (32 * div_limbs) or r >> (32 * rem_limbs):
            raise ValueError("unsatisfiable: div_rem_biguint: the quotient or the remainder has more digits than its target has limbs")
        return digits(q, div_limbs), digits(r, rem_limbs)


def _divrem_body(ev, vs):
    a, _, div, rem = ev.groups
    q, r = CircuitBuilderBiguint.divrem_values(vs[:len(a)], vs[len(a):], len(div), len(rem))
    return q + r


GENERATORS["divrem"] = GeneratorKind(_divrem_body, "biguint_divrem", "div_rem_biguint: a limb of the div-rem generator", given=True)
