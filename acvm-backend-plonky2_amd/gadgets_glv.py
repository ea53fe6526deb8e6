"""plonky2_ecdsa/curve/gadgets/glv.rs:23-255, :339-383 `CircuitBuilderGlv`, `curve_msm_circuit` and `random_access_curve_points` as a
mixin of builder.CircuitBuilder, above gadgets_curve's.  The GLVDecompositionGenerator (glv.rs:258-285) belongs to no gate: it is
the generator "glvdec", which the witness plan lists as "glv_decompose".  `precompute_window` (glv.rs:325-337) has no caller
upstream and is left out."""
from .builder import GENERATORS, GeneratorKind
from .gadgets_biguint import digits, integer
from .gadgets_curve import BASE, SCALAR
from .gadgets_nonnative import NONNATIVE_FIELDS

N = NONNATIVE_FIELDS[SCALAR][1]
# glv.rs:23-44 (little-endian u64 words there)
GLV_BETA = 0x7AE96A2B657C07106E64479EAC3434E99CF0497512F58995C1396C28719501EE
GLV_S = 0x5363AD4CC05C30E0A5261C028812645A122E22EA20816678DF02967C1B23BD72
A1 = 0x3086D221A7D46BCDE86C90E49284EB15
MINUS_B1 = 0xE4437ED6010E88286F547FA90ABFE4C3
A2 = 0x114CA50F7A8E2F3F657C1108D9D44CFD8
B2 = 0x3086D221A7D46BCDE86C90E49284EB15
# glv.rs:186-206, :241-250: curve_msm_circuit's starting point, its negative, and the correction that is added at the end
MSM_RANDO = (0xA86C70FE28EB2CB4E881AA81971AE5121389F53E8B82771E5435099CAAACA00F,
             0x3C20A74F2CC59D7DF8BE94B58EE35F088885C02B6E16821DABDD5C2B0901B91B)
MSM_NEG_RANDO = (MSM_RANDO[0], 0xC3DF58B0D33A628207416B4A711CA0F7777A3FD491E97DE25422A3D3F6FE4314)
MSM_TO_ADD = (0x04F07480028E1A4379E40FAC7D38B237DCB21FC25AA8287F3BC10079ECB2821D,
              0xC3144A41D7A799C9EB6EE728CF791E371210CD8AA94214FD31362398F775F69B)
GLV_LIMBS = 4                                            # k1 and k2: add_virtual_nonnative_target_sized(4)


def _round_div(a, b):                                    # Ratio::new(a, b).round() for an odd b: no ties
    return (2 * a + b) // (2 * b)


def decompose_secp256k1_scalar(k):
    """glv.rs:50-88 on integers: k in [0, N) -> (|k1|, |k2|, k1 < 0, k2 < 0) with k1 + GLV_S * k2 == k modulo N
    (Algorithm 15.41, Handbook of Elliptic and Hyperelliptic Curve Cryptography)."""
    assert 0 <= k < N
    c1 = _round_div(B2 * k, N) % N
    c2 = _round_div(MINUS_B1 * k, N) % N
    k1_raw = (k - c1 * A1 - c2 * A2) % N
    k2_raw = (c1 * MINUS_B1 - c2 * B2) % N
    assert (k1_raw + GLV_S * k2_raw) % N == k
    k1_neg, k2_neg = k1_raw > N // 2, k2_raw > N // 2
    return (N - k1_raw if k1_neg else k1_raw), (N - k2_raw if k2_neg else k2_raw), k1_neg, k2_neg


class CircuitBuilderGlv:
    def secp256k1_glv_beta(self):
        """glv.rs:113-115"""
        return self.constant_nonnative(GLV_BETA, BASE)

    def decompose_secp256k1_scalar(self, k):
        """glv.rs:117-149: (k1, k2, k1_neg, k2_neg) from the GLVDecompositionGenerator (event "glvdec"), k1 and k2 of four limbs,
        the two signs unsafe bools, then k1_raw + GLV_S * k2_raw == k over the scalar field."""
        k = list(k)
        k1 = self.add_virtual_nonnative_target_sized(GLV_LIMBS, SCALAR)
        k2 = self.add_virtual_nonnative_target_sized(GLV_LIMBS, SCALAR)
        k1_neg = self.add_virtual_bool_target_unsafe()
        k2_neg = self.add_virtual_bool_target_unsafe()
        self._listed_generator("glvdec", k, (), k1 + k2, (k1_neg, k2_neg))
        k1_raw = self.nonnative_conditional_neg(k1, k1_neg, SCALAR)
        k2_raw = self.nonnative_conditional_neg(k2, k2_neg, SCALAR)
        s = self.constant_nonnative(GLV_S, SCALAR)
        should_be_k = self.mul_nonnative(s, k2_raw, SCALAR)
        should_be_k = self.add_nonnative(should_be_k, k1_raw, SCALAR)
        self.connect_nonnative(should_be_k, k, SCALAR)
        return k1, k2, k1_neg, k2_neg

    def glv_mul(self, p, k):
        """glv.rs:151-168: k * p as k1 * (+-p) + k2 * (+-(beta x, y))"""
        k1, k2, k1_neg, k2_neg = self.decompose_secp256k1_scalar(k)
        beta = self.secp256k1_glv_beta()
        beta_px = self.mul_nonnative(beta, p[0], BASE)
        sp = (beta_px, p[1])
        p_neg = self.curve_conditional_neg(p, k1_neg)
        sp_neg = self.curve_conditional_neg(sp, k2_neg)
        return self.curve_msm_circuit(p_neg, sp_neg, k1, k2)

    def curve_msm_circuit(self, p, q, n, m):
        """glv.rs:175-255: n * p + m * q with a two-bit window (Algorithm 9.23 of the same handbook), for p != q; n and m have
        the same number of limbs (upstream passes four).  precomputation[i + 4 j] = i p + j q, entries 0 kept at the starting
        point; per window two doublings, one random access, one conditional add (skipped for index 0)."""
        limbs_n = self.split_nonnative_to_2_bit_limbs(n, SCALAR)
        limbs_m = self.split_nonnative_to_2_bit_limbs(m, SCALAR)
        assert len(limbs_n) == len(limbs_m)
        rando_t = self.constant_affine_point(*MSM_RANDO)
        neg_rando = self.constant_affine_point(*MSM_NEG_RANDO)
        precomputation = [p] * 16
        cur_p = cur_q = rando_t
        for i in range(4):
            precomputation[i] = cur_p
            precomputation[4 * i] = cur_q
            cur_p = self.curve_add(cur_p, p)
            cur_q = self.curve_add(cur_q, q)
        for i in range(1, 4):
            precomputation[i] = self.curve_add(precomputation[i], neg_rando)
            precomputation[4 * i] = self.curve_add(precomputation[4 * i], neg_rando)
        for i in range(1, 4):
            for j in range(1, 4):
                precomputation[i + 4 * j] = self.curve_add(precomputation[i], precomputation[4 * j])
        four = self.constant(4)
        zero = self.zero()
        result = rando_t
        for limb_n, limb_m in reversed(list(zip(limbs_n, limbs_m))):
            result = self.curve_repeated_double(result, 2)
            index = self.mul_add(four, limb_m, limb_n)
            r = self.random_access_curve_points(index, precomputation)
            is_zero = self.is_equal(index, zero)
            should_add = self.not_(is_zero)
            result = self.curve_conditional_add(result, r, should_add)
        to_add = self.constant_affine_point(*MSM_TO_ADD)
        return self.curve_add(result, to_add)

    def random_access_curve_points(self, access_index, v):
        """glv.rs:339-383: limb i of every point's x, then of every y, through one `random_access` each (sixteen in all); a
        point with fewer than eight limbs reads the zero u32 there."""
        num_limbs = 8
        zero = self.zero_u32()
        x_limbs = [[pt[0][i] if i < len(pt[0]) else zero for pt in v] for i in range(num_limbs)]
        y_limbs = [[pt[1][i] if i < len(pt[1]) else zero for pt in v] for i in range(num_limbs)]
        selected_x = [self.random_access(access_index, limbs) for limbs in x_limbs]
        selected_y = [self.random_access(access_index, limbs) for limbs in y_limbs]
        return selected_x, selected_y

    @staticmethod
    def glv_values(k_limbs, k1_limbs=GLV_LIMBS, k2_limbs=GLV_LIMBS):
        """GLVDecompositionGenerator::run_once (glv.rs:274-285) on limb values: k = fold(k) mod N (`from_noncanonical_biguint`),
        then k1's digits, k2's, and the two signs.  ValueError where `set_biguint_target` panics: more digits than limbs."""
        k1, k2, k1_neg, k2_neg = decompose_secp256k1_scalar(integer(k_limbs) % N)
        if k1 >> (32 * k1_limbs) or k2 >> (32 * k2_limbs):
            raise ValueError("unsatisfiable: the GLV decomposition has more digits than its target has limbs")
        return digits(k1, k1_limbs) + digits(k2, k2_limbs) + [int(k1_neg), int(k2_neg)]


GENERATORS["glvdec"] = GeneratorKind(lambda ev, vs: CircuitBuilderGlv.glv_values(vs), "glv_decompose",
                                     "decompose_secp256k1_scalar: a limb of the GLV decomposition generator", given=True)
