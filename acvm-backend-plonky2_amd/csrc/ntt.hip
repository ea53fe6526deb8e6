// ntt.hip -- batched Goldilocks NTT for gfx950: LDS-tiled passes, radix-8/4/2
// register rounds with shift twiddles.
//
// Replaces (inside `circuit_data.prove`, plonky2-backend/src/actions/prove_action.rs:96)
// plonky2 0.2.2 field/src/fft.rs `fft_classic` / `ifft` and
// PolynomialCoeffs::lde + coset_fft.
//
// MI355X-first layout instead of plonky2's natural->natural transforms:
//   * values -> coefficients is a DIF transform (natural in, BIT-REVERSED out);
//     coefficients stay in bit-reversed positions for their whole life;
//   * the 8x LDE on the coset g<w_N> (g = GL_GEN) is 8 independent size-n DIT transforms
//     (bit-reversed in, natural out) with coset shifts g*w_N^r, r < 8; natural
//     LDE row i = 8k + r is output k of coset r.  No transpose, no bit-reversal
//     pass and no zero-padded 8n-point FFT ever touches HBM.
// A transform of 2^d points is split into passes of <= 12 layers; a pass stages a
// 2^12-element tile (32 KB, XOR-swizzled: pidx() below) in LDS and reads/writes HBM in runs of
// >= 128 contiguous bytes.  Inside a pass the layers are done in rounds of up to
// three: a lane holds 8 elements in registers, multiplies them by 7 per-group
// twiddles (one coalesced load each from a table packed per round -- no index
// arithmetic, no scattered root-table gathers) and then runs an 8-point DFT whose
// internal twiddles are powers of w_8 = 2^24, i.e. shifts (2 is a 192nd
// root of unity in Goldilocks): 7 general modmuls per 8 elements per three
// layers instead of 12.  This kernel is VALU-issue bound on gfx950, in the HALF-rate
// instruction class (carry chains, v_mad_u64_u32: 4.2 cycles per wave64 instruction,
// profiles/r03_ubench.txt): 0.73-0.82 of the 39.5 T lane-instr/s its mix allows.
// HBM traffic of a 2^17-point LDE: 25n * 8 B per dense column against 9n * 8 B
// algorithmic (the intermediate between the 12-layer and the 5-layer pass goes out
// and back: a 1 MB column-coset does not fit a CU's LDS) -- 2.5 TB/s while the
// kernel runs, not its limiter.  No MFMA.
#include "internal.hpp"
#include <algorithm>
#include <memory>
#include <vector>

namespace p2 {

// exponent of 2 for the constant twiddle w_{2^(lam+1)}^q (w_64 = 2^3), mod 192
__host__ __device__ constexpr int tw_exp(int lam, int q, bool inv) {
  int e = (3 * (32 >> lam) * q) % 192;
  return inv ? (192 - e) % 192 : e;
}
__host__ __device__ constexpr int brev_c(int x, int bits) {
  int r = 0;
  for (int i = 0; i < bits; i++) r |= ((x >> i) & 1) << (bits - 1 - i);
  return r;
}

// in-register 2^LOGR-point DFT; DIT: bit-reversed in -> natural out; DIF: natural in -> bit-reversed out
template <int LOGR, int DIT, bool INV>
__device__ __forceinline__ void dft_regs(gl_t (&v)[1 << LOGR]) {
  constexpr int R = 1 << LOGR;
  static_for<0, LOGR>([&](auto lc) {
    constexpr int lam = DIT ? decltype(lc)::value : LOGR - 1 - decltype(lc)::value;
    static_for<0, R>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      if constexpr ((j & (1 << lam)) == 0) {
        constexpr int k = j | (1 << lam);
        constexpr int e = tw_exp(lam, j & ((1 << lam) - 1), INV);
        if constexpr (DIT) {
          const gl_t u = v[j];
          if constexpr (e < 96) {
            const gl_t t = mul_pow2<e>(v[k]);
            v[j] = gl_add(u, t);
            v[k] = gl_sub(u, t);
          } else {
            const gl_t t = mul_pow2<e - 96>(v[k]);  // twiddle = -2^(e-96)
            v[j] = gl_sub(u, t);
            v[k] = gl_add(u, t);
          }
        } else {
          const gl_t u = v[j], x = v[k];
          v[j] = gl_add(u, x);
          if constexpr (e < 96) v[k] = mul_pow2<e>(gl_sub(u, x));
          else v[k] = mul_pow2<e - 96>(gl_sub(x, u));
        }
      }
    });
  });
}

// LDS index swizzle.  ds_read_b64 serves a
// wave in two groups of 32 lanes over 32 eight-byte slots, ds_write_b64 in four groups of 16 lanes over 16 slots
// (MI355X_MICROARCH.md, LDS).  In a round on tile bits [beta0, beta0 + 3) the lanes of a group differ in element bits
// {3..7} (beta0 = 0), {0,1,2,6,7} (beta0 = 3) or {0..4} (beta0 >= 5, and the load / store phases): the slot bits
//   s0 = e0^e4, s1 = e1^e5, s2 = e2^e6, s3 = e3^e6, s4 = e4^e7
// are a GF(2)-linear map of full rank on each of those sets (and s0..s3 on the first four bits of each for the
// stores), so every access of the d >= 12 plans is conflict-free with no padding at all.  Linear means
// swz(a ^ b) = swz(a) ^ swz(b): a lane's eight addresses are swz(base) ^ swz(j << beta0), the second term wave-uniform.
__device__ __forceinline__ uint32_t pidx(uint32_t e) { return e ^ ((e >> 4) & 7u) ^ ((e >> 3) & 0x18u); }

// A full tile is 2^12 elements (32 KB of LDS) on 512 lanes that hold 8 elements each, so the largest round is radix 8; smaller
// transforms run on one smaller tile.  (Radix-16 rounds on 256 lanes and a 2^13 tile were built and measured slower; the
// wave-private rounds and the direct kernels below are written for exactly this shape.)
constexpr int NTT_TILE_BITS = 12;
constexpr int NTT_PER = 8;
constexpr int NTT_THREADS = (1 << NTT_TILE_BITS) / NTT_PER;
// waves per SIMD the full-tile kernels are compiled for: 8 = four 512-lane workgroups per CU, i.e. <= 64 VGPRs.  hipcc reaches
// 59-60 on its own; saying so makes it schedule for that bound (LDE 1.22-1.24 -> 1.205-1.21 ms at 2^20 rows) and
// keeps an edit that would silently cost a quarter of the occupancy (every variant above 64 VGPRs measured 20-30 % slower)
// from compiling into one
constexpr int NTT_MIN_WAVES = 8;
static_assert(NTT_THREADS == 512, "wave-private rounds and direct passes: 512 lanes x 8 elements");
constexpr int MAX_ROUNDS = NTT_MAX_ROUNDS;
struct PassArgs {
  const gl_t *src;    // [cols][n] (or [cosets][cols][n])
  gl_t *dst;          // [cosets][cols][n]
  const gl_t *ptw;    // packed per-round twiddles of this plan
  const gl_t *scale;  // optional [cosets][n], multiplied into the input of the first DIT pass
  gl_t post;          // multiplied into the output of the last pass (1 = none)
  uint32_t d;         // log2 n
  uint32_t s;         // log2 global stride of the pass's lowest layer
  uint32_t a;         // layers in this pass
  uint32_t tb;        // log2 contiguous run; tile = 2^(a+tb)
  uint32_t cols;        // column stride between cosets in src / dst
  uint32_t tiles, cols_grid, cosets;  // launch shape (1-D grid, decoded XCD-aware in the kernel)
  uint32_t src_single;  // 1: src has no coset dimension
  uint32_t coset_first, coset_stride;  // global coset of grid.z = first + z * stride (indexes `scale`)
  uint32_t nrounds;
  uint32_t r[MAX_ROUNDS];       // layers per round, ascending tile bit
  uint32_t tw_off[MAX_ROUNDS];  // offset of the round's table in ptw
  const uint32_t *colnz;        // optional [cols]: class of every column (ColHints, internal.hpp); only class 2 (dense)
                                // columns are transformed here, the others are written by structured_fill_kernel
  const gl_t *ftw;              // direct strided passes: folded twiddles of the round before the last (fold_table_kernel)
  const gl_t *ftw2;             // direct head / tail pass: the same kind of table in its lane order (head_fold_table_kernel)
};

__device__ __forceinline__ uint32_t gidx(uint32_t e, uint32_t hi_base, uint32_t lo0, uint32_t s, uint32_t tb) {
  return hi_base + ((e >> tb) << s) + lo0 + (e & ((1u << tb) - 1));
}

// block -> (tile, column, coset), false when the block has nothing to do.  1-D grid decoded XCD-aware: the hardware deals
// consecutive block ids round-robin over the 8 XCDs, each with its own L2.  The 2^rate_bits coset transforms of one (tile, column)
// read the SAME coefficients (and neighbouring rows of the scale table): they get consecutive slots of ONE XCD, so the tile comes
// from HBM once and from that XCD's L2 afterwards (a speed choice only: any placement gives the same result).
__device__ __forceinline__ bool pass_unit(const PassArgs &A, uint32_t &tile, uint32_t &col, uint32_t &coset) {
  const uint32_t units = A.tiles * A.cols_grid;
  const uint32_t xcd = blockIdx.x & 7u, slot = blockIdx.x >> 3;
  coset = slot % A.cosets;
  const uint32_t unit = (slot / A.cosets) * 8u + xcd;
  if (unit >= units) return false;
  tile = unit % A.tiles;
  col = unit / A.tiles;
  // Structured columns (internal.hpp ColHints): a transform is linear, so a zero column maps to zeros and
  // v * (unit column of the fixed row) to v * (that unit column's transform): structured_fill_kernel wrote them,
  // nothing to do here (block-uniform scalar branch).
  return !(A.colnz != nullptr && A.colnz[col] != 2u);
}
// the column of (col, coset) in src and dst, and the coset's row of the scale table (nullptr: none)
struct ColPtrs {
  const gl_t *src;
  gl_t *dst;
  const gl_t *scale;
};
__device__ __forceinline__ ColPtrs col_ptrs(const PassArgs &A, uint32_t col, uint32_t coset) {
  const size_t n = (size_t)1 << A.d;
  return {A.src + ((size_t)(A.src_single ? 0 : coset) * A.cols + col) * n, A.dst + ((size_t)coset * A.cols + col) * n,
          A.scale ? A.scale + (size_t)(A.coset_first + coset * A.coset_stride) * n : nullptr};
}
// tile -> global index of its hi block and first lo-run: element e of the tile is gidx(e, hi_base, lo0, s, tb)
struct TilePos {
  uint32_t hi_base, lo0;
};
__device__ __forceinline__ TilePos tile_pos(const PassArgs &A, uint32_t tile) {
  const uint32_t runs = 1u << (A.s - A.tb);  // lo-runs per hi block
  const uint32_t hi = tile / runs, lo0 = (tile % runs) << A.tb;
  return {hi << (A.s + A.a), lo0};
}

// Twiddle tables hold one row per exponent e; register j of a round takes row bitrev(j).
// rows 1 .. R-1 of a packed table T[(e-1) * M + lo] (round_table_kernel), tp = &T[lo], stride = M; row 0 is 1 and not stored
template <int R>
__device__ __forceinline__ void load_packed(gl_t (&t)[R], const gl_t *tp, size_t stride) {
#pragma unroll
  for (int e = 1; e < R; e++) {
    t[e] = *tp;
    tp += stride;
  }
}
// the R rows of a folded table F[(e * 2^rl + high) * M + lo] (fold_table_kernel), tp = &F[high * M + lo], stride = 2^rl * M
template <int R>
__device__ __forceinline__ void load_folded(gl_t (&t)[R], const gl_t *tp, size_t stride) {
#pragma unroll
  for (int e = 0; e < R; e++) {
    t[e] = *tp;
    tp += stride;
  }
}

// one round: layers on tile bits [beta0, beta0 + LOGR); the group twiddle of position j is
// theta^(bitrev(j)), theta = w_{2^(s0+LOGR)}^(lo), read from the packed table T[(e-1)*M + lo].
// MUL = (s0 > 0): the round has general twiddles (the first round of a transform has none).
template <int DIT, bool INV, int LOGR, bool MUL>
__device__ __forceinline__ void round_regs(gl_t *lds, const PassArgs &A, uint32_t TB, uint32_t beta0, uint32_t lo0,
                                           const gl_t *tw) {
  constexpr int R = 1 << LOGR;
  const uint32_t ngroups = 1u << (TB - LOGR);
  const uint32_t s0 = beta0 - A.tb + A.s;  // log2 M
  // Index arithmetic is a tenth of this kernel's instructions if done per access: the swizzled LDS index of element
  // base | (j << beta0) is pidx(base) ^ pidx(j << beta0) (the swizzle is GF(2)-linear), the second term wave-uniform;
  // the packed twiddle table is walked with one 64-bit add per entry.
  uint32_t lj[R];
#pragma unroll
  for (int j = 0; j < R; j++) lj[j] = pidx((uint32_t)j << beta0);
  const size_t tstride = (size_t)1 << s0;
  for (uint32_t g = threadIdx.x; g < ngroups; g += blockDim.x) {
    const uint32_t low = g & ((1u << beta0) - 1), high = g >> beta0;
    const uint32_t base = (high << (beta0 + LOGR)) | low;
    const uint32_t lo = (((base & ((1u << beta0) - 1)) >> A.tb) << A.s) + lo0 + (base & ((1u << A.tb) - 1));
    gl_t v[R];
    uint32_t li[R];
    {
      const uint32_t l0 = pidx(base);
#pragma unroll
      for (int j = 0; j < R; j++) li[j] = l0 ^ lj[j];
    }
#pragma unroll
    for (int j = 0; j < R; j++) v[j] = lds[li[j]];
    gl_t t[R];
    if constexpr (MUL) load_packed(t, tw + lo, tstride);
    if constexpr (DIT && MUL) {
      static_for<1, R>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        v[j] = gl_mul(v[j], t[brev_c(j, LOGR)]);
      });
    }
    dft_regs<LOGR, DIT, INV>(v);
    if constexpr (!DIT && MUL) {
      static_for<1, R>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        v[j] = gl_mul(v[j], t[brev_c(j, LOGR)]);
      });
    }
#pragma unroll
    for (int j = 0; j < R; j++) lds[li[j]] = v[j];
  }
}

template <int DIT, bool INV>
__device__ __forceinline__ void do_round(gl_t *lds, const PassArgs &A, uint32_t TB, uint32_t beta0, uint32_t logr,
                                         uint32_t lo0, const gl_t *tw) {
  const bool mul = beta0 - A.tb + A.s > 0;
#define P2_ROUND(L)                                                        \
  do {                                                                     \
    if (mul) round_regs<DIT, INV, L, true>(lds, A, TB, beta0, lo0, tw);    \
    else round_regs<DIT, INV, L, false>(lds, A, TB, beta0, lo0, tw);       \
  } while (0)
  switch (logr) {
  case 3: P2_ROUND(3); break;
  case 2: P2_ROUND(2); break;
  default: P2_ROUND(1); break;
  }
#undef P2_ROUND
}

// One tile of one pass: global -> LDS (XOR-swizzled), the pass's rounds, LDS -> global.
// TBC = 12: the full 2^12-element tile with NTT_THREADS lanes -- the global loads/stores of a lane are NTT_PER
// independent accesses issued back to back (compile-time trip count) so their latencies overlap;
// TBC = 0: any smaller tile (small transforms), runtime loops.
template <int DIT, bool INV, int TBC>
__device__ __forceinline__ void tile_body(gl_t *lds, const PassArgs &A, uint32_t tile, uint32_t col, uint32_t coset) {
  static_assert(TBC == 0 || TBC == NTT_TILE_BITS, "a full tile or a runtime-sized smaller one");
  constexpr int PER = NTT_PER, NT = NTT_THREADS;
  const uint32_t TB = TBC ? TBC : A.a + A.tb;
  const auto [hi_base, lo0] = tile_pos(A, tile);
  const auto [src, dst, scale] = col_ptrs(A, col, coset);
  const uint32_t tsize = 1u << TB;
  // lane e + i * NT of the tile: when a contiguous run (2^tb elements) divides NT, the global index is linear in i
  // (g0 + i * gstep) and so is the swizzled LDS index (l0 + i * NT: the swizzle only touches bits below log2 NT)
  const bool glin = (1u << A.tb) <= (uint32_t)NT;
  const uint32_t g0 = gidx(threadIdx.x, hi_base, lo0, A.s, A.tb), gstep = (NT >> (glin ? A.tb : 0)) << A.s;
  const uint32_t l0 = pidx(threadIdx.x);
  if constexpr (TBC != 0) {
    gl_t x[PER];
    uint32_t g[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
      g[i] = glin ? g0 + (uint32_t)i * gstep : gidx(threadIdx.x + i * NT, hi_base, lo0, A.s, A.tb);
      x[i] = src[g[i]];
    }
    if (scale) {
      gl_t sc[PER];
#pragma unroll
      for (int i = 0; i < PER; i++) sc[i] = scale[g[i]];
#pragma unroll
      for (int i = 0; i < PER; i++) x[i] = gl_mul(x[i], sc[i]);
    }
#pragma unroll
    for (int i = 0; i < PER; i++) lds[l0 + (uint32_t)i * NT] = x[i];
  } else {
    for (uint32_t e = threadIdx.x; e < tsize; e += blockDim.x) {
      const uint32_t g = gidx(e, hi_base, lo0, A.s, A.tb);
      gl_t x = src[g];
      if (scale) x = gl_mul(x, scale[g]);
      lds[pidx(e)] = x;
    }
  }
  __syncthreads();
  // A radix-8 round on tile bits [beta, beta + 3) below bit 9 of a full tile touches, in wave w, exactly the elements
  // whose bits [9, 12) are w (lane g = 64 w + l holds base = (g >> beta << (beta + 3)) | (g & (2^beta - 1)) and its 8
  // strides): consecutive such rounds exchange data inside a wave only, and a wave's LDS operations execute in order --
  // no workgroup barrier between them.
  // That argument needs: 512 lanes in wave64 (wave w = lanes [64 w, 64 w + 64)), ONE group per lane (g == threadIdx.x: the
  // trip count of round_regs' loop is 1) and round_regs' base = (g >> beta << (beta + 3)) | low split -- tied down here so that
  // an edit to any of them fails to compile instead of racing on LDS.
  static_assert(NTT_PER == 8 && NTT_THREADS == 512, "wave-private rounds: one radix-8 group per lane of a 2^12 tile");
#if defined(__HIP_DEVICE_COMPILE__) && !defined(__gfx950__)
#error "wave-private rounds assume wave64: gfx950 (CDNA has no wave32 mode) is the only target of this file"
#endif
  const bool one_group_per_lane = (1u << (TB - 3)) == blockDim.x;
  auto wave_private = [&](uint32_t beta, uint32_t r) { return TBC == NTT_TILE_BITS && one_group_per_lane && r == 3 && beta + 3 <= 9; };
  if (DIT) {
    uint32_t beta = A.tb;
    for (uint32_t i = 0; i < A.nrounds; i++) {
      do_round<1, INV>(lds, A, TB, beta, A.r[i], lo0, A.ptw + A.tw_off[i]);
      if (i + 1 < A.nrounds && wave_private(beta, A.r[i]) && wave_private(beta + A.r[i], A.r[i + 1])) asm volatile("" ::: "memory");
      else __syncthreads();
      beta += A.r[i];
    }
  } else {
    uint32_t beta = A.tb + A.a;
    for (uint32_t i = A.nrounds; i-- > 0;) {
      beta -= A.r[i];
      do_round<0, INV>(lds, A, TB, beta, A.r[i], lo0, A.ptw + A.tw_off[i]);
      if (i > 0 && wave_private(beta, A.r[i]) && wave_private(beta - A.r[i - 1], A.r[i - 1])) asm volatile("" ::: "memory");
      else __syncthreads();
    }
  }
  const bool post = A.post != 1;
  if constexpr (TBC != 0) {
    gl_t x[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) x[i] = lds[l0 + (uint32_t)i * NT];
    if (post) {
#pragma unroll
      for (int i = 0; i < PER; i++) x[i] = gl_mul(x[i], A.post);
    }
#pragma unroll
    for (int i = 0; i < PER; i++) dst[glin ? g0 + (uint32_t)i * gstep : gidx(threadIdx.x + i * NT, hi_base, lo0, A.s, A.tb)] = x[i];
  } else {
    for (uint32_t e = threadIdx.x; e < tsize; e += blockDim.x) {
      gl_t x = lds[pidx(e)];
      if (post) x = gl_mul(x, A.post);
      dst[gidx(e, hi_base, lo0, A.s, A.tb)] = x;
    }
  }
}

// One pass as its own launch: every size, every round from the packed tables.  The only form of the transforms below 2^12 points
// and of strided passes of 1, 2 or 4 layers; with P2GPU_NTT_DIRECT=0 of every pass.
template <int DIT, bool INV, int TBC>
__global__ __launch_bounds__(TBC ? NTT_THREADS : 256, TBC ? NTT_MIN_WAVES : 1) void ntt_pass_kernel(PassArgs A) {
  extern __shared__ gl_t lds[];
  uint32_t tile, col, coset;
  if (!pass_unit(A, tile, col, coset)) return;
  tile_body<DIT, INV, TBC>(lds, A, tile, col, coset);
}

// ---- direct passes: coefficients -> values (DIT) ---------------------------------------------------------------------------------
// Those transforms are DIT passes on full 2^12 tiles.  ntt_pass_kernel above stages a tile in
// LDS, runs every round LDS -> registers -> LDS with a table twiddle on 7 of 8 inputs, and copies the tile out: five LDS round
// trips and three barriers for the 12-layer pass, three and three for the 5-layer one.  Two observations remove a third of that:
//   * The LAST round of a pass holds, in lane t, exactly the elements t | (j << beta) that lane t would copy to global memory
//     afterwards, and (strided passes) the FIRST round's elements base | (j << tb) are what a coalesced load hands a lane: the
//     first round runs straight from global memory, the last one stores straight to it.
//   * The twiddle of the last round is w_{2^(s0 + r)}^(lo * brev(j)) with lo = lo' + 2^s0' * k, k the OUTPUT index of the round
//     before: w^(lo' * brev(j)) is constant over that earlier round's butterfly group (fixed lo', fixed j = its `high` bits), so
//     it is multiplied into that round's input twiddles (one folded table: fold_table_kernel), and what is left,
//     w_{2^(r' + r)}^(k * brev(j)), is a power of w_64 = 2^3 -- a SHIFT -- with k uniform over the wave (k sits in bits >= 6 of the
//     lane's group index): a scalar branch on k, then compile-time shift amounts.
// Same values (the field result of a butterfly network does not depend on how its twiddles are factored): bit-exact against the
// oracle and against ntt_pass_kernel (P2GPU_NTT_DIRECT=0).  The 12-layer first pass goes further (ntt_dit_head2_kernel below).
// the shift twiddles of a last round of RL layers after a round of RP layers: register j *= w_{2^(RP+RL)}^(k * brev(j))
template <bool INV, int RL, int RP, int K>
__device__ __forceinline__ void shift_twiddles(gl_t (&v)[1 << RL]) {
  constexpr int UNIT = 192 >> (RP + RL);
  static_for<1, (1 << RL)>([&](auto jc) {
    constexpr int j = decltype(jc)::value;
    constexpr int e0 = (UNIT * K * brev_c(j, RL)) % 192;
    constexpr int e = INV ? (192 - e0) % 192 : e0;
    v[j] = mul_pow2_any<e>(v[j]);
  });
}
template <bool INV, int RL, int RP>
__device__ __forceinline__ void shift_twiddles_k(gl_t (&v)[1 << RL], uint32_t k) {
  static_assert(RP == 2 || RP == 3, "round before the last: two or three layers");
  switch (__builtin_amdgcn_readfirstlane(k)) {  // k is wave-uniform: a scalar branch
  case 0: break;
  case 1: shift_twiddles<INV, RL, RP, 1>(v); break;
  case 2: shift_twiddles<INV, RL, RP, 2>(v); break;
  case 3: shift_twiddles<INV, RL, RP, 3>(v); break;
  case 4: if constexpr (RP == 3) shift_twiddles<INV, RL, RP, 4>(v); break;
  case 5: if constexpr (RP == 3) shift_twiddles<INV, RL, RP, 5>(v); break;
  case 6: if constexpr (RP == 3) shift_twiddles<INV, RL, RP, 6>(v); break;
  default: if constexpr (RP == 3) shift_twiddles<INV, RL, RP, 7>(v); break;
  }
}
// A round on tile bits [beta0, beta0 + LOGR) of a 2^12 tile in LDS whose input twiddles also carry the general part of the LAST
// round's (RL layers, the tile's top bits = this round's `high`): table row e = brev(j), then high, then lo.
// DIF: the same table multiplies the round's OUTPUTS (its own general twiddle x the top round's deferred part).
template <int DIT, bool INV, int LOGR>
__device__ __forceinline__ void round_folded(gl_t *lds, const PassArgs &A, uint32_t beta0, uint32_t rl, uint32_t lo0, const gl_t *ftw) {
  constexpr int R = 1 << LOGR;
  const uint32_t ngroups = 1u << (12 - LOGR);
  const uint32_t s0 = beta0 - A.tb + A.s;
  uint32_t lj[R];
#pragma unroll
  for (int j = 0; j < R; j++) lj[j] = pidx((uint32_t)j << beta0);
  const size_t estride = (size_t)1 << (s0 + rl);
  for (uint32_t g = threadIdx.x; g < ngroups; g += NTT_THREADS) {
    const uint32_t low = g & ((1u << beta0) - 1), high = g >> beta0;
    const uint32_t base = (high << (beta0 + LOGR)) | low;
    const uint32_t lo = ((low >> A.tb) << A.s) + lo0 + (low & ((1u << A.tb) - 1));
    gl_t v[R], t[R];
    uint32_t li[R];
    const uint32_t l0 = pidx(base);
#pragma unroll
    for (int j = 0; j < R; j++) li[j] = l0 ^ lj[j];
#pragma unroll
    for (int j = 0; j < R; j++) v[j] = lds[li[j]];
    load_folded(t, ftw + ((size_t)high << s0) + lo, estride);
    if constexpr (DIT) {
      static_for<0, R>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        v[j] = gl_mul(v[j], t[brev_c(j, LOGR)]);
      });
    }
    dft_regs<LOGR, DIT, INV>(v);
    if constexpr (!DIT) {
      static_for<0, R>([&](auto jc) {
        constexpr int j = decltype(jc)::value;
        v[j] = gl_mul(v[j], t[brev_c(j, LOGR)]);
      });
    }
#pragma unroll
    for (int j = 0; j < R; j++) lds[li[j]] = v[j];
  }
}
// Second swizzle, for the head pass whose first round runs in registers (ntt_dit_head2_kernel): its LDS accesses differ, within a
// lane group, in element bits {3,4,5,6} (16-lane store groups after round 0), {6..10} / {6..9} (round on bits 3-5, wave = bits 0-2),
// {3,4,5,9,10} / {3,4,5,9} (round on bits 6-8) and {0..4} (last round): slot bits s0 = e0^e3^e6, s1 = e1^e4^e7, s2 = e2^e5^e8,
// s3 = e3^e9, s4 = e4^e10 have full rank on each of them (found by exhaustive search over shift-and-mask forms: the only two-term
// one).  GF(2)-linear like pidx: pidx2(a ^ b) = pidx2(a) ^ pidx2(b).
__device__ __forceinline__ constexpr uint32_t pidx2(uint32_t e) { return e ^ ((e >> 3) & 7u) ^ ((e >> 6) & 31u); }
// The last round of a pass, LDS -> registers -> global: RL layers on the tile's top bits, shift twiddles (the round before had RP
// layers; its folded table carried the rest), then the pass's output scale.
template <bool INV, int RL, int RP, int SW = 0>
__device__ __forceinline__ void round_to_global(const gl_t *lds, gl_t *dst, const PassArgs &A, uint32_t hi_base, uint32_t lo0) {
  constexpr int R = 1 << RL;
  constexpr uint32_t beta0 = 12 - RL;
  auto sw = [](uint32_t e) { return SW ? pidx2(e) : pidx(e); };
  uint32_t lj[R];
#pragma unroll
  for (int j = 0; j < R; j++) lj[j] = sw((uint32_t)j << beta0);
  const bool post = A.post != 1;
#pragma unroll
  for (uint32_t it = 0; it < ((1u << beta0) / NTT_THREADS); it++) {
    const uint32_t g = threadIdx.x + it * NTT_THREADS;
    gl_t v[R];
    const uint32_t l0 = sw(g);
#pragma unroll
    for (int j = 0; j < R; j++) v[j] = lds[l0 ^ lj[j]];
    shift_twiddles_k<INV, RL, RP>(v, (g >> (beta0 - RP)) & ((1u << RP) - 1));
    dft_regs<RL, 1, INV>(v);
    if (post) {
#pragma unroll
      for (int j = 0; j < R; j++) v[j] = gl_mul(v[j], A.post);
    }
    const uint32_t a0 = hi_base + ((g >> A.tb) << A.s) + lo0 + (g & ((1u << A.tb) - 1));
#pragma unroll
    for (int j = 0; j < R; j++) dst[a0 + ((uint32_t)j << (beta0 - A.tb + A.s))] = v[j];
  }
}
// The 12-layer first pass of a DIT transform of >= 2^12 points (s = 0, tb = 0: contiguous tiles), three LDS round trips and two
// barriers.  Its FIRST round runs in registers: a lane loads 8 CONSECUTIVE words (64 B: the round on bits 0-2 is then its own eight
// registers; a wave still covers 4 KB contiguous), scales them by the coset scale, runs the twiddle-free 8-point transform and only
// then stores to LDS.  The second round is on shifts (w_64 = 2^3, so the 64-point transform on tile bits 0-5 needs no table): the
// round on bits 3-5 multiplies input j by w_64^(k1 brev(j)), k1 = element bits 0-2: made WAVE-uniform by giving wave w the groups
// with k1 = w (lane = bits 6-11), so the eight shift amounts are compile-time behind one scalar branch; the round on bits 6-8
// (folded table, laid out in this kernel's lane order: head_fold_table_kernel) keeps wave <-> k1 and therefore needs no barrier in
// between (a wave's LDS operations execute in order, see wave_private in tile_body); then the last round -> global
// (round_to_global).  One general product per element besides the coset scale.  LDS addresses through pidx2 (every access
// conflict-free).
template <bool INV>
__global__ __launch_bounds__(NTT_THREADS, NTT_MIN_WAVES) void ntt_dit_head2_kernel(PassArgs A) {
  extern __shared__ gl_t lds[];
  uint32_t tile, col, coset;
  if (!pass_unit(A, tile, col, coset)) return;
  const auto [src, dst, scale] = col_ptrs(A, col, coset);
  const uint32_t tbase = tile << 12, t = threadIdx.x, w = t >> 6, l = t & 63u;
  gl_t v[8];
  {
    const ulonglong2 *s2 = reinterpret_cast<const ulonglong2 *>(src + tbase + 8 * t);  // (columns and tiles are 64 B aligned)
    ulonglong2 x2[4];
#pragma unroll
    for (int i = 0; i < 4; i++) x2[i] = s2[i];
    if (scale) {
      const ulonglong2 *c2 = reinterpret_cast<const ulonglong2 *>(scale + tbase + 8 * t);
      ulonglong2 sc[4];
#pragma unroll
      for (int i = 0; i < 4; i++) sc[i] = c2[i];
#pragma unroll
      for (int i = 0; i < 4; i++) {
        v[2 * i] = gl_mul(x2[i].x, sc[i].x);
        v[2 * i + 1] = gl_mul(x2[i].y, sc[i].y);
      }
    } else {
#pragma unroll
      for (int i = 0; i < 4; i++) {
        v[2 * i] = x2[i].x;
        v[2 * i + 1] = x2[i].y;
      }
    }
  }
  dft_regs<3, 1, INV>(v);  // bits 0-2: no twiddles
  {
    const uint32_t p0 = pidx2(8 * t);  // pidx2(k) = k for k < 8
#pragma unroll
    for (int k = 0; k < 8; k++) lds[p0 ^ (uint32_t)k] = v[k];
  }
  __syncthreads();
  {  // bits 3-5: element = w + 8 j + 64 l
    const uint32_t p0 = pidx2(w | (l << 6));
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = lds[p0 ^ pidx2((uint32_t)j << 3)];
    shift_twiddles_k<INV, 3, 3>(v, w);
    dft_regs<3, 1, INV>(v);
#pragma unroll
    for (int j = 0; j < 8; j++) lds[p0 ^ pidx2((uint32_t)j << 3)] = v[j];
  }
  asm volatile("" ::: "memory");  // the same wave, the same 512 elements (bits 0-2 = w): in-order LDS operations, no barrier
  {  // bits 6-8: element = w + 8 a + 64 i + 512 J, lane = a + 8 J; twiddles F2[e * 512 + t]
    const uint32_t p0 = pidx2(w | ((l & 7u) << 3) | ((l >> 3) << 9));
    gl_t tw[8];
    const gl_t *tp = A.ftw2 + t;
#pragma unroll
    for (int e = 0; e < 8; e++) tw[e] = tp[e * NTT_THREADS];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = lds[p0 ^ pidx2((uint32_t)i << 6)];
    static_for<0, 8>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      v[j] = gl_mul(v[j], tw[brev_c(j, 3)]);
    });
    dft_regs<3, 1, INV>(v);
#pragma unroll
    for (int i = 0; i < 8; i++) lds[p0 ^ pidx2((uint32_t)i << 6)] = v[i];
  }
  __syncthreads();
  round_to_global<INV, 3, 3, 1>(lds, dst, A, tbase, 0);
}
// A strided DIT pass of a = 3 + RM + RL layers (RM = 0: no middle round; RL = 0: a = 3, no LDS at all) on 2^12-element tiles of
// 2^a rows x 2^tb contiguous words: first round global -> registers (its 8 elements are the rows base + j: one coalesced
// load each), [middle round in LDS,] last round -> global.  The round before the last uses the folded table.
template <bool INV, int RM, int RL>
__global__ __launch_bounds__(NTT_THREADS, NTT_MIN_WAVES) void ntt_dit_strided_kernel(PassArgs A) {
  extern __shared__ gl_t lds[];
  uint32_t tile, col, coset;
  if (!pass_unit(A, tile, col, coset)) return;
  const auto [src, dst, scale] = col_ptrs(A, col, coset);
  const auto [hi_base, lo0] = tile_pos(A, tile);
  {
    // first round: group g = lane; low = its tb contiguous bits, high = the tile bits above the round
    const uint32_t g = threadIdx.x, low = g & ((1u << A.tb) - 1), high = g >> A.tb;
    const uint32_t base = (high << (A.tb + 3)) | low;
    const uint32_t a0 = hi_base + ((high << 3) << A.s) + lo0 + low, lo = lo0 + low;
    gl_t v[8], t[8];
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = src[a0 + ((uint32_t)j << A.s)];
    constexpr bool FOLD1 = RM == 0 && RL != 0;  // the first round is the one before the last
    if constexpr (FOLD1) load_folded(t, A.ftw + ((size_t)high << A.s) + lo, (size_t)1 << (A.s + RL));
    else load_packed(t, A.ptw + A.tw_off[0] + lo, (size_t)1 << A.s);
    static_for<(FOLD1 ? 0 : 1), 8>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      v[j] = gl_mul(v[j], t[brev_c(j, 3)]);
    });
    dft_regs<3, 1, INV>(v);
    if constexpr (RL == 0) {
      if (A.post != 1) {
#pragma unroll
        for (int j = 0; j < 8; j++) v[j] = gl_mul(v[j], A.post);
      }
#pragma unroll
      for (int j = 0; j < 8; j++) dst[a0 + ((uint32_t)j << A.s)] = v[j];
      return;
    } else {
      const uint32_t l0 = pidx(base);
#pragma unroll
      for (int j = 0; j < 8; j++) lds[l0 ^ pidx((uint32_t)j << A.tb)] = v[j];
    }
  }
  if constexpr (RL != 0) {
    __syncthreads();
    if constexpr (RM != 0) {
      round_folded<1, INV, RM>(lds, A, A.tb + 3, RL, lo0, A.ftw);
      __syncthreads();
    }
    round_to_global<INV, RL, (RM != 0 ? RM : 3)>(lds, dst, A, hi_base, lo0);
  }
}

// ---- the mirror images: values -> coefficients (DIF) ----------------------------------------------------------------------------
// A DIF round multiplies its OUTPUTS: after the round on [beta, beta + r) output j takes w^-(lo brev(j)), lo = the element's bits
// below beta.  For the pass's FIRST (top) round lo = lo' + 2^s0' k with k the INPUT index of the round below: w^-(2^s0' k brev(j)) is a
// power of w_64 -- a shift, k wave-uniform -- applied at once, and w^-(lo' brev(j)) is constant over the group of the round below
// (fixed lo', j = its `high`), so that round's output twiddles carry it (the same folded table, inverse root).  First round from
// global memory, last round to it.
template <bool INV, int RL, int RP, int SW = 0>
__device__ __forceinline__ void round_from_global(const gl_t *src, gl_t *lds, const PassArgs &A, uint32_t hi_base, uint32_t lo0) {
  constexpr int R = 1 << RL;
  constexpr uint32_t beta0 = 12 - RL;
  auto sw = [](uint32_t e) { return SW ? pidx2(e) : pidx(e); };
#pragma unroll
  for (uint32_t it = 0; it < ((1u << beta0) / NTT_THREADS); it++) {
    const uint32_t g = threadIdx.x + it * NTT_THREADS;
    const uint32_t a0 = hi_base + ((g >> A.tb) << A.s) + lo0 + (g & ((1u << A.tb) - 1));
    gl_t v[R];
#pragma unroll
    for (int j = 0; j < R; j++) v[j] = src[a0 + ((uint32_t)j << (beta0 - A.tb + A.s))];
    dft_regs<RL, 0, INV>(v);
    shift_twiddles_k<INV, RL, RP>(v, (g >> (beta0 - RP)) & ((1u << RP) - 1));
    const uint32_t l0 = sw(g);
#pragma unroll
    for (int j = 0; j < R; j++) lds[l0 ^ sw((uint32_t)j << beta0)] = v[j];
  }
}
// A strided DIF pass of a = 3 + RM + RL layers: top round (RL layers) global -> registers -> LDS with shift twiddles, [middle round
// in LDS with the folded table,] bottom round (3 layers) LDS -> registers -> global.  RL = 0: a = 3, one round, no LDS.
template <bool INV, int RM, int RL>
__global__ __launch_bounds__(NTT_THREADS, NTT_MIN_WAVES) void ntt_dif_strided_kernel(PassArgs A) {
  extern __shared__ gl_t lds[];
  uint32_t tile, col, coset;
  if (!pass_unit(A, tile, col, coset)) return;
  const auto [src, dst, scale] = col_ptrs(A, col, coset);
  const auto [hi_base, lo0] = tile_pos(A, tile);
  if constexpr (RL != 0) {
    round_from_global<INV, RL, (RM != 0 ? RM : 3)>(src, lds, A, hi_base, lo0);
    __syncthreads();
    if constexpr (RM != 0) {
      round_folded<0, INV, RM>(lds, A, A.tb + 3, RL, lo0, A.ftw);
      __syncthreads();
    }
  }
  {
    // bottom round: group g = lane; low = its tb contiguous bits, high = the tile bits above the round
    const uint32_t g = threadIdx.x, low = g & ((1u << A.tb) - 1), high = g >> A.tb;
    const uint32_t base = (high << (A.tb + 3)) | low;
    const uint32_t a0 = hi_base + ((high << 3) << A.s) + lo0 + low, lo = lo0 + low;
    gl_t v[8], t[8];
    if constexpr (RL == 0) {
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = src[a0 + ((uint32_t)j << A.s)];
    } else {
      const uint32_t l0 = pidx(base);
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = lds[l0 ^ pidx((uint32_t)j << A.tb)];
    }
    constexpr bool FOLD1 = RM == 0 && RL != 0;  // the bottom round is the one below the top
    if constexpr (FOLD1) load_folded(t, A.ftw + ((size_t)high << A.s) + lo, (size_t)1 << (A.s + RL));
    else load_packed(t, A.ptw + A.tw_off[0] + lo, (size_t)1 << A.s);
    dft_regs<3, 0, INV>(v);
    static_for<(FOLD1 ? 0 : 1), 8>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      v[j] = gl_mul(v[j], t[brev_c(j, 3)]);
    });
    if (A.post != 1) {
#pragma unroll
      for (int j = 0; j < 8; j++) v[j] = gl_mul(v[j], A.post);
    }
#pragma unroll
    for (int j = 0; j < 8; j++) dst[a0 + ((uint32_t)j << A.s)] = v[j];
  }
}
// The 12-layer LAST pass of a DIF transform (contiguous tiles), the mirror of ntt_dit_head2_kernel: round on bits 9-11 from a
// coalesced load with shift twiddles -> LDS | rounds on bits 6-8 (folded table) and 3-5 (shifts) with wave = element bits 0-2, no
// barrier between them | round on bits 0-2 in registers, output scale, 64 B per lane to global.
template <bool INV>
__global__ __launch_bounds__(NTT_THREADS, NTT_MIN_WAVES) void ntt_dif_tail2_kernel(PassArgs A) {
  extern __shared__ gl_t lds[];
  uint32_t tile, col, coset;
  if (!pass_unit(A, tile, col, coset)) return;
  const auto [src, dst, scale] = col_ptrs(A, col, coset);
  const uint32_t tbase = tile << 12, t = threadIdx.x, w = t >> 6, l = t & 63u;
  round_from_global<INV, 3, 3, 1>(src, lds, A, tbase, 0);
  __syncthreads();
  gl_t v[8];
  {  // bits 6-8: element = w + 8 a + 64 i + 512 J, lane = a + 8 J; output twiddles F2[e * 512 + t]
    const uint32_t p0 = pidx2(w | ((l & 7u) << 3) | ((l >> 3) << 9));
    gl_t tw[8];
    const gl_t *tp = A.ftw2 + t;
#pragma unroll
    for (int e = 0; e < 8; e++) tw[e] = tp[e * NTT_THREADS];
#pragma unroll
    for (int i = 0; i < 8; i++) v[i] = lds[p0 ^ pidx2((uint32_t)i << 6)];
    dft_regs<3, 0, INV>(v);
    static_for<0, 8>([&](auto jc) {
      constexpr int j = decltype(jc)::value;
      v[j] = gl_mul(v[j], tw[brev_c(j, 3)]);
    });
#pragma unroll
    for (int i = 0; i < 8; i++) lds[p0 ^ pidx2((uint32_t)i << 6)] = v[i];
  }
  asm volatile("" ::: "memory");  // the same wave, the same 512 elements (bits 0-2 = w)
  {  // bits 3-5: element = w + 8 j + 64 l; output j takes w_64^-(w brev(j))
    const uint32_t p0 = pidx2(w | (l << 6));
#pragma unroll
    for (int j = 0; j < 8; j++) v[j] = lds[p0 ^ pidx2((uint32_t)j << 3)];
    dft_regs<3, 0, INV>(v);
    shift_twiddles_k<INV, 3, 3>(v, w);
#pragma unroll
    for (int j = 0; j < 8; j++) lds[p0 ^ pidx2((uint32_t)j << 3)] = v[j];
  }
  __syncthreads();
  {
    const uint32_t p0 = pidx2(8 * t);
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = lds[p0 ^ (uint32_t)k];
  }
  dft_regs<3, 0, INV>(v);  // bits 0-2: no twiddles
  if (A.post != 1) {
#pragma unroll
    for (int k = 0; k < 8; k++) v[k] = gl_mul(v[k], A.post);
  }
  ulonglong2 *d2 = reinterpret_cast<ulonglong2 *>(dst + tbase + 8 * t);
#pragma unroll
  for (int i = 0; i < 4; i++) d2[i] = make_ulonglong2(v[2 * i], v[2 * i + 1]);
}

// ---- plan -----------------------------------------------------------------------
// packed twiddles of one round: T[(e-1) * M + lo] = root_n^((lo * e) << (d - s0 - r)), e in [1, 2^r)
__global__ void round_table_kernel(gl_t *out, gl_t root_n, uint32_t d, uint32_t s0, uint32_t r) {
  const uint32_t M = 1u << s0, cnt = ((1u << r) - 1) * M;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t e = i / M + 1, lo = i % M;
  out[i] = gl_pow(root_n, ((uint64_t)lo * e) << (d - s0 - r));
}

// folded twiddles of a round of r layers at s0 whose inputs also take the general part of the next (last, rl layers) round's:
// F[(e * 2^rl + J) * M + lo] = w_{2^(s0+r)}^(lo e) * w_{2^(s0+r+rl)}^(lo brev_rl(J)), M = 2^s0, e < 2^r, J < 2^rl
__global__ void fold_table_kernel(gl_t *out, gl_t root_n, uint32_t d, uint32_t s0, uint32_t r, uint32_t rl) {
  const uint32_t M = 1u << s0, cnt = (1u << (r + rl)) * M;
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= cnt) return;
  const uint32_t lo = i % M, J = (i / M) & ((1u << rl) - 1), e = i >> (s0 + rl);
  const uint64_t ex = (((uint64_t)lo * e) << (d - s0 - r)) + (((uint64_t)lo * bitrev32(J, rl)) << (d - s0 - r - rl));
  out[i] = gl_pow(root_n, ex);
}
// the head pass's folded table (s0 = 6, r = 3, rl = 3) in the lane order of ntt_dit_head2_kernel: F2[e * 512 + t] for lane t whose
// group is lo = (t >> 6) + 8 (t & 7), J = (t & 63) >> 3
__global__ void head_fold_table_kernel(gl_t *out, gl_t root_n, uint32_t d) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= 8u * 512u) return;
  const uint32_t e = i >> 9, t = i & 511u, lo = (t >> 6) + 8u * (t & 7u), J = (t & 63u) >> 3;
  const uint64_t ex = (((uint64_t)lo * e) << (d - 9)) + (((uint64_t)lo * bitrev32(J, 3)) << (d - 12));
  out[i] = gl_pow(root_n, ex);
}
// The whole transform of the structured columns of a batch (ColHints): class 0 -> zeros (not even stored when the
// column's clean mark says dst holds them already), class 1 -> val[c] * basis.  One lane per 2 elements, coalesced;
// blocks of dense columns return at once.  By linearity these are the canonical values the butterfly network
// would produce.
__global__ __launch_bounds__(256) void structured_fill_kernel(gl_t *dst, uint32_t d, uint32_t col_stride, uint32_t cosets,
                                                              ColHints h, uint32_t coset_first, uint32_t coset_stride) {
  const uint32_t col = blockIdx.y;
  const uint32_t cls = h.cls[col];
  if (cls == 2u) return;
  if (cls < 2u && col >= h.virt_first) return;  // never read from memory: the leaf hash and the query gather recompute it
  if (cls == 0u && h.clean != nullptr && h.clean[col] != 0u) return;
  const size_t n = (size_t)1 << d;
  const size_t step = (size_t)gridDim.x * blockDim.x;
  if (cls == 3u) {  // zero outside the special rows: the same linear combination of their unit columns' transforms
    gl_t v[MAX_SPARSE_ROWS];
#pragma unroll
    for (uint32_t s = 0; s < MAX_SPARSE_ROWS; s++) v[s] = s < h.nrows ? h.val[(size_t)s * h.val_stride + col] : (gl_t)0;
    for (uint32_t coset = 0; coset < cosets; coset++) {
      gl_t *out = dst + ((size_t)coset * col_stride + col) * n;
      const gl_t *bs = h.basis + (h.basis_per_coset ? (size_t)(coset_first + coset * coset_stride) * n : 0);
      for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) {
        Acc160 acc;
        acc.clear();
#pragma unroll
        for (uint32_t s = 0; s < MAX_SPARSE_ROWS; s++)
          if (s < h.nrows) acc.mac(v[s], bs[(size_t)s * h.basis_stride + i]);
        out[i] = acc.value();
      }
    }
    return;
  }
  const gl_t v = cls == 1u ? h.val[col] : 0;
  for (uint32_t coset = 0; coset < cosets; coset++) {  // one block covers its slice of every coset: 8x fewer blocks to retire
    gl_t *out = dst + ((size_t)coset * col_stride + col) * n;
    const gl_t *bs = h.basis + (h.basis_per_coset ? (size_t)(coset_first + coset * coset_stride) * n : 0);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += step) out[i] = cls == 1u ? gl_mul(v, bs[i]) : (gl_t)0;
  }
}

namespace {

size_t lds_bytes(uint32_t TB) { return std::max<size_t>((size_t)1 << TB, 256) * sizeof(gl_t); }  // no padding: pidx() is a permutation of every 256-element block

// P2GPU_NTT_DIRECT=0: every pass through ntt_pass_kernel (A/B measurements, and the reference the direct kernels are tested against)
bool direct_on() {
  static const bool on = env_flag("P2GPU_NTT_DIRECT", true);
  return on;
}

// rounds of three layers; a remainder of one layer joins the round before it as 2 + 2 (a lone 1 only when a == 1)
void split_rounds(uint32_t a, std::vector<uint32_t> &r) {
  r.assign(a / 3, 3);
  if (a % 3 == 1 && a >= 4) {
    r.back() = 2;
    r.push_back(2);
  } else if (a % 3) {
    r.push_back(a % 3);
  }
}

// Does the pass have a direct kernel?  Full tiles whose first round has three layers: the 12-layer contiguous pass [3,3,3,3]
// (head / tail) and the strided passes [3], [3,2], [3,3], [3,2,2], [3,3,2], [3,3,3].
bool has_direct_form(const NttPass &ps) {
  return ps.a + ps.tb == NTT_TILE_BITS && ps.r[0] == 3 && (ps.s == 0 ? ps.a == 12 : (ps.a == 3 || (ps.a >= 5 && ps.a <= 9)));
}

void fill_pass_args(PassArgs &A, const NttPlan *plan, size_t i, const gl_t *src, gl_t *dst, uint32_t cols, uint32_t cosets,
                    const gl_t *scale, gl_t post, bool src_per_coset, CosetMap cm, uint32_t stride_all, const uint32_t *colnz) {
  const size_t np = plan->passes.size();
  const NttPass &ps = plan->passes[i];
  A.src = (i == 0) ? src : dst;
  A.dst = dst;
  A.ptw = plan->ptw;
  A.scale = (i == 0 && plan->dir == NttDir::ToValues) ? scale : nullptr;
  A.post = (i == np - 1) ? post : 1;
  A.d = plan->d;
  A.s = ps.s; A.a = ps.a; A.tb = ps.tb;
  A.cols = stride_all;  // column stride between cosets (a launch may cover a column chunk)
  A.src_single = (i == 0 && !src_per_coset) ? 1 : 0;
  A.coset_first = cm.first;
  A.coset_stride = cm.stride;
  A.nrounds = ps.nrounds;
  A.colnz = colnz;
  A.ftw = ps.direct && ps.s != 0 ? plan->ptw + ps.ftw_off : nullptr;
  A.ftw2 = ps.direct && ps.s == 0 ? plan->ptw + ps.ftw_off : nullptr;
  for (int k = 0; k < MAX_ROUNDS; k++) { A.r[k] = ps.r[k]; A.tw_off[k] = ps.tw_off[k]; }
  A.tiles = 1u << (plan->d - (A.a + A.tb));
  A.cols_grid = cols; A.cosets = cosets;
}

template <int DIT, bool INV>
void launch_generic(hipStream_t st, const PassArgs &A, dim3 grid, uint32_t TB, size_t lb) {
  if (TB == NTT_TILE_BITS) hipLaunchKernelGGL((ntt_pass_kernel<DIT, INV, NTT_TILE_BITS>), grid, dim3(NTT_THREADS), lb, st, A);
  else hipLaunchKernelGGL((ntt_pass_kernel<DIT, INV, 0>), grid, dim3(TB >= 8 ? 256 : 64), lb, st, A);
}

// (Both passes of a two-pass transform in ONE launch -- per-XCD work queues, the intermediate handed over through L2 -- was
// built, bit-exact, and measured slower and heavier on HBM than two launches: profiles/r04_lde_fused.md;
// `git show 33c653e:acvm-backend-plonky2_amd/csrc/ntt.hip` has it, and 891bf88 is the last commit with the NTT_EXP_* timing
// experiments and the radix-16 / 2^13-tile build knobs.)
// The names given to ProfScope are rocprofv3's demangled symbols, so the bench line and profiles/ agree; string literals: the
// profiler keeps the pointer.
void ntt_passes(hipStream_t st, const NttPlan *plan, const gl_t *src, gl_t *dst, uint32_t cols, uint32_t cosets,
                const gl_t *scale, gl_t post, bool src_per_coset, CosetMap cm, uint32_t stride_all, const uint32_t *colnz,
                uint32_t dense) {
  const uint32_t d = plan->d;
  const bool dit = plan->dir == NttDir::ToValues;
  for (size_t i = 0; i < plan->passes.size(); i++) {
    const NttPass &ps = plan->passes[i];
    PassArgs A;
    fill_pass_args(A, plan, i, src, dst, cols, cosets, scale, post, src_per_coset, cm, stride_all, colnz);
    const uint32_t TB = A.a + A.tb;
    dim3 grid((((A.tiles * cols + 7u) / 8u) * 8u) * cosets);
    // expected HBM bytes: every output element is written once; the input is read once per element, except
    // that the cosets of one (tile, column) share their source through one XCD's L2 (first LDE pass)
    // (structured columns are skipped by the kernels: `dense`, when the caller knows it, is what the launch really transforms)
    const double bytes = 8.0 * (double)(dense ? dense : cols) * ((size_t)1 << d) * (cosets + (A.src_single ? 1.0 : (double)cosets));
    const size_t lb = lds_bytes(TB);
    if (!(ps.direct && direct_on())) {
      ProfScope psx(dit ? (TB == NTT_TILE_BITS ? "ntt_pass_kernel<1, false, 12>" : "ntt_pass_kernel<1, false, 0>")
                        : (TB == NTT_TILE_BITS ? "ntt_pass_kernel<0, true, 12>" : "ntt_pass_kernel<0, true, 0>"), bytes);
      if (dit) launch_generic<1, false>(st, A, grid, TB, lb);
      else launch_generic<0, true>(st, A, grid, TB, lb);
    } else if (ps.s == 0) {
      ProfScope psd(dit ? "ntt_dit_head2_kernel<false>" : "ntt_dif_tail2_kernel<true>", bytes);
      if (dit) hipLaunchKernelGGL((ntt_dit_head2_kernel<false>), grid, dim3(NTT_THREADS), lb, st, A);
      else hipLaunchKernelGGL((ntt_dif_tail2_kernel<true>), grid, dim3(NTT_THREADS), lb, st, A);
    } else {
#define P2_STRIDED(RM, RL)                                                                                               \
  do {                                                                                                                   \
    ProfScope psd(dit ? "ntt_dit_strided_kernel<false, " #RM ", " #RL ">" : "ntt_dif_strided_kernel<true, " #RM ", " #RL ">", bytes); \
    if (dit) hipLaunchKernelGGL((ntt_dit_strided_kernel<false, RM, RL>), grid, dim3(NTT_THREADS), (RL) ? lb : 0, st, A);  \
    else hipLaunchKernelGGL((ntt_dif_strided_kernel<true, RM, RL>), grid, dim3(NTT_THREADS), (RL) ? lb : 0, st, A);       \
  } while (0)
      if (ps.rm == 0 && ps.rl == 0) P2_STRIDED(0, 0);
      else if (ps.rm == 0 && ps.rl == 2) P2_STRIDED(0, 2);
      else if (ps.rm == 0 && ps.rl == 3) P2_STRIDED(0, 3);
      else if (ps.rm == 2 && ps.rl == 2) P2_STRIDED(2, 2);
      else if (ps.rm == 3 && ps.rl == 2) P2_STRIDED(3, 2);
      else P2_STRIDED(3, 3);
#undef P2_STRIDED
    }
  }
}

}  // namespace

NttPlan *ntt_plan_create(hipStream_t st, uint32_t d, NttDir dir) {
  std::unique_ptr<NttPlan, decltype(&ntt_plan_destroy)> p(new NttPlan(), ntt_plan_destroy);
  p->d = d;
  p->dir = dir;
  const uint32_t TBMAX = NTT_TILE_BITS;
  const uint32_t b = d < TBMAX ? d : TBMAX;
  struct P { uint32_t s, a, tb; };
  std::vector<P> strided;
  {
    uint32_t rem = d - b, s = b;
    uint32_t npass = rem == 0 ? 0 : (rem <= 9 ? 1 : 2);
    for (uint32_t i = 0; i < npass; i++) {
      uint32_t a = (npass == 1) ? rem : (i == 0 ? (rem + 1) / 2 : rem / 2);
      uint32_t tb = TBMAX - a;
      if (tb > s) tb = s;
      strided.push_back(P{s, a, tb});
      s += a;
    }
  }
  std::vector<P> passes;
  if (dir == NttDir::ToValues) {
    passes.push_back(P{0, b, 0});
    for (auto &x : strided) passes.push_back(x);
  } else {
    for (size_t i = strided.size(); i-- > 0;) passes.push_back(strided[i]);
    passes.push_back(P{0, b, 0});
  }
  // table layout
  size_t total = 0;
  std::vector<uint32_t> rr;
  for (auto &ps : passes) {
    NttPass np;
    np.s = ps.s; np.a = ps.a; np.tb = ps.tb;
    split_rounds(ps.a, rr);
    np.nrounds = (uint32_t)rr.size();
    if (np.nrounds > (uint32_t)MAX_ROUNDS) return nullptr;  // (cannot happen: a <= 12 layers are four rounds)
    uint32_t beta = ps.tb;
    for (uint32_t i = 0; i < np.nrounds; i++) {
      np.r[i] = rr[i];
      np.tw_off[i] = (uint32_t)total;
      uint32_t s0 = beta - ps.tb + ps.s;
      if (s0 > 0) total += (size_t)((1u << rr[i]) - 1) << s0;
      if (i + 2 == np.nrounds) np.fold_s0 = s0;
      beta += rr[i];
    }
    np.direct = has_direct_form(np);
    if (np.direct && np.nrounds >= 2) {
      np.rm = np.nrounds == 3 ? np.r[1] : 0;
      np.rl = np.r[np.nrounds - 1];
      np.fold_r = np.r[np.nrounds - 2];
      np.ftw_off = (uint32_t)total;
      // (the 12-layer pass: 8 x 512 words in the lane order of ntt_dit_head2_kernel / ntt_dif_tail2_kernel)
      total += ps.s == 0 ? 4096 : (size_t)1 << (np.fold_r + np.rl + np.fold_s0);
    }
    p->passes.push_back(np);
  }
  p->table_len = total;
  if (total >> 32) return nullptr;  // tw_off / ftw_off are 32-bit word offsets (d = 24 with its folded tables: ~2^25 words)
  if (total) {
    if (hipMalloc((void **)&p->ptw, total * sizeof(gl_t)) != hipSuccess) return nullptr;
    gl_t root = gl_root(d);
    if (dir == NttDir::ToCoeffs) root = gl_inv(root);
    for (auto &np : p->passes) {
      uint32_t beta = np.tb;
      for (uint32_t i = 0; i < np.nrounds; i++) {
        uint32_t s0 = beta - np.tb + np.s;
        if (s0 > 0) {
          uint32_t cnt = ((1u << np.r[i]) - 1) << s0;
          hipLaunchKernelGGL(round_table_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, p->ptw + np.tw_off[i], root, d,
                             s0, np.r[i]);
        }
        beta += np.r[i];
      }
      if (np.direct && np.nrounds >= 2) {
        const uint32_t cnt = 1u << (np.fold_r + np.rl + np.fold_s0);
        if (np.s == 0) hipLaunchKernelGGL(head_fold_table_kernel, dim3(16), dim3(256), 0, st, p->ptw + np.ftw_off, root, d);
        else hipLaunchKernelGGL(fold_table_kernel, dim3((cnt + 255) / 256), dim3(256), 0, st, p->ptw + np.ftw_off, root, d, np.fold_s0, np.fold_r, np.rl);
      }
    }
  }
  return p.release();
}
void ntt_plan_destroy(NttPlan *p) {
  if (!p) return;
  if (p->ptw) (void)hipFree(p->ptw);
  delete p;
}

void ntt_batch(hipStream_t st, const NttPlan *plan, const gl_t *src, gl_t *dst, uint32_t cols, uint32_t cosets,
               const gl_t *scale, gl_t post, bool src_per_coset, CosetMap cm, uint32_t stride_cols, const ColHints *hints) {
  if (cols == 0) return;
  if (hints) {
    const size_t n = (size_t)1 << plan->d;
    const uint32_t bx = (uint32_t)std::max<size_t>(1, n / (256 * 4));
    // (profile bytes: the structured columns that are actually stored -- those below virt_first; with no dense count from an earlier
    // proof every column is counted)
    const uint32_t stored = hints->virt_first < cols ? hints->virt_first : cols;
    const uint32_t filled = hints->dense_hint && hints->dense_hint <= cols ? (stored > hints->dense_hint ? stored - hints->dense_hint : 0) : cols;
    ProfScope ps("structured_fill_kernel", 8.0 * filled * cosets * (double)n);
    // Columns at or above virt_first are stored only when they are dense (the transform kernels) or of class 3, and class 3 exists
    // only with more than one special row (public-input circuits): otherwise the grid stops at virt_first -- 80 instead of 234
    // column rows of blocks for a circuit without ECC gates, most of which would only look at their class and leave
    const uint32_t fill_cols = hints->nrows > 1 ? cols : std::min(cols, hints->virt_first);
    if (fill_cols)
      hipLaunchKernelGGL(structured_fill_kernel, dim3(bx, fill_cols), dim3(256), 0, st, dst, plan->d,
                         stride_cols ? stride_cols : cols, cosets, *hints, cm.first, cm.stride);
    if (hints->fill_only) return;
  }
  ntt_passes(st, plan, src, dst, cols, cosets, scale, post, src_per_coset, cm, stride_cols ? stride_cols : cols, hints ? hints->cls : nullptr,
             hints && hints->dense_hint && hints->dense_hint <= cols ? hints->dense_hint : 0);
}

}  // namespace p2
