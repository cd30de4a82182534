// pailliercryptolib_amd -- the product-scanning arithmetic of hensel_ps.hpp on BALANCED (signed) limbs: a 1024-bit prime in
// K = 36 limbs of LB = 29 bits instead of 38 limbs of 28.
//
// Why: an unsigned column of 3K products below 2^(2LB) must stay below 2^64, which at K = 38 forces 28-bit limbs, and the
// unit-quotient trick of hensel_ps.hpp needs P = k*p with a 28-bit k: 1064 bits carry a 1024-bit prime, 8 % more limb
// products than the prime needs.  With limbs in [-2^(LB-1), 2^(LB-1)] a 29-bit radix has the SAME product magnitude
// (2^56) as the unsigned 28-bit limbs, a column of 3K products is 108 * 2^56 < 2^63, and 36 * 29 = 1044 bits hold the
// prime itself (k = 1, P = p).  The unit-quotient trick is lost (p is not -1 mod 2^LB) at no cost in multiplier slots:
// a true-digit reduction at K-1 limbs costs (K-1)^2 + (K-1) (the second term: one v_mul_lo_u32 per digit), the unit one at
// K limbs K(K-1).  What is saved are the operand products: 741 + 1444 -> 666 + 1296 per pair squaring.
//
// The arithmetic: int32_t limbs, one int64_t accumulator per column, acc += (int64_t)x * y is ONE v_mad_i64_i32.
//   digit column    q = sext_LB(lo(acc) * n0inv)  (v_mul_lo_u32, v_bfe_i32);  acc += q * n_0;  acc >>= LB (arithmetic, exact)
//   result column   r = sext_LB(acc);  acc = (acc + 2^(LB-1)) >> LB           (v_bfe_i32, one 64-bit add, one shift)
// Signed digits (|Q| <= R/2) keep every residue in about (-p/2 - p^2/R, p/2 + p^2/R): no headroom factor R >= 16 P is
// needed, only that the value fits K balanced limbs (|v| < 2^(LB*K-1)).  n0inv = -n^-1 mod 2^LB.
// Constants (capi_keys.inc: the key's balanced set) are the same VALUES as an unsigned set with k = 1 would hold -- in [0, p),
// the sign convention z = a - p*b of the pairs kept -- with balanced LIMBS; the a of a pair counts exactly modulo p^2, so it is
// not reduced to (-p/2, p/2).  hensel_decrypt_psb_kernel<36, 29, MINW> is instantiated in k_hensel.hip part 52 and serves the
// 2048-bit class (primes up to LB*K - 4 = 1040 bits) in place of hensel_decrypt_ps_kernel<38, 28, MINW>; PGPU_PS_BALANCED=0
// brings that one back.  Follow-ups not built: K = 18 for the 1024-bit class fits (54 * 2^56); the 3072-bit class does not
// (3 * 54 limbs > 128) and keeps the unsigned form.
// Measured against the unsigned K = 38 form: tools/ubench_ps.hip, profiles/ps_balanced.txt.
#ifndef PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_PS_BAL_HPP_
#define PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_PS_BAL_HPP_

#include "hensel_ps.hpp"

// 1 (default): a pair squaring forms a2 = 2a once (K shifts) and uses it twice -- the symmetric product takes a2[i] * a[j]
// (i < j) straight into the column accumulator, with no cross sum of its own and no 64-bit shift-and-add per column, and the
// second product is a2 * b instead of a * (2b).  0: the cross sums doubled by a shift, b doubled (A/B: tools/ubench_ps.hip has
// both forms as template arguments; profiles/ps_window6.txt).  Model and column bounds: tests/test_ps_window6_model.py.
#ifndef PGPU_PSB_DOUBLED
#define PGPU_PSB_DOUBLED 1
#endif
// 1 (default): the single product of two independent operands -- a2 * b of a pair squaring (doubled form), a * c of a pair
// product -- is split in the middle (Karatsuba): 3 * 18^2 = 972 limb products instead of 1296 for 36 limb subtractions and 140
// 64-bit adds, 196 / 163 instructions fewer per pair squaring / pair product.  The same column sums in another order, so the
// same digits and limbs, bit for bit; partial sums may wrap modulo 2^64 and the wraps cancel.  The symmetric product, the
// two-product scan, the reductions, the entry and the exit keep the schoolbook form.  0: the schoolbook product everywhere
// (A/B: tools/ubench_ps.hip has both forms as template arguments; profiles/ps_karatsuba.txt).  Model:
// tests/test_ps_karatsuba_model.py.
#ifndef PGPU_PSB_KARATSUBA
#define PGPU_PSB_KARATSUBA 1
#endif
// 1 (default): the upper half of a reduction is folded the same way.  From column K on every quotient digit is known, and the
// q * n terms of columns K .. 2K-2 are the upper part of a plain product of two known operands, q = q0 + q1 B^18 and
// n = n0 + n1 B^18: its cross terms q0 n1 + q1 n0 of index k = 18 .. 34 (column k + 18) are L'_k + H'_k + M'_k with L' = q0 n0,
// H' = q1 n1, M' = (q0 - q1)(n1 - n0).  L'_k is the sum the digit-serial column k formed anyway, H'_k the sum column k + 36
// needs anyway: both wait in a chain, and the 2 x 153 cross products become the 153 of M' -- 1143 q * n products per reduction
// instead of 1296, for 18 subtractions (dq = q0 - q1; dn = n1 - n0 is wave-uniform, formed once per kernel).  Where the operand
// product is in the Karatsuba form already (a2 * b, a * c) the terms ride on its chains and joins (L'_k in L_k, H'_k in Hh_k:
// the same columns), with no new waiting value and no new join.  The same column sums in another order, the same digits and
// limbs bit for bit.  The symmetric product's reduction (chains of its own: measured, no gain in the headline,
// profiles/ps_kara_reduction.txt), the two-product scan, the entry and the exit keep the schoolbook reduction.  0: the
// schoolbook reduction everywhere, the parent's code instruction for instruction (A/B: tools/ubench_ps.hip has both forms as
// template arguments).  Takes effect with PGPU_PSB_KARATSUBA.  Model: tests/test_ps_kara_reduction_model.py.
#ifndef PGPU_PSB_KARA_RED
#define PGPU_PSB_KARA_RED 1
#endif

namespace pgpu {

// the low LB bits of v as a signed number (v_bfe_i32)
template <int LB>
__device__ __forceinline__ int32_t psb_sext(uint32_t v) { return __builtin_amdgcn_sbfe((int)v, 0u, (unsigned)LB); }

// acc += x * y  (one v_mad_i64_i32)
__device__ __forceinline__ void psb_mac(int64_t& acc, int32_t x, int32_t y) { acc += (int64_t)x * y; }
// ... as a link of a chain the optimiser must leave in this order (ps_mac_pinned)
__device__ __forceinline__ void psb_mac_pinned(int64_t& acc, int32_t x, int32_t y) {
  acc += (int64_t)x * y;
  asm volatile("" ::"v"(acc));
}

// ... where the partial sum may wrap modulo 2^64 (the Karatsuba joins): the same instruction, no signed overflow in the source
__device__ __forceinline__ void psb_mac_wrap(int64_t& acc, int32_t x, int32_t y) {
  acc = (int64_t)((uint64_t)acc + (uint64_t)((int64_t)x * y));
}

// a column of 3K products of limbs up to 2^(LB-1), the digit step's q * n_0 and the recorded digit: inside int64_t
template <int K, int LB>
struct PsbFits {
  static constexpr bool value = 2 * (LB - 1) < 62 && LB + 6 < 62 &&
                                3 * (uint64_t)K * ((uint64_t)1 << (2 * (LB - 1))) + ((uint64_t)1 << (LB + 6)) < ((uint64_t)1 << 63);
};

// One Montgomery product by product scanning on balanced limbs (ps_montmul of hensel_ps.hpp; same NP / SYM / QMODE):
//   r = (x1*y1 [+ x2*y2] [+ qio as a number]) * R^-1 mod n,   |limb| <= 2^(LB-1) in, limbs in [-2^(LB-1), 2^(LB-1)) out
// n: the balanced limbs of the modulus itself (wave-uniform), n0inv = -n^-1 mod 2^LB.  The caller sees to it that the result
// fits K balanced limbs (then the carry out of the top column is zero).  r may be x2 or y1.
// DBL (with SYM): x1 holds 2 * y1, |limb| <= 2^LB.  The pairs i < j are x1[i] * y1[j], the diagonal y1[i]^2, all on the one
// accumulator: a column is at most 18 products of 2^(2LB-1), one square and K q*n terms -- 73 * 2^56 at K = 36, LB = 29.
// KARA (single product, not SYM, K even): the operand products in the Karatsuba form, |x1 limb| <= 2^LB, |y1 limb| <= 2^(LB-1):
// the differences of the halves fit int32_t (2^(LB+1), 2^LB), a half product's column sum is at most 18 * 2^(2LB-1) < 2^63.
// KRED (with KARA): the q * n terms of columns K .. 2K-2 in the folded form (PGPU_PSB_KARA_RED), dn[j] = n[H + j] - n[j]
// (wave-uniform, |dn| < 2^LB); dq = q0 - q1 is at most 2^LB.  A chain that waits then holds at most 17 operand products of
// 2^(2LB-1) and 17 q * n terms of 2^(2LB-2), and everything about it is wrapping arithmetic.  Without KRED dn is not read.
template <int K, int LB, int NP, bool SYM, int QMODE, bool DBL = false, bool KARA = false, bool KRED = false>
__device__ __forceinline__ void psb_montmul(int32_t (&r)[K], const int32_t (&x1)[K], const int32_t (&y1)[K],
                                            const int32_t (&x2)[K], const int32_t (&y2)[K], const int32_t (&n)[K],
                                            const int32_t (&dn)[K / 2], uint32_t n0inv, int32_t (&qio)[K]) {
  static_assert(!(SYM && NP != 1), "a symmetric product is a single one");
  static_assert(SYM || !DBL, "the doubled operand belongs to the symmetric product");
  static_assert(!KARA || (NP == 1 && !SYM && K % 2 == 0), "the split serves the single product of two operands, in two halves");
  static_assert(!KRED || KARA, "the folded reduction rides on the chains of the split product");
  static_assert(PsbFits<K, LB>::value, "a column sums up to 3K products below 2^(2(LB-1)): must stay below 2^63");
  constexpr int H = K / 2;
  int32_t q[K];
  int64_t acc = 0;
  int32_t onev = 1;
  asm("" : "+v"(onev));   // (keeps "+= 32-bit value" ONE v_mad_i64_i32 instead of a sign extension and an add)
  // KARA: the differences of the halves, and the column sums of the low and the high half products while they wait
  int32_t dx[KARA ? H : 1], dy[KARA ? H : 1];
  uint64_t lo[KARA ? 2 * H - 1 : 1], hi[KARA ? 2 * H - 1 : 1];
  // KRED: q0 - q1 (formed at column K, when q is complete)
  int32_t dq[KRED ? H : 1];
  if constexpr (KARA) {
#pragma unroll
    for (int j = 0; j < H; ++j) {
      dx[j] = x1[j] - x1[H + j];
      dy[j] = y1[H + j] - y1[j];
    }
  }
  ps_static_for<2 * K>([&](auto colc) __attribute__((always_inline)) {
    constexpr int col = decltype(colc)::value;
    // ---- q_i * n_j of the digits found so far, j >= 1 (n_0 belongs to the digit step), onto the carry of the column below
    if constexpr (!KRED) {
      constexpr int ilo = col < K ? 0 : col - K + 1;
      constexpr int ihi = col < K ? col : K;               // i <= col - 1
      if constexpr (ihi > ilo) {
        ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = ilo + decltype(ic)::value;
          if constexpr (PGPU_PS_PIN == 2 || (PGPU_PS_PIN == 1 && SYM)) psb_mac_pinned(acc, q[i], n[col - i]);
          else psb_mac(acc, q[i], n[col - i]);
        });
      }
    } else {
      // the folded form.  Below K: the q0 * n0 terms of columns H .. K-1 (i and col - i both below H) go into the chain that
      // waits as L'_col (with the operand products, below), every other term straight onto the accumulator, the newest
      // digit last.  From K on: only the q1 * n1 terms of index col - K < H; those of index H .. 2H-2 are H', the cross
      // terms L' + H' + M' (both with the operand products, below)
      if constexpr (col == K) {
#pragma unroll
        for (int j = 0; j < H; ++j) dq[j] = q[j] - q[H + j];
      }
      if constexpr (col > 0 && col < K) {
        ps_static_for<col>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = decltype(ic)::value;
          if constexpr (!(col >= H && i < H && col - i < H)) {
            if constexpr (PGPU_PS_PIN == 2 || (PGPU_PS_PIN == 1 && SYM)) psb_mac_pinned(acc, q[i], n[col - i]);
            else psb_mac(acc, q[i], n[col - i]);
          }
        });
      } else if constexpr (col >= K && col < K + H) {
        constexpr int m = col - K;
        ps_static_for<m + 1>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = decltype(ic)::value;
          if constexpr (PGPU_PS_PIN == 2 || (PGPU_PS_PIN == 1 && SYM)) psb_mac_pinned(acc, q[H + i], n[H + m - i]);
          else psb_mac(acc, q[H + i], n[H + m - i]);
        });
      }
    }
    // ---- products of the operands ----
    if constexpr (SYM) {
      constexpr int ilo = col < K ? 0 : col - K + 1;       // pairs i < j, i + j = col, j < K
      constexpr int ihi = (col + 1) / 2;                   // i < col - i
      if constexpr (DBL) {
        if constexpr (ihi > ilo) {
          ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = ilo + decltype(ic)::value;
            psb_mac(acc, x1[i], y1[col - i]);
          });
        }
        if constexpr (col % 2 == 0) psb_mac(acc, y1[col / 2], y1[col / 2]);
      } else {
        if constexpr (ihi > ilo) {
          int64_t cross = 0;
          ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = ilo + decltype(ic)::value;
            psb_mac(cross, x1[i], x1[col - i]);
          });
          acc = (int64_t)((uint64_t)acc + ((uint64_t)cross << 1));
        }
        if constexpr (col % 2 == 0) psb_mac(acc, x1[col / 2], x1[col / 2]);
      }
    } else if constexpr (KARA) {
      // x = x0 + x1 B^H, y = y0 + y1 B^H:  x y = L + (L + Hh + M) B^H + Hh B^2H  with L = x0 y0, Hh = x1 y1 and
      // M = (x0 - x1)(y1 - y0) -- 3 H^2 products.  The column sums L_k, Hh_k are chains of their own from a zero addend
      // (L_k waits from column k to k + H, Hh_k from k + H to k + 2H); the M products go straight onto the accumulator.
      // Everything here is wrapping 64-bit arithmetic (a partial sum of the M products may pass 2^63 where they land before
      // the join; the wraps cancel): the finished column is the schoolbook column.
      if constexpr (col <= 2 * H - 2) {
        constexpr int ilo = col < H ? 0 : col - H + 1;
        constexpr int ihi = col < H ? col + 1 : H;
        int64_t s = 0;
        ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = ilo + decltype(ic)::value;
          psb_mac_wrap(s, x1[i], y1[col - i]);
        });
        if constexpr (KRED && col >= H) {                  // L'_col: the q0 * n0 terms of this column, the same i
          ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = ilo + decltype(ic)::value;
            psb_mac_wrap(s, q[i], n[col - i]);
          });
        }
        lo[col] = (uint64_t)s;
        acc = (int64_t)((uint64_t)acc + lo[col]);
      }
      if constexpr (col >= H && col <= 3 * H - 2) {
        constexpr int k = col - H;
        constexpr int ilo = k < H ? 0 : k - H + 1;
        constexpr int ihi = k < H ? k + 1 : H;
        int64_t s = 0;
        ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = ilo + decltype(ic)::value;
          psb_mac_wrap(s, x1[H + i], y1[H + k - i]);
        });
        if constexpr (KRED && k >= H) {                    // H'_k: the q1 * n1 terms column k + 2H would take
          ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = ilo + decltype(ic)::value;
            psb_mac_wrap(s, q[H + i], n[H + k - i]);
          });
        }
        hi[k] = (uint64_t)s;
        acc = (int64_t)((uint64_t)acc + (lo[k] + hi[k]));
        ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
          constexpr int i = ilo + decltype(ic)::value;
          psb_mac_wrap(acc, dx[i], dy[k - i]);
        });
        if constexpr (KRED && k >= H) {                    // M'_k
          ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
            constexpr int i = ilo + decltype(ic)::value;
            psb_mac_wrap(acc, dq[i], dn[k - i]);
          });
        }
      }
      if constexpr (col >= 2 * H && col <= 4 * H - 2) acc = (int64_t)((uint64_t)acc + hi[col - 2 * H]);
    } else {
      constexpr int ilo = col < K ? 0 : col - K + 1;
      constexpr int ihi = col < K ? col + 1 : K;
      ps_static_for<ihi - ilo>([&](auto ic) __attribute__((always_inline)) {
        constexpr int i = ilo + decltype(ic)::value;
        if constexpr (PGPU_PS_PIN == 2) {
          psb_mac_pinned(acc, x1[i], y1[col - i]);
          if constexpr (NP == 2) psb_mac_pinned(acc, x2[i], y2[col - i]);
        } else {
          psb_mac(acc, x1[i], y1[col - i]);
          if constexpr (NP == 2) psb_mac(acc, x2[i], y2[col - i]);
        }
      });
    }
    if constexpr (col < K) {
      if constexpr (QMODE == 2) psb_mac(acc, qio[col], onev);
      q[col] = psb_sext<LB>((uint32_t)acc * n0inv);
      psb_mac(acc, q[col], n[0]);
      acc >>= LB;                                          // (exact: the low LB bits are zero)
      if constexpr (QMODE == 1) qio[col] = q[col];
    } else {
      r[col - K] = psb_sext<LB>((uint32_t)acc);
      if constexpr (col + 1 < 2 * K) acc = (acc + ((int64_t)1 << (LB - 1))) >> LB;
    }
  });
}

// the parking area and the window table hold 32-bit patterns: the balanced limbs go through the helpers of hensel_ps.hpp
template <int K>
__device__ __forceinline__ uint32_t (&psb_bits(int32_t (&v)[K]))[K] { return reinterpret_cast<uint32_t(&)[K]>(v); }
template <int K>
__device__ __forceinline__ const uint32_t (&psb_bits(const int32_t (&v)[K]))[K] { return reinterpret_cast<const uint32_t(&)[K]>(v); }

// (a, b) = (a, b)^2 (ps_pairsqr):  t = a*a with its digits q;  b = (2*a*b + q) reduced;  a = t.   |2b| <= 2^LB fits int32_t
// DBL: a2 = 2a serves both products (|2a| <= 2^LB as well): t = sym(a2, a), b = (a2*b + q) reduced -- the same column sums in
// another order of summation, so the same digits and the same limbs, bit for bit.
// KARA (with DBL): the b part's a2 * b in the Karatsuba form of psb_montmul.
// KRED (with DBL and KARA): the b part's reduction folded onto the chains of a2 * b.
template <int K, int LB, bool DBL = (PGPU_PSB_DOUBLED != 0), bool KARA = (PGPU_PSB_KARATSUBA != 0),
          bool KRED = (DBL && KARA && PGPU_PSB_KARA_RED != 0)>
__device__ __forceinline__ void psb_pairsqr(int32_t (&a)[K], int32_t (&b)[K], const int32_t (&n)[K], const int32_t (&dn)[K / 2],
                                            uint32_t n0inv) {
  static_assert(!KRED || (DBL && KARA), "the folded reduction belongs to the doubled Karatsuba form");
  int32_t qd[K], t[K];
  if constexpr (DBL) {
    int32_t a2[K];
#pragma unroll
    for (int j = 0; j < K; ++j) a2[j] = a[j] * 2;
    psb_montmul<K, LB, 1, true, 1, true>(t, a2, a, a2, a, n, dn, n0inv, qd);
    psb_montmul<K, LB, 1, false, 2, false, KARA, KRED>(b, a2, b, a2, b, n, dn, n0inv, qd);
  } else {
    psb_montmul<K, LB, 1, true, 1>(t, a, a, a, a, n, dn, n0inv, qd);
#pragma unroll
    for (int j = 0; j < K; ++j) b[j] *= 2;
    psb_montmul<K, LB, 1, false, 2>(b, a, b, a, b, n, dn, n0inv, qd);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) a[j] = t[j];
}

// (a, b) = (a, b) (x) (c, d) (ps_pairmul: b waits in LDS through the first product, t through the second)
// KARA: the first product a * c in the Karatsuba form (balanced operands: the window loop and the table build; the entry and
// the exit, whose limbs are relaxed sums and which run once, pass false)
// KRED (with KARA): the first product's reduction folded onto its chains; the two-product scan keeps the schoolbook reduction
template <int K, int LB, bool KARA = (PGPU_PSB_KARATSUBA != 0), bool KRED = (KARA && PGPU_PSB_KARA_RED != 0)>
__device__ __forceinline__ void psb_pairmul(int32_t (&a)[K], int32_t (&b)[K], const int32_t (&c)[K], const int32_t (&d)[K],
                                            const int32_t (&n)[K], const int32_t (&dn)[K / 2], uint32_t n0inv, uint4* slot) {
  int32_t qd[K];
  {
    int32_t t[K];
    ps_park_store<K>(slot, psb_bits<K>(b));
    __builtin_amdgcn_sched_barrier(0);
    psb_montmul<K, LB, 1, false, 1, false, KARA, KRED>(t, a, c, a, c, n, dn, n0inv, qd);
    __builtin_amdgcn_sched_barrier(0);
    ps_park_swap<K>(slot, psb_bits<K>(b), psb_bits<K>(t));
    __builtin_amdgcn_sched_barrier(0);
  }
  psb_montmul<K, LB, 2, false, 2>(b, a, d, b, c, n, dn, n0inv, qd);
  __builtin_amdgcn_sched_barrier(0);
  ps_park_load<K>(psb_bits<K>(a), slot);
}

// r = x*y*R^-1 mod n, one product
template <int K, int LB>
__device__ __forceinline__ void psb_mul(int32_t (&r)[K], const int32_t (&x)[K], const int32_t (&y)[K], const int32_t (&n)[K],
                                        uint32_t n0inv) {
  int32_t none[K], nodn[K / 2] = {};
  psb_montmul<K, LB, 1, false, 0>(r, x, y, x, y, n, nodn, n0inv, none);
}

// a += k with a carry round that re-balances (limbs may be sums of a few balanced limbs); the value must fit K balanced limbs
template <int K, int LB>
__device__ __forceinline__ void psb_add(int32_t (&a)[K], const int32_t (&k)[K]) {
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int32_t u = a[j] + k[j] + c;
    a[j] = j + 1 < K ? psb_sext<LB>((uint32_t)u) : u;
    c = (u + (1 << (LB - 1))) >> LB;
  }
}

// NI relaxed unsigned limbs of LB bits (below 2^31: the pair rows the other kernels write) -> K balanced limbs, NI <= K
template <int K, int LB, int NI>
__device__ __forceinline__ void psb_relimb(int32_t (&out)[K], const uint32_t (&in)[NI]) {
  static_assert(NI <= K, "the chunk must fit");
  uint32_t c = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const uint32_t u = (j < NI ? in[j] : 0u) + c;            // (below 2^31 + 4: the bias below cannot wrap)
    out[j] = j + 1 < K ? psb_sext<LB>(u) : (int32_t)u;
    c = (u + (1u << (LB - 1))) >> LB;
  }
}

// canonical unsigned limbs of v modulo 2^(LB*K) (two's complement); returns the sign: 0 (v >= 0) or -1 (v < 0).
// Limbs of v may be sums of a few balanced limbs.
template <int K, int LB>
__device__ __forceinline__ int32_t psb_canon(uint32_t (&out)[K], const int32_t (&v)[K]) {
  int32_t c = 0;
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const int32_t u = v[j] + c;
    out[j] = (uint32_t)u & PsLimb<LB>::mask;
    c = u >> LB;
  }
  return c;
}

// c*R modulo the side's p^2 as a pair (a, b) from the pair row of the n^2 domain (ps_entry_from_pair_row: per chunk of the
// row a single product for its b half and a pair product for its a half).  The constants are values in [0, p) in balanced
// limbs; a chunk is below 2^(29*35), so the sums of at most four chunk products stay below 5 p -- K balanced limbs hold
// +-2^(LB*K-1) >= +-7.9 p (tests/test_ps_balanced_model.py).  ma / mb leave holding copies of a / b.
template <int K, int LB>
__device__ __forceinline__ void psb_entry_from_pair_row(const HenselArgs& A, int side, size_t elem, const int32_t (&n)[K],
                                                        uint32_t n0inv, uint4* slot, int32_t (&a)[K], int32_t (&b)[K],
                                                        int32_t (&ma)[K], int32_t (&mb)[K]) {
  static_assert(LB == kLimbBits, "the row limbs are re-balanced, not re-cut");
  constexpr int NI = (K * LB - 2) / LB + 1;      // row limbs per entry chunk that fit a half, plus one for the carry
#define HCTX(field) (side ? A.ctx[1].field : A.ctx[0].field)
  const uint32_t* row = A.ct_pair + elem * A.ct_pair_stride;
  int32_t acc_a[K], acc_b[K], nodn[K / 2] = {};      // (nodn: the schoolbook reduction reads no differences)
#pragma unroll
  for (int j = 0; j < K; ++j) acc_a[j] = acc_b[j] = 0;
#pragma unroll 1
  for (int i = 0; i < A.pchunks; ++i) {
    const int first = i * A.pchunk_limbs;
    uint32_t za[NI], zb[NI];
    int32_t cb[K], tb[K];
#pragma unroll
    for (int j = 0; j < NI; ++j) {
      const bool in = j < A.pchunk_limbs && first + j < A.pair_l2;
      za[j] = in ? row[first + j] : 0u;
      zb[j] = in ? row[A.pair_l2 + first + j] : 0u;
    }
#pragma unroll
    for (int j = 0; j < K; ++j) {
      b[j] = 0;
      cb[j] = (int32_t)HCTX(pcb)[(size_t)i * K + j];
      ma[j] = (int32_t)HCTX(pconv)[(size_t)i * 2 * K + j];
      mb[j] = (int32_t)HCTX(pconv)[(size_t)i * 2 * K + K + j];
    }
    int32_t zl[K];
    psb_relimb<K, LB, NI>(zl, zb);
    psb_mul<K, LB>(tb, zl, cb, n, n0inv);
    psb_relimb<K, LB, NI>(a, za);
    psb_pairmul<K, LB, false>(a, b, ma, mb, n, nodn, n0inv, slot);
    psb_add<K, LB>(b, tb);
    psb_add<K, LB>(acc_a, a);
    psb_add<K, LB>(acc_b, b);
  }
#pragma unroll
  for (int j = 0; j < K; ++j) {
    a[j] = ma[j] = acc_a[j];
    b[j] = mb[j] = acc_b[j];
  }
#undef HCTX
}

// Exit: (a, b) times (hp, 0) under the prime (P = p: no factor k to cancel first).  The product is the pair (a', b') of
// hp + p * (L * hp) modulo p^2, L = L_p(c^(p-1)): a' = hp + j p with the canonical hp in [0, p), so
//   mp = (j - b') mod p,   j = [a' >= p] - [a' < 0]   (a' is signed here: |a'| < 0.6 p, so j is -1 or 0; the general form
// is kept), and |j - b'| < p: one conditional + p makes it canonical.  Written as canonical words to row 2*elem + side of A.out.
template <int K, int LB>
__device__ __forceinline__ void psb_exit_words(const HenselArgs& A, int side, size_t elem, bool live, uint4* slot,
                                               const int32_t (&n)[K], uint32_t n0inv, int32_t (&a)[K], int32_t (&b)[K],
                                               int32_t (&ma)[K], int32_t (&mb)[K]) {
  constexpr int W64 = (K * LB + 63) / 64;
#define HCTX(field) (side ? A.ctx[1].field : A.ctx[0].field)
#pragma unroll
  for (int j = 0; j < K; ++j) {
    ma[j] = (int32_t)HCTX(h)[j];
    mb[j] = 0;
  }
  int32_t nodn[K / 2] = {};
  psb_pairmul<K, LB, false>(a, b, ma, mb, n, nodn, n0inv, slot);
  uint32_t u0[K], u1[K];
  const int32_t neg_a = psb_canon<K, LB>(u0, a);             // -1: a' < 0
#pragma unroll
  for (int j = 0; j < K; ++j) ma[j] = a[j] - n[j];
  const int32_t below_p = psb_canon<K, LB>(u0, ma);          // -1: a' < p
  const int32_t jflag = (below_p + 1) + neg_a;
#pragma unroll
  for (int j = 0; j < K; ++j) ma[j] = (j == 0 ? jflag : 0) - b[j];
  const int32_t neg_d = psb_canon<K, LB>(u0, ma);            // j - b'
#pragma unroll
  for (int j = 0; j < K; ++j) ma[j] += n[j];
  (void)psb_canon<K, LB>(u1, ma);                            // j - b' + p
#pragma unroll
  for (int j = 0; j < K; ++j) u0[j] = neg_d ? u1[j] : u0[j];
  if (live) {
    uint64_t* out = A.out + (2 * elem + side) * A.out_stride;
    const int ow = A.out_words;
    ps_static_for<W64>([&](auto wc) __attribute__((always_inline)) {
      constexpr int ww = decltype(wc)::value;
      if (ww < ow) out[ww] = ps_word<K, LB, ww>(u0);
    });
    for (int ww = W64; ww < ow; ++ww) out[ww] = 0;
  }
#undef HCTX
}

// hensel_decrypt_ps_kernel on balanced limbs: the same launch shape (one wavefront = 64 ciphertexts of ONE side), the same
// window table, masked gather, window loop and digit scan; the constants of A.ctx are the key's BALANCED set (capi_keys.inc:
// values in [0, p) in balanced limbs, nhat = n = p, n0inv = -p^-1 mod 2^LB), the pair rows of A.ct_pair the 29-bit rows every
// other kernel writes, the output the same canonical words (mp, mq) for crt_kernel.
template <int K, int LB, int MINW>
__global__ __launch_bounds__(kWGThreads, MINW) void hensel_decrypt_psb_kernel(HenselArgs A) {
  constexpr int K4 = (K + 3) / 4;
  raise_wave_priority();
  __shared__ uint4 park_[kWavesPerWG][K4][kWave];
  const int lane = threadIdx.x % kWave, wv = threadIdx.x / kWave;
  uint4* slot = &park_[wv][0][lane];
  const size_t wave_id = (size_t)blockIdx.x * kWavesPerWG + wv;
  const int side = __builtin_amdgcn_readfirstlane((int)(wave_id & 1));
  const size_t first_elem = (wave_id >> 1) * kWave;
  size_t elem = first_elem + lane;
  if (elem >= A.count) elem = A.count - 1;
#define HCTX(field) (side ? A.ctx[1].field : A.ctx[0].field)
  int32_t n[K], a[K], b[K], ma[K], mb[K];
#pragma unroll
  for (int j = 0; j < K; ++j) n[j] = (int32_t)ps_uniform(HCTX(nhat)[j]);   // wave-uniform: SGPR operands of the products
  const uint32_t n0inv = ps_uniform(HCTX(n0inv));
  // n1 - n0 of the folded reductions (PGPU_PSB_KARA_RED), wave-uniform like n
  int32_t dn[K / 2];
#pragma unroll
  for (int j = 0; j < K / 2; ++j) dn[j] = PGPU_PSB_KARA_RED != 0 ? (int32_t)ps_uniform((uint32_t)(n[K / 2 + j] - n[j])) : 0;
  const int w = A.window, tsize = 1 << w, half = tsize >> 1;
  const bool gather = A.ct_gather != 0;
  // the odd-power table and the product placed inside the window (hensel_ps.hpp); the masked policy keeps the full table and
  // the fixed order
  const bool odd = !gather && A.ps_odd_table != 0;
  uint4* tw = reinterpret_cast<uint4*>(A.table + wave_id * ps_table_words<K>(ps_table_entries(w, odd))) + lane;
  const uint64_t* ep = A.exp + (size_t)side * A.exp_stride;
  const int nwin = (A.exp_bits + w - 1) / w;
  auto digit = [&](int i) -> int {
    int bit = i * w;
    int word = bit >> 6, sh = bit & 63;
    uint64_t v = (word < A.exp_words) ? ep[word] >> sh : 0;
    if (sh + w > 64 && word + 1 < A.exp_words) v |= ep[word + 1] << (64 - sh);
    return (int)(v & (uint64_t)(tsize - 1));
  };

  // ---- c*R as a pair from the pair row of the n^2 domain ----
  psb_entry_from_pair_row<K, LB>(A, side, elem, n, n0inv, slot, a, b, ma, mb);
  // ---- window table (hensel_ps.hpp), one loop for both forms.  Half-squared: entry 0 = one, entry 1 = base, entry 2k =
  // (entry k)^2, entry 2k+1 = entry 2k times base.  Odd powers: entry j = base^(2j-1); trip 0 squares the base into the slot
  // of the LAST entry, every later trip k fetches it from there as the multiplier and writes entry k+1 = entry k times
  // base^2 -- the last trip over the slot it read.  The base leaves the entry below 2.1 p / 4.2 p, its square and the
  // products by it below 0.6 p (tests/test_ps_odd_table_model.py) ----
  ps_table_store<K>(tw, 1, psb_bits<K>(a), psb_bits<K>(b));
  {
    uint32_t oa[K], ob[K];
#pragma unroll
    for (int j = 0; j < K; ++j) {
      oa[j] = HCTX(one)[j];
      ob[j] = HCTX(one)[K + j];
    }
    ps_table_store<K>(tw, 0, oa, ob);
  }
#pragma unroll 1
  for (int k = odd ? 0 : 1; k < half && half > 1; ++k) {
    const bool sq = !odd || k == 0, mu = !odd || k > 0;
    ps_table_load<K>(psb_bits<K>(a), psb_bits<K>(b), tw, k > 1 ? k : 1, tsize, false);
    if (sq) {
      psb_pairsqr<K, LB>(a, b, n, dn, n0inv);
      ps_table_store<K>(tw, odd ? half : 2 * k, psb_bits<K>(a), psb_bits<K>(b));
    }
    __builtin_amdgcn_sched_barrier(0);      // (the multiplier is fetched AFTER the squaring: held across it, it costs 2K registers)
    if (mu) {
      ps_table_load<K>(psb_bits<K>(ma), psb_bits<K>(mb), tw, odd ? half : 1, tsize, false);
      psb_pairmul<K, LB>(a, b, ma, mb, n, dn, n0inv, slot);
      ps_table_store<K>(tw, odd ? k + 1 : 2 * k + 1, psb_bits<K>(a), psb_bits<K>(b));
    }
  }
  // ---- main loop: per window w squarings and one multiplication by a table entry (always, also entry 0 = one).  Half-
  // squared form: the top digit's entry is loaded, every other window multiplies after its squarings.  Odd form: the top
  // window is an ordinary one from `one` with the bits the exponent leaves it (A.exp_bits covers the exponent), and the
  // product of digit d = 2^s o follows w - s squarings (ps_window_place: wave-uniform, in SGPRs) ----
#pragma unroll
  for (int j = 0; j < K; ++j) {
    a[j] = (int32_t)HCTX(one)[j];
    b[j] = (int32_t)HCTX(one)[K + j];
  }
  int win = nwin - 1;
  if (!odd && nwin > 0) {
    ps_table_load<K>(psb_bits<K>(a), psb_bits<K>(b), tw, digit(nwin - 1), tsize, gather);
    --win;
  }
#pragma unroll 1
  for (; win >= 0; --win) {
    const int wl = (odd && win == nwin - 1) ? A.exp_bits - win * w : w;
    int pos, idx;
    ps_window_place(digit(win), wl, odd, pos, idx);
#pragma unroll 1
    for (int i = 0; i <= wl; ++i) {
      if (i == pos) {
        // (the entry is fetched where it is used: held across squarings it would cost 2K registers)
        ps_table_load<K>(psb_bits<K>(ma), psb_bits<K>(mb), tw, idx, tsize, gather);
        psb_pairmul<K, LB>(a, b, ma, mb, n, dn, n0inv, slot);
      }
      if (i < wl) psb_pairsqr<K, LB>(a, b, n, dn, n0inv);
    }
  }
  // ---- exit under the prime: (a, b) times (hp, 0);  mp = ([a' >= p] - [a' < 0] - b') mod p ----
  psb_exit_words<K, LB>(A, side, elem, first_elem + lane < A.count, slot, n, n0inv, a, b, ma, mb);
#undef HCTX
}

}  // namespace pgpu

#endif  // PAILLIERCRYPTOLIB_AMD_CSRC_HENSEL_PS_BAL_HPP_
