// The field of P-384 (DR_CURVE_P384_RO / DR_CURVE_P384_NU), p = 2^384 - 2^128 - 2^96 + 2^32 - 1, for gfx950: 14 SIGNED limbs of 28 bits
// in Montgomery form with R = 2^392 (an element a is held as a R mod p; conversions happen where values cross the ABI).  The radix and
// the column scheme are fe448.hip.h's and fp521.hip.h's: one partial product is one 64-bit multiply-add into a signed 64-bit column.
//
// Why Montgomery here.  In radix B = 2^28, p = -1 + 2^4 B - 2^12 B^3 - 2^16 B^4 + 2^20 B^13, so p = -1 mod 2^28 and -p^-1 = 1 (mod 2^28):
// the quotient digit of a reduction step is the low 28 bits of the current column itself, and adding m p is m taken off that column
// (which leaves its carry) plus four shifted copies of m on the columns 1, 3, 4 and 13 places up — no product by a full-width modulus.
// It is the form fp256.hip.h uses in radix 2^29.
//
// Value of an element: sum l[i] 2^(28 i), limbs signed; the element it stands for is that value times R^-1 mod p.
// THE STEP.  A product has the columns c_0..c_26.  Fourteen steps k = 0..13 take m = c_k mod 2^28, carry c_k >> 28 into c_(k+1) and add
// m 2^4, -m 2^12, -m 2^16, m 2^20 to c_(k+1), c_(k+3), c_(k+4), c_(k+13); the result is c_14..c_26 carried into limbs 0..12 with the last
// carry as limb 13.  Its value is T = (a b + M p) / 2^392 with 0 <= M < 2^392, so |T| < p + |a b| / 2^392.
// THE BUDGET.  A column sums at most 14 products.  The steps add to one column at most one carry (below 2^36) and one each of the
// four shifted digits (2^32 + 2^40 + 2^44 + 2^48), under 2^49 in all.  So mul needs 14 max|a_i| max|b_j| + 2^49 < 2^63.
//
//   "normal" (n) : limbs 0..12 in [-2^22, 2^28 + 2^22), limb 13 in (-2^21, 2^21), |value| < 2^385 — what mul, sqr, mul2, mul_small and carry
//                  return (mul, sqr and mul2 leave limbs 0..12 in [0, 2^28); carry leaves limb 13 in [0, 2^20) and its fold, up to 2^22,
//                  on limbs 0, 1, 3, 4).  unpack returns a product: n.  The constants below are n, F384::small(v) is 1 n.
//   "k n"        : |limb| <= k (2^28 + 2^22) for limbs 0..12, |limb 13| <= k 2^21, |value| < k 2^385: sums, differences and negations of
//                  normal values; cneg / neg of an n is 1 n.
//   contract     : mul(a, b) needs  14 ka kb (2^28 + 2^22)^2 + 2^49 < 2^63, that is  ka kb <= 8  (115.6 2^56 against 128 2^56; 9 gives
//                  130); then |T| < p + 8 2^770 / 2^392 < 2^385: n out.  sqr(a) needs a <= 2 n.  mul2(a, b, c, d) = a b + c d with one
//                  reduction needs ka kb + kc kd <= 8.  (One operand is at most 7 n: 8 n does not fit a 32-bit limb.)  The limb budget
//                  alone, with limb 13 as large as the others, keeps the columns in 64 bits; the product is then right
//                  (T R = a b mod p) while |T| < 2^395 fits limb 13, that is |value(a)| |value(b)| < 2^786, and normal below 2^776.
//                  mul_small(a, k): |a_i| k < 2^62.  carry(a): any limbs with |l_i| < 2^31 - 2^5 keep their value mod p and come out with
//                  limbs 0..12 within 2^27 of [0, 2^28); n out for |value| < 2^390 (32 n).  pack, is_zero, is_odd, equal, inv and the root
//                  take any limbs with |l_i| < 2^31 - 2^5 (equal: their difference).
//
// CARRY FOLDS.  R is 2^8 p, so a value can grow 256-fold before a product's bound moves, but a sum that is tripled twice and then
// multiplied (the group law does) would leave "normal" by value.  carry therefore ripples and then folds the bits of limb 13 from 2^384
// up (h, signed, |h| <= 64 for 32 n) with 2^384 = 2^128 + 2^96 - 2^32 + 1 (mod p): h, -h 2^4, h 2^12, h 2^16 onto limbs 0, 1, 3, 4.  One
// class then describes limbs and value together, as in fp521.hip.h.
//
// CANONICAL VALUES.  pack, is_zero, is_odd and equal work on the element itself, a R^-1 mod p: canon_limbs runs the fourteen steps
// on the limbs alone (T in (-9, p + 9) for limbs below 2^31), adds p and takes p off twice where it fits.  Limbs that spell p, p + 1 or
// 2^384 therefore come out as the elements 0, R^-1 and 2^384 R^-1.
//
// Inversion: Bernstein-Yang division steps (divstep28.hip.h) in the shape Fq runs, inv_divsteps<14, 28, 40>, -p^-1 mod 2^28 = 1:
// floor((49 * 384 + 57) / 17) = 1110 steps <= 40 x 28, |d|, |e| < 21 p < 2^389, which the signed top limb holds.  It runs on the canonical
// element x = a R^-1 and gives x^-1 as a lazy 1 n operand of value class 16; the product with R^2 that follows returns x^-1 R.  The chain
// of p - 2 (f384_inv_chain) is kept for the host check to compare against.
// Roots: p = 3 mod 4, one exponentiation by (p - 3) / 4 = 2^382 - 2^126 - 2^94 + 2^30 - 1 (255 ones, a zero, 32 ones, 64 zeros, 30 ones)
// gives a^((p + 1) / 4) = a a^((p - 3) / 4) and its square decides squareness.
//
// Plain integer C++: compiles for the device (hipcc) and for the host (g++, tests/native/p384_host_check.cpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "divstep28.hip.h"
#include "limb28.hip.h"

namespace dr {

constexpr int L384 = 14;              // limbs
constexpr int W384 = 12;              // 32-bit words of a canonical element
constexpr int32_t M384 = MASK28;      // a 28-bit limb
constexpr int F384_DIVSTEP_BATCHES = 40;

// the field's description for limb28.hip.h (its constants AND the members that header calls back: small, unpack, reduce), which gives
// the element type, the limb-wise operations, the column products mul, mul2 and sqr over reduce, sqr_n, pack, is_zero, is_odd and equal
struct Fp384Consts {
    static constexpr int LIMBS = L384, WORDS = W384;
    // p, R^2 mod p, b R mod p (b of y^2 = x^3 - 3 x + b) and sqrt(12) R mod p in canonical 28-bit limbs
    static constexpr uint32_t P14[14] = {0xfffffffu, 0x000000fu, 0x0000000u, 0xffff000u, 0xffeffffu, 0xfffffffu, 0xfffffffu,
                                         0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0x00fffffu};
    static constexpr int32_t R2[14] = {0x0010000, 0xfe00000, 0x0ffffff, 0x0000000, 0x0000002, 0x0000000, 0xffffe00,
                                       0x0000fff, 0x0020000, 0x0100000, 0x0000000, 0x0000000, 0x0000000, 0x0000000};
    static constexpr int32_t B[14] = {0x12dcccd, 0x8870d04, 0x2ec0811, 0xd9474c3, 0xfc429ad, 0x1920022, 0x7f2209b,
                                      0x938ae27, 0x74bee94, 0x2094e33, 0x1f41f02, 0xf9b62b2, 0xb604fbf, 0x0008114};
    static constexpr int32_t SQRT12[14] = {0x3f1f8d7, 0x6f1be9a, 0x6471cdf, 0x3c2308f, 0x3d4f231, 0xd4183d3, 0x9cb6776,
                                           0x6b11b68, 0x3a76147, 0xfceaacb, 0x383c093, 0x98e428a, 0xb3ae40b, 0x008fa36};
    // p as little-endian words
    static constexpr uint32_t PW[12] = {0xffffffffu, 0x00000000u, 0x00000000u, 0xffffffffu, 0xfffffffeu, 0xffffffffu,
                                        0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    DR_L28_MEMBER static Limb28<Fp384Consts> small(int32_t v);
    DR_L28_MEMBER static Limb28<Fp384Consts> reduce(int64_t (&c)[2 * LIMBS - 1]);
    DR_L28_MEMBER static Limb28<Fp384Consts> unpack(const uint32_t (&w)[WORDS]);
};
using F384 = Limb28<Fp384Consts>;

// the element v for |v| <= 15: v R mod p with R = 2^392 = 2^8 - 2^12 B + 2^20 B^3 + 2^24 B^4 (mod p) in signed limbs; 1 n
DR_L28_MEMBER F384 Fp384Consts::small(int32_t v) {
    F384 r = F384::zero();
    r.l[0] = v * (1 << 8);
    r.l[1] = -v * (1 << 12);
    r.l[3] = v * (1 << 20);
    r.l[4] = v * (1 << 24);
    return r;
}

// any limbs with |l_i| < 2^31 - 2^5: one ripple, then the bits of limb 13 from 2^384 up folded onto limbs 0, 1, 3, 4 (head of the file)
DR_L28_FN F384 carry(const F384& a) {
    F384 r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < L384 - 1; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = t & M384;
        c = t >> 28;
    }
    const int32_t t = a.l[L384 - 1] + c;
    const int32_t h = t >> 20;                          // |h| < 2^11 + 1
    r.l[L384 - 1] = t & 0xfffff;
    r.l[0] += h;
    r.l[1] -= h * (1 << 4);
    r.l[3] += h * (1 << 12);
    r.l[4] += h * (1 << 16);
    return r;
}

// columns c_0..c_26 -> (sum c_k 2^(28 k)) / 2^392 mod p: the fourteen steps, then c_14..c_26 carried.  n out under mul's contract.
DR_L28_MEMBER F384 Fp384Consts::reduce(int64_t (&c)[2 * L384 - 1]) {
#pragma unroll
    for (int k = 0; k < L384; k++) {
        const int64_t v = c[k];
        const int64_t m = v & M384;
        c[k + 1] += (v >> 28) + (m << 4);               // (v - m) / 2^28: the column itself cancels against -m
        c[k + 3] -= m << 12;
        c[k + 4] -= m << 16;
        c[k + 13] += m << 20;
    }
    F384 r;
    int64_t u = c[L384];
#pragma unroll
    for (int k = 0; k < L384 - 1; k++) {
        r.l[k] = (int32_t)(u & M384);
        u = (k < L384 - 2 ? c[L384 + 1 + k] : 0) + (u >> 28);
    }
    r.l[L384 - 1] = (int32_t)u;
    return r;
}

// The products are limb28.hip.h's over reduce: mul(a, b) = a b R^-1 (196 multiply-adds; contract and step at the head of the file),
// mul2(a, b, c, d) = (a b + c d) R^-1 with one reduction (392; ka kb + kc kd <= 8) and sqr(a) = a^2 R^-1 (105; a <= 2 n).

// k a for a small constant k: |a_i| k < 2^62.  The columns ripple in 64 bits, the bits from 2^384 up (|h| < 2^43) fold as in carry, the
// limbs ripple again and what is left above 2^384 (|h| <= 2) folds without a ripple: n out
DR_L28_FN F384 mul_small(const F384& a, int32_t k) {
    int64_t t[L384];
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < L384 - 1; i++) {
        const int64_t v = (int64_t)a.l[i] * k + c;
        t[i] = v & M384;
        c = v >> 28;
    }
    const int64_t top = (int64_t)a.l[L384 - 1] * k + c;
    const int64_t h = top >> 20;
    t[L384 - 1] = top & 0xfffff;
    t[0] += h;
    t[1] -= h * (1 << 4);
    t[3] += h * (1 << 12);
    t[4] += h * (1 << 16);
    F384 r;
    c = 0;
#pragma unroll
    for (int i = 0; i < L384 - 1; i++) {
        const int64_t v = t[i] + c;
        r.l[i] = (int32_t)(v & M384);
        c = v >> 28;
    }
    const int32_t top2 = (int32_t)(t[L384 - 1] + c);
    const int32_t h2 = top2 >> 20;
    r.l[L384 - 1] = top2 & 0xfffff;
    r.l[0] += h2;
    r.l[1] -= h2 * (1 << 4);
    r.l[3] += h2 * (1 << 12);
    r.l[4] += h2 * (1 << 16);
    return r;
}

// ---------------------------------------------------------------- canonical form: 12 x u32 words, value in [0, p)
// the limbs of the ELEMENT a stands for, a R^-1 mod p, in [0, p): limbs 0..12 in [0, 2^28), limb 13 in [0, 2^20).  The fourteen steps on
// the limbs alone give T in (-9, p + 9); T + p is positive and below 3 p, so p is taken off twice where it fits.
DR_L28_FN void canon_limbs(const F384& a, int32_t (&u)[L384]) {
    int64_t col[2 * L384 - 1];
#pragma unroll
    for (int k = 0; k < 2 * L384 - 1; k++) col[k] = k < L384 ? (int64_t)a.l[k] : 0;
    const F384 t = Fp384Consts::reduce(col);
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < L384 - 1; i++) {
        const int32_t v = t.l[i] + (int32_t)Fp384Consts::P14[i] + c;
        u[i] = v & M384;
        c = v >> 28;
    }
    u[L384 - 1] = t.l[L384 - 1] + (int32_t)Fp384Consts::P14[L384 - 1] + c;      // not masked: below 2^22
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        int32_t d[L384];
        c = 0;
#pragma unroll
        for (int i = 0; i < L384 - 1; i++) {
            const int32_t v = u[i] - (int32_t)Fp384Consts::P14[i] + c;
            d[i] = v & M384;
            c = v >> 28;
        }
        d[L384 - 1] = u[L384 - 1] - (int32_t)Fp384Consts::P14[L384 - 1] + c;
        const bool take = d[L384 - 1] >= 0;
#pragma unroll
        for (int i = 0; i < L384; i++) u[i] = take ? d[i] : u[i];
    }
}
// (pack is limb28.hip.h's over canon_limbs)
// words (any value below 2^384) -> the element in Montgomery form: the value reinterpreted in radix 2^28 (limb 13 below 2^20) times R^2
// (the loop is limb28.hip.h's limbs_of_words, kept in place: through the shared routine the compiler orders the product that follows
// differently in four P-384 kernels — same counts)
DR_L28_MEMBER F384 Fp384Consts::unpack(const uint32_t (&w)[W384]) {
    F384 r;
#pragma unroll
    for (int i = 0; i < L384; i++) {
        const int bit = 28 * i, j = bit >> 5, sh = bit & 31;
        uint32_t v = w[j] >> sh;
        if (sh > 4 && j + 1 < W384) v |= w[j + 1] << (32 - sh);
        r.l[i] = (int32_t)(v & (uint32_t)M384);
    }
    return mul(r, F384::constant<R2>());
}
DR_L28_FN F384 unpack(const uint32_t (&w)[W384]) { return Fp384Consts::unpack(w); }
// whether 12 words are below p
DR_L28_FN bool below_p(const uint32_t (&w)[W384]) {
    bool lt = false, eq = true;
#pragma unroll
    for (int j = W384 - 1; j >= 0; j--) {
        lt = lt || (eq && w[j] < Fp384Consts::PW[j]);
        eq = eq && w[j] == Fp384Consts::PW[j];
    }
    return lt;
}

// ---------------------------------------------------------------- inversion and roots
// a^((p - 3) / 4): with x_k = a^(2^k - 1), x255 from x2, x3, x6, x12, x15, x30, x60, x120, x240, then a zero bit, x32, 64 zero bits
// and x30.  381 squarings and 13 products; a: 1 n
DR_L28_FN F384 f384_pow_p34(const F384& a) {
    const F384 x2 = mul(sqr(a), a);
    const F384 x3 = mul(sqr(x2), a);
    const F384 x6 = mul(sqr_n(x3, 3), x3);
    const F384 x12 = mul(sqr_n(x6, 6), x6);
    const F384 x15 = mul(sqr_n(x12, 3), x3);
    const F384 x30 = mul(sqr_n(x15, 15), x15);
    const F384 x32 = mul(sqr_n(x30, 2), x2);
    const F384 x60 = mul(sqr_n(x30, 30), x30);
    const F384 x120 = mul(sqr_n(x60, 60), x60);
    const F384 x240 = mul(sqr_n(x120, 120), x120);
    const F384 x255 = mul(sqr_n(x240, 15), x15);
    const F384 r = mul(sqr_n(x255, 33), x32);
    return mul(sqr_n(r, 94), x30);
}
// a^-1 (0 -> 0) by division steps on the canonical element, back into Montgomery form by the product with R^2 (1 n of value class 16
// times n); n out
DR_L28_FN F384 inv(const F384& a) {
    int32_t x[L384], out[L384];
    canon_limbs(a, x);
    inv_divsteps<L384, 28, F384_DIVSTEP_BATCHES>(Fp384Consts::P14, 1u, x, out);
    F384 r;
#pragma unroll
    for (int i = 0; i < L384; i++) r.l[i] = out[i];
    return mul(r, F384::constant<Fp384Consts::R2>());
}
// a^-1 (0 -> 0) as a^(p - 2) = (a^((p - 3) / 4))^4 a; a: 1 n, n out
DR_L28_FN F384 f384_inv_chain(const F384& a) { return mul(sqr_n(f384_pow_p34(a), 2), a); }
// r = a^((p + 1) / 4); true iff r^2 = a (a is a square, 0 included).  a: 1 n
DR_L28_FN bool f384_sqrt(const F384& a, F384& r) {
    r = mul(f384_pow_p34(a), a);
    return equal(sqr(r), a);
}

}  // namespace dr
