// The field of P-521 (DR_CURVE_P521_RO / DR_CURVE_P521_NU), p = 2^521 - 1, for gfx950: 19 SIGNED limbs of 28 bits, standard form (a
// Mersenne prime: no Montgomery form, no generated multiplier, reduction is a fold).  The radix and the column scheme are
// fe448.hip.h's: one partial product is one 64-bit multiply-add into a signed 64-bit column.  19 x 28 = 532 = 521 + 11: the top limb
// of a carried element holds 17 bits, and 2^532 = 2^11 (mod p).
//
// Value of an element: sum l[i] 2^(28 i) mod p, limbs signed; the value itself may be negative or above p.
//   "normal" (n) : limbs 0..17 in (-2^15, 2^28 + 2^15), limb 18 in [0, 2^17) — what mul, sqr, mul_small and carry return.  (mul, sqr and
//                  mul_small leave limbs 0..17 in [0, 2^28) but limb 2 in [-1, 2^28]; carry leaves limb 0 within 2^14 of [0, 2^28).)
//                  unpack returns limbs 0..17 in [0, 2^28) and limb 18 below 2^28: that is 1 n.
//   "k n"        : |limb| <= k (2^28 + 2^15), every limb: sums, differences and negations of normal values; cneg / neg of an n is 1 n.
//   contract     : mul(a, b) needs  19.001 max|a_i| max|b_j| + 2^37 < 2^63, that is  ka kb <= 6  (1 n x 6 n, 2 n x 3 n);
//                  sqr(a) needs a <= 2 n; mul_small(a, k): |a_i| k < 2^62; carry, pack, is_zero, is_odd, equal, inv and the root take
//                  any limbs with |l_i| < 2^31 - 2^5 (equal: their difference).
//
// THE FOLD.  A product has columns 0..36; column 19 + j folds onto column j with the factor 2^11.  A high column is a sum of up to 18
// products of ~2^56 each and times 2^11 it does not fit 64 bits, so each high column c is SPLIT before it is folded:
//     c 2^11 = (c mod 2^17) 2^11 + floor(c / 2^17) 2^28,
// the first term (below 2^28) onto column j, the second (|.| < 2^46) onto column j + 1 (j <= 17: the product has no column 37).  An
// output column is then one low column (at most 19 products), a term below 2^28 and a term below 2^46: the 19.001 above.  The carry
// out of limb 18 is taken at bit 17 (2^521 = 1) and rippled through limbs 0 and 1, its last bit left on limb 2.
// The product is schoolbook, 361 multiply-adds (sqr: 190).
//
// ZERO HAS TWO IMAGES, 0 and p (all limbs full).  pack, is_zero, is_odd and equal work on the canonical value: canon_limbs carries,
// adds p (the sum is positive and below 3 p) and takes p off twice where it fits, so limbs that spell p, p + 1 or 2^521 come out as 0, 1
// and 1.
//
// Inversion: Bernstein-Yang division steps (divstep28.hip.h) on the field's own NINETEEN limbs, inv_divsteps<19, 28, 54>,
// -p^-1 mod 2^28 = 1.  floor((49 * 521 + 57) / 17) = 1505 steps = 54 batches of 28 (53 x 28 = 1484 is short), so |d|, |e| <
// (54 / 2 + 1) p = 28 p < 2^526, which the signed top limb holds (2^531): the eleven spare bits of limb 18 do what fe448.hip.h needs a
// seventeenth limb for.  The alternative, the chain of p - 2 = 2^521 - 3 (f521_inv_chain: 520 squarings and 13 products), is kept for
// the tests and the comparison in DESIGN section 8s.
// Roots: p = 3 mod 4, one exponentiation by (p - 3) / 4 = 2^519 - 1 gives a^((p + 1) / 4) = a a^((p - 3) / 4) = a^(2^519) and its
// square decides squareness.
//
// Plain integer C++: compiles for the device (hipcc) and for the host (g++, tests/native/p521_host_check.cpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "divstep28.hip.h"
#include "limb28.hip.h"

namespace dr {

constexpr int L521 = 19;              // limbs
constexpr int W521 = 17;              // 32-bit words of a canonical element
constexpr int32_t M521 = MASK28;      // a 28-bit limb
constexpr int32_t T521 = 0x0001ffff;  // the 17 bits of limb 18
constexpr int F521_DIVSTEP_BATCHES = 54;

// the field's description for limb28.hip.h (its constants AND the members that header calls back: p_limb, small, unpack), which gives
// the element type, the limb-wise operations, sqr_n, pack, is_zero, is_odd and equal
struct Fp521Consts {
    static constexpr int LIMBS = L521, WORDS = W521, TOP_BITS = 17;
    static constexpr uint32_t P19[19] = {0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu,
                                         0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0x1ffffu};
    DR_L28_MEMBER static int32_t p_limb(int i) { return i == LIMBS - 1 ? T521 : M521; }
    DR_L28_MEMBER static Limb28<Fp521Consts> small(int32_t v);
    DR_L28_MEMBER static Limb28<Fp521Consts> unpack(const uint32_t (&w)[WORDS]);
};
using F521 = Limb28<Fp521Consts>;

DR_L28_MEMBER F521 Fp521Consts::small(int32_t v) {           // |v| < 2^28
    F521 r = F521::zero();
    r.l[0] = v;
    return r;
}

// any limbs with |l_i| < 2^31 - 2^5 -> normal: one ripple, the carry out of limb 18 taken at bit 17 (|c| < 2^14 + 1) onto limb 0
DR_L28_FN F521 carry(const F521& a) {
    F521 r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < L521 - 1; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = t & M521;
        c = t >> 28;
    }
    const int32_t t = a.l[L521 - 1] + c;
    r.l[L521 - 1] = t & T521;
    r.l[0] += t >> 17;
    return r;
}

// nineteen signed 64-bit columns (|r_i| < 2^63 - 2^37) -> normal.  The carry out of column 18 (bit 17 up, |c| < 2^46) goes onto limb 0,
// whose carry (|c| < 2^19) goes onto limb 1, whose carry (-1, 0 or 1) is left on limb 2.
DR_L28_FN F521 f521_carry64(const int64_t (&r)[L521]) {
    F521 o;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < L521 - 1; i++) {
        const int64_t t = r[i] + c;
        o.l[i] = (int32_t)(t & M521);
        c = t >> 28;
    }
    const int64_t t18 = r[L521 - 1] + c;
    o.l[L521 - 1] = (int32_t)(t18 & T521);
    const int64_t t0 = (int64_t)o.l[0] + (t18 >> 17);
    o.l[0] = (int32_t)(t0 & M521);
    const int64_t t1 = (int64_t)o.l[1] + (t0 >> 28);
    o.l[1] = (int32_t)(t1 & M521);
    o.l[2] += (int32_t)(t1 >> 28);
    return o;
}

// a b: 361 multiply-adds.  Contract and fold at the head of the file.
DR_L28_FN F521 mul(const F521& a, const F521& b) {
    int64_t r[L521];
    int64_t up = 0;                                     // floor(c / 2^17) of the high column before
#pragma unroll
    for (int j = 0; j < L521; j++) {
        int64_t c0 = 0, c1 = 0;                         // product columns j and j + 19
#pragma unroll
        for (int i = 0; i < L521; i++) {
            if (i <= j) c0 += (int64_t)a.l[i] * b.l[j - i];
            else c1 += (int64_t)a.l[i] * b.l[j + L521 - i];
        }
        r[j] = c0 + ((c1 & T521) << 11) + up;
        up = c1 >> 17;
    }
    return f521_carry64(r);
}

// a^2: the off-diagonal products once, against the doubled operand (190 multiply-adds); a <= 2 n
DR_L28_FN F521 sqr(const F521& a) {
    int32_t a2[L521];
#pragma unroll
    for (int i = 0; i < L521; i++) a2[i] = 2 * a.l[i];
    int64_t r[L521];
    int64_t up = 0;
#pragma unroll
    for (int j = 0; j < L521; j++) {
        int64_t c0 = 0, c1 = 0;
#pragma unroll
        for (int i = 0; i < L521; i++) {
            const int m0 = j - i, m1 = j + L521 - i;
            if (m0 >= i) c0 += i == m0 ? (int64_t)a.l[i] * a.l[i] : (int64_t)a2[i] * a.l[m0];
            if (m1 >= i && m1 < L521) c1 += i == m1 ? (int64_t)a.l[i] * a.l[i] : (int64_t)a2[i] * a.l[m1];
        }
        r[j] = c0 + ((c1 & T521) << 11) + up;
        up = c1 >> 17;
    }
    return f521_carry64(r);
}

// k a for a small constant k: |a_i| k < 2^62
DR_L28_FN F521 mul_small(const F521& a, int32_t k) {
    int64_t r[L521];
#pragma unroll
    for (int i = 0; i < L521; i++) r[i] = (int64_t)a.l[i] * k;
    return f521_carry64(r);
}

// ---------------------------------------------------------------- canonical form: 17 x u32 words, value in [0, p)
// (canon_limbs, the limbs of the representative in [0, p), limbs 0..17 in [0, 2^28), limb 18 in [0, 2^17), is limb28.hip.h's: carry()
// leaves a value in (-2^14, 2^521 + 2^14); + p is positive and below 3 p.  pack is that header's over it.)
// words -> limbs (no arithmetic: the value is reinterpreted in radix 2^28); any value below 2^532 (bits 532..543 are not read: the
// callers' values are below p, or 528 bits of an encoding that below_p judges); 1 n out
DR_L28_MEMBER F521 Fp521Consts::unpack(const uint32_t (&w)[W521]) { return limbs_of_words<Fp521Consts>(w); }
DR_L28_FN F521 unpack(const uint32_t (&w)[W521]) { return Fp521Consts::unpack(w); }
// whether 17 words are below p = 0x1ff ffffffff ... ffffffff
DR_L28_FN bool below_p(const uint32_t (&w)[W521]) {
    uint32_t lo = 0xffffffffu;
#pragma unroll
    for (int j = 0; j < W521 - 1; j++) lo &= w[j];
    return w[W521 - 1] < 0x1ffu || (w[W521 - 1] == 0x1ffu && lo != 0xffffffffu);
}

// ---------------------------------------------------------------- inversion and roots
// a^((p - 3) / 4) = a^(2^519 - 1): with x_k = a^(2^k - 1), x_2k = x_k^(2^k) x_k up to x_512, then 519 = 512 + 4 + 2 + 1.
// 518 squarings and 12 products; a: 1 n
DR_L28_FN F521 f521_pow_p34(const F521& a) {
    const F521 x2 = mul(sqr(a), a);
    const F521 x4 = mul(sqr_n(x2, 2), x2);
    const F521 x8 = mul(sqr_n(x4, 4), x4);
    const F521 x16 = mul(sqr_n(x8, 8), x8);
    const F521 x32 = mul(sqr_n(x16, 16), x16);
    const F521 x64 = mul(sqr_n(x32, 32), x32);
    const F521 x128 = mul(sqr_n(x64, 64), x64);
    const F521 x256 = mul(sqr_n(x128, 128), x128);
    const F521 x512 = mul(sqr_n(x256, 256), x256);
    const F521 x516 = mul(sqr_n(x512, 4), x4);
    const F521 x518 = mul(sqr_n(x516, 2), x2);
    return mul(sqr(x518), a);
}
// a^-1 (0 -> 0) by division steps: a lazy value with |limb| < 2^28 (1 n), |value| < 28 p
DR_L28_FN F521 inv(const F521& a) {
    int32_t x[L521], out[L521];
    canon_limbs(a, x);
    inv_divsteps<L521, 28, F521_DIVSTEP_BATCHES>(Fp521Consts::P19, 1u, x, out);
    F521 r;
#pragma unroll
    for (int i = 0; i < L521; i++) r.l[i] = out[i];
    return r;
}
// a^-1 (0 -> 0) as a^(p - 2) = a^(2^521 - 3) = (a^(2^519 - 1))^4 a; a: 1 n, n out
DR_L28_FN F521 f521_inv_chain(const F521& a) { return mul(sqr_n(f521_pow_p34(a), 2), a); }
// r = a^((p + 1) / 4); true iff r^2 = a (a is a square, 0 included).  a: 1 n
DR_L28_FN bool f521_sqrt(const F521& a, F521& r) {
    r = mul(f521_pow_p34(a), a);
    return equal(sqr(r), a);
}

}  // namespace dr
