// The field of Ed448 (DR_CURVE_ED448_RO / DR_CURVE_ED448_NU), p = 2^448 - 2^224 - 1, for gfx950: 16 SIGNED limbs of 28 bits, standard form
// (2^448 = 2^224 + 1 mod p is exact and the 2^224 term falls on limb 8, so there is no Montgomery form and no generated multiplier).  The
// radix and the column scheme are fq28.hip.h's: one partial product is one 64-bit multiply-add into a signed 64-bit column
// (hipcc issues it as v_mad_u64_u32 where it proves both limbs non-negative, as v_mad_i64_i32 otherwise).  16 x 28 = 448
// leaves no spare limb: all laziness lives in the four spare bits of each limb.
//
// Value of an element: sum l[i] 2^(28 i) mod p, limbs signed; the value itself may be negative or above p.
//   "normal" (n) : limbs in (-2^10, 2^28 + 2^10) — what mul, sqr, mul_small and carry return.  (carry leaves limbs 1..7, 9..15 in
//                  [0, 2^28) and limbs 0 and 8 within 2^4 of that; mul, sqr and mul_small leave 0, 8 in [0, 2^28) and 1, 9 within 2^9.)
//   "k n"        : |limb| <= k (2^28 + 2^10): sums, differences and negations of normal values; cneg / neg of an n is 1 n.
//   contract     : mul(a, b) needs  38 max|a_i| max|b_j| + 2^40 < 2^63, that is  ka kb <= 3  (1 n x 3 n, 2 n x 1.5 n; NOT 2 n x 2 n);
//                  sqr(a) needs a <= 1.7 n (callers pass 1 n); mul_small(a, k): |a_i| k < 2^62; carry, pack, is_zero, is_odd, equal,
//                  inv and the roots take any limbs with |l_i| < 2^31 - 2^5 (equal: their difference).
// Why 38: with the fold, output column 8 collects product columns 8 (9 terms), 16 (15 terms) and twice column 24 (7 terms).
//
// The product is SCHOOLBOOK, 256 multiply-adds (sqr: 136), gathered as the four product columns j, j + 8, j + 16, j + 24 that feed
// output limbs j and j + 8:  r_j = c_j + c_(j+16) + c_(j+24),  r_(j+8) = c_(j+8) + c_(j+16) + 2 c_(j+24).  The golden-ratio Karatsuba
// (192) multiplies sums of halves, which costs one of the four spare bits on both operands of its middle product; the group law below
// would pay for that with a carry before most products.
//
// Inversion: Bernstein-Yang division steps (divstep28.hip.h) on SEVENTEEN limbs, inv_divsteps<17, 28, 47>, -p^-1 mod 2^28 = 1.
// floor((49 * 448 + 57) / 17) = 1294 steps = 47 batches of 28 (46 x 28 = 1288 is one short), so |d|, |e| < (47 / 2 + 1) p = 24.5 p, which
// no signed 28-bit-radix top limb of a 16-limb number holds (8 p at the most): the seventeenth limb carries it and is folded back
// (2^448 = 2^224 + 1).  ~47 batches of ~900 instructions against 447 squarings for the chain of p - 2.
// Roots: p = 3 mod 4, one exponentiation by (p - 3) / 4 = 2^446 - 2^222 - 1 gives a^((p + 1) / 4) = a a^((p - 3) / 4) and its square
// decides squareness.
//
// Plain integer C++: compiles for the device (hipcc) and for the host (g++, tests/native/ed448_field_host_check.cpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "divstep28.hip.h"
#include "limb28.hip.h"

namespace dr {

constexpr int L448 = 16;              // limbs
constexpr int W448 = 14;              // 32-bit words of a canonical element
constexpr int32_t M448 = MASK28;
constexpr int F448_DIVSTEP_BATCHES = 47;

// the field's description for limb28.hip.h (its constants AND the members that header calls back: p_limb, small, unpack), which gives
// the element type, the limb-wise operations, sqr_n, pack, is_zero, is_odd and equal
struct Fe448Consts {
    static constexpr int LIMBS = L448, WORDS = W448, TOP_BITS = 28;
    // p with a seventeenth (zero) limb, for the division steps
    static constexpr uint32_t P17[17] = {0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xffffffeu,
                                         0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0xfffffffu, 0};
    static constexpr int32_t EDWARDS_D_NEG = 39081;      // d = -39081
    static constexpr int32_t MONT_A = 156326;            // curve448: v^2 = u^3 + A u^2 + u
    DR_L28_MEMBER static int32_t p_limb(int i) { return i == 8 ? M448 - 1 : M448; }
    DR_L28_MEMBER static Limb28<Fe448Consts> small(int32_t v);
    DR_L28_MEMBER static Limb28<Fe448Consts> unpack(const uint32_t (&w)[WORDS]);
};
using F448 = Limb28<Fe448Consts>;

DR_L28_MEMBER F448 Fe448Consts::small(int32_t v) {           // |v| < 2^28
    F448 r = F448::zero();
    r.l[0] = v;
    return r;
}

// any limbs with |l_i| < 2^31 - 2^5 -> normal: one ripple, the carry out of limb 15 (|c| <= 8) folded onto limbs 0 and 8
DR_L28_FN F448 carry(const F448& a) {
    F448 r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < L448; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = t & M448;
        c = t >> 28;
    }
    r.l[0] += c;
    r.l[8] += c;
    return r;
}

// sixteen signed 64-bit columns (|r_i| < 2^63 - 2^40) -> normal.  The carry out of column 15 (|c| < 2^36) goes onto limbs 0 and 8, whose
// own carries (|c| <= 2^8 + 1) are left on limbs 1 and 9.
DR_L28_FN F448 f448_carry64(const int64_t (&r)[L448]) {
    F448 o;
    int64_t c = 0;
#pragma unroll
    for (int i = 0; i < L448; i++) {
        const int64_t t = r[i] + c;
        o.l[i] = (int32_t)(t & M448);
        c = t >> 28;
    }
    const int64_t t0 = (int64_t)o.l[0] + c, t8 = (int64_t)o.l[8] + c;
    o.l[0] = (int32_t)(t0 & M448);
    o.l[1] += (int32_t)(t0 >> 28);
    o.l[8] = (int32_t)(t8 & M448);
    o.l[9] += (int32_t)(t8 >> 28);
    return o;
}

// a b: 256 multiply-adds.  Contract at the head of the file.
DR_L28_FN F448 mul(const F448& a, const F448& b) {
    int64_t r[L448];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        int64_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;         // product columns j, j + 8, j + 16, j + 24
#pragma unroll
        for (int i = 0; i < L448; i++) {
            if (j - i >= 0) c0 += (int64_t)a.l[i] * b.l[j - i];
            if (j + 8 - i >= 0 && j + 8 - i < L448) c1 += (int64_t)a.l[i] * b.l[j + 8 - i];
            if (j + 16 - i >= 0 && j + 16 - i < L448) c2 += (int64_t)a.l[i] * b.l[j + 16 - i];
            if (j + 24 - i >= 0 && j + 24 - i < L448) c3 += (int64_t)a.l[i] * b.l[j + 24 - i];
        }
        r[j] = c0 + c2 + c3;
        r[j + 8] = c1 + c2 + 2 * c3;
    }
    return f448_carry64(r);
}

// a^2: the off-diagonal products once, against the doubled operand (136 multiply-adds)
DR_L28_FN F448 sqr(const F448& a) {
    int32_t a2[L448];
#pragma unroll
    for (int i = 0; i < L448; i++) a2[i] = 2 * a.l[i];
    int64_t r[L448];
#pragma unroll
    for (int j = 0; j < 8; j++) {
        int64_t c[4] = {0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 4; q++) {
            const int k = j + 8 * q;
#pragma unroll
            for (int i = 0; i < L448; i++) {
                const int m = k - i;
                if (m < 0 || m >= L448 || i > m) continue;
                c[q] += i == m ? (int64_t)a.l[i] * a.l[i] : (int64_t)a2[i] * a.l[m];
            }
        }
        r[j] = c[0] + c[2] + c[3];
        r[j + 8] = c[1] + c[2] + 2 * c[3];
    }
    return f448_carry64(r);
}

// k a for a small constant k (39081, 156326): |a_i| k < 2^62
DR_L28_FN F448 mul_small(const F448& a, int32_t k) {
    int64_t r[L448];
#pragma unroll
    for (int i = 0; i < L448; i++) r[i] = (int64_t)a.l[i] * k;
    return f448_carry64(r);
}

// ---------------------------------------------------------------- canonical form: 14 x u32 words, value in [0, p)
// (canon_limbs, the limbs of the representative in [0, p), each in [0, 2^28), is limb28.hip.h's: carry() leaves a value in
// (-2^229, 2^448 + 2^229); + p is positive and below 3 p.  pack is that header's over it.)
// words -> limbs (no arithmetic: the value is reinterpreted in radix 2^28); any 448-bit value, normal out
DR_L28_MEMBER F448 Fe448Consts::unpack(const uint32_t (&w)[W448]) { return limbs_of_words<Fe448Consts>(w); }
DR_L28_FN F448 unpack(const uint32_t (&w)[W448]) { return Fe448Consts::unpack(w); }
// whether 14 words are below p = ff..ff fffffffe ff..ff (word 7 is the odd one)
DR_L28_FN bool below_p(const uint32_t (&w)[W448]) {
    uint32_t hi = 0xffffffffu, lo = 0xffffffffu;
#pragma unroll
    for (int j = 8; j < W448; j++) hi &= w[j];
#pragma unroll
    for (int j = 0; j < 7; j++) lo &= w[j];
    const bool geq = hi == 0xffffffffu && (w[7] == 0xffffffffu || (w[7] == 0xfffffffeu && lo == 0xffffffffu));
    return !geq;
}

// ---------------------------------------------------------------- inversion and roots
// a^-1 (0 -> 0): a lazy value with |limb| < 2^28 + 2^5 (1 n), |value| < 24.5 p
DR_L28_FN F448 inv(const F448& a) {
    int32_t u[L448], x[17], out[17];
    canon_limbs(a, u);
#pragma unroll
    for (int i = 0; i < L448; i++) x[i] = u[i];
    x[16] = 0;
    inv_divsteps<17, 28, F448_DIVSTEP_BATCHES>(Fe448Consts::P17, 1u, x, out);
    F448 r;
#pragma unroll
    for (int i = 0; i < L448; i++) r.l[i] = out[i];
    r.l[0] += out[16];                                  // 2^448 = 2^224 + 1
    r.l[8] += out[16];
    return r;
}
// a^((p - 3) / 4) = a^(2^446 - 2^222 - 1): with x_k = a^(2^k - 1), x_223^(2^223) x_222.  445 squarings and 12 products; a: 1 n
DR_L28_FN F448 f448_pow_p34(const F448& a) {
    const F448 x2 = mul(sqr(a), a);
    const F448 x3 = mul(sqr(x2), a);
    const F448 x6 = mul(sqr_n(x3, 3), x3);
    const F448 x12 = mul(sqr_n(x6, 6), x6);
    const F448 x24 = mul(sqr_n(x12, 12), x12);
    const F448 x27 = mul(sqr_n(x24, 3), x3);
    const F448 x54 = mul(sqr_n(x27, 27), x27);
    const F448 x108 = mul(sqr_n(x54, 54), x54);
    const F448 x111 = mul(sqr_n(x108, 3), x3);
    const F448 x222 = mul(sqr_n(x111, 111), x111);
    const F448 x223 = mul(sqr(x222), a);
    return mul(sqr_n(x223, 223), x222);
}
// r = a^((p + 1) / 4); true iff r^2 = a (a is a square, 0 included).  a: 1 n
DR_L28_FN bool f448_sqrt(const F448& a, F448& r) {
    r = mul(f448_pow_p34(a), a);
    return equal(sqr(r), a);
}

}  // namespace dr
