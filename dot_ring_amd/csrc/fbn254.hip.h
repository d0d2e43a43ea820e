// The field of Baby JubJub, the BN254 scalar field p = 21888242871839275222246405745257275088548364400416034343698204186575808495617
// (0x30644e72...43e1f593f0000001, 254 bits), for gfx950: 9 signed limbs of 29 bits, 64-bit column accumulators, Montgomery form
// with R = 2^261 (an element a is held as a R mod p; conversions happen where points cross the ABI).  R / p = 169.
//
// The quotient digit.  In radix 2^29, p = 2^28 + 1 (mod 2^29), and (2^28 + 1)^2 = 1 (mod 2^29), so -p^-1 = -(2^28 + 1) = 0x0FFFFFFF
// (mod 2^29): the digit of column t is m = (-t - (t << 28)) mod 2^29, two shifts and adds rather than a product.  (fr29.hip.h's
// p = 1 mod 2^32 lets it negate; this p is 1 only mod 2^28.)  Unlike P-256's p, this one is dense: adding m p costs 9 multiply-adds,
// so a product is 81 column products plus 81 reduction products — the count fr29.hip.h's Montgomery product has.  This header is
// separate from fr29.hip.h (not a template parameter of it) so that no existing kernel's code changes.
//
// The element type, the limb-wise operations, the column products over reduce() below, the word layout and the predicates on the
// canonical words are limb29.hip.h's (shared with the other 9 x 29 fields, not with fr29.hip.h); this header holds the constants, the
// Montgomery step, carry, the canonicalisation of pack and the exponentiation.
//
// Value of an element: sum l[i] 2^(29 i), limbs SIGNED; the element it stands for is that value times R^-1 mod p.
// Reduction of a product (columns c_0..c_16, int64): nine steps k = 0..8 take m from c_k, add m P_j to c_(k+j) (j = 0..8), and carry
// c_k >> 29 (exact) into c_(k+1); the result is c_9..c_16 carried into 9 limbs.  Its value is T = (a b + M p) / 2^261 with
// 0 <= M < 2^261, so T lies in (a b / 2^261, a b / 2^261 + p).
// Contract (limb bounds and value bounds):
//   "normal"  : limbs 0..7 in [0, 2^29), limb 8 in (-2^22, 2^23), value in (-2^253, p + 2^253) — what mul / sqr / mul2 return
//   mul(a, b) : max|a_i| max|b_j| <= 2^59.3 over all i, j (a column sums nine such products and nine reduction products below 2^58:
//               < 2^62.9), and |value(a)| |value(b)| < 2^514 (then T lies in (-2^253, p + 2^253)).  So: normal x normal, normal x
//               (a sum or difference of two normals), normal x carry(sum of up to sixteen normals); two sums need one carried first
//   sqr(a)    : |a_i| <= 2^29.65 for every i, |value| < 2^257 (a normal, or a carried sum of up to four)
//   mul2(a, b, c, d) = a b + c d, one reduction: every limb of all four at most 2^29 in magnitude (normals or their negations: 18
//               products per column, < 2^62.2 with the reduction's), |a b + c d| < 2^514
//   add / sub / neg / dbl / cneg: limb-wise, no carry; the caller keeps the operands of the next product within the bounds above
//   carry(a)  : limbs below 2^30 in magnitude -> limbs 0..7 in [0, 2^29), limb 8 = value >> 232 (signed); the value is unchanged
//   pack(a)   : limbs below 2^30 in magnitude, |value| < 2^263 -> the canonical element in [0, p) as 8 little-endian words
//   unpack(w) : 8 words (any value below 2^256) -> the element w in Montgomery form, normal
#pragma once
#include "limb29.hip.h"

namespace dr {

struct FbnConsts {
    // p, R mod p (the Montgomery one), R^2 mod p and the curve's d R mod p, in 29-bit limbs
    static constexpr uint32_t P[9] = {0x10000001u, 0x1f0fac9fu, 0x0e5c2450u, 0x07d090f3u, 0x1585d283u, 0x02db40c0u, 0x00a6e141u, 0x0e5c2634u, 0x0030644eu};
    static constexpr uint32_t ONE[9] = {0x0fffff57u, 0x1ea70ab4u, 0x052c068bu, 0x17504f49u, 0x0aa8075bu, 0x1d4240ceu, 0x11d54c07u, 0x052ac7a8u, 0x000dc836u};
    static constexpr uint32_t R2[9] = {0x05b69bd4u, 0x06170a5au, 0x020cddceu, 0x1db6310bu, 0x0e54d0ffu, 0x1cf855e3u, 0x1c15e103u, 0x07d09161u, 0x000a054au};
    static constexpr uint32_t D[9] = {0x1611ce80u, 0x066d1d9fu, 0x114ee73du, 0x0ef5785du, 0x03cfaeebu, 0x097286efu, 0x0c386668u, 0x04e63f7eu, 0x00008b01u};
    // p, (p - 1) / 2 and p - 2 as little-endian words
    static constexpr uint32_t PW[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    static constexpr uint32_t HALF_P[8] = {0xf8000000u, 0xa1f0fac9u, 0x3cdcb848u, 0x9419f424u, 0x40c0ac2eu, 0xdc2822dbu, 0x7098d014u, 0x18322739u};
    static constexpr uint32_t PM2[8] = {0xefffffffu, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    DR_DEV static Limb29<FbnConsts> reduce(int64_t (&c)[17]);
    DR_DEV static void pack(const Limb29<FbnConsts>& a, uint32_t (&w)[8]);
};
using Fbn = Limb29<FbnConsts>;         // an element of the BN254 scalar field in Montgomery form, signed 29-bit limbs

DR_DEV Fbn bn_one() { return Fbn::constant<FbnConsts::ONE>(); }

// limbs 0..7 into [0, 2^29), the rest into limb 8 (signed)
DR_DEV Fbn carry(const Fbn& a) {
    Fbn r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29 - 1; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = t & (int32_t)MASK29;
        c = t >> 29;
    }
    r.l[LIMBS29 - 1] = a.l[LIMBS29 - 1] + c;
    return r;
}

// columns c_0..c_16 -> (sum c_k 2^(29 k)) / 2^261 mod p, carried (the Montgomery reduction of the header)
DR_DEV Fbn FbnConsts::reduce(int64_t (&c)[17]) {
#pragma unroll
    for (int k = 0; k < LIMBS29; k++) {
        const uint32_t t = (uint32_t)c[k];
        const int64_t m = (int64_t)((0u - t - (t << 28)) & MASK29);      // -c_k p^-1 mod 2^29
#pragma unroll
        for (int j = 0; j < LIMBS29; j++) c[k + j] += m * (int64_t)FbnConsts::P[j];
        c[k + 1] += c[k] >> 29;                                          // c_k is now a multiple of 2^29
    }
    Fbn r;
    int64_t u = c[9];
#pragma unroll
    for (int k = 0; k < LIMBS29 - 2; k++) {
        r.l[k] = (int32_t)((uint32_t)u & MASK29);
        u = c[10 + k] + (u >> 29);
    }
    r.l[LIMBS29 - 2] = (int32_t)((uint32_t)u & MASK29);
    r.l[LIMBS29 - 1] = (int32_t)(u >> 29);
    return r;
}

// ---------------------------------------------------------------- 8 x u32 words <-> limbs
// the limbs of w as they are (w already in Montgomery form, as the per-context tables are)
DR_DEV Fbn bn_unpack_raw(const uint32_t (&w)[8]) { return limbs_of_words<FbnConsts>(w); }
DR_DEV Fbn bn_unpack(const uint32_t (&w)[8]) { return mul(bn_unpack_raw(w), Fbn::constant<FbnConsts::R2>()); }   // w R mod p
// canonical little-endian words of the element a stands for (a R^-1 mod p); the layout loop is limb29.hip.h's words_of_limbs, kept in
// place as in fp256.hip.h
DR_DEV void FbnConsts::pack(const Fbn& a, uint32_t (&w)[8]) {
    int64_t c[17];
#pragma unroll
    for (int k = 0; k < 17; k++) c[k] = k < LIMBS29 ? (int64_t)a.l[k] : 0;
    // |value| < 2^263: T = (value + M p) / 2^261 lies in (-4, p + 4) — one conditional addition and one subtraction of p
    Fbn t = reduce(c);
    const bool negative = t.l[LIMBS29 - 1] < 0;
    t = carry(select(negative, add(t, Fbn::constant<FbnConsts::P>()), t));
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        const uint32_t u = (uint32_t)t.l[i];
        const int bit = 29 * i, j = bit >> 5, sh = bit & 31;
        w[j] |= u << sh;
        if (sh > 3 && j + 1 < 8) w[j + 1] |= u >> (32 - sh);
    }
    sub_p_if_ge<FbnConsts>(w);
}
DR_DEV void bn_pack(const Fbn& a, uint32_t (&w)[8]) { FbnConsts::pack(a, w); }

// ---------------------------------------------------------------- exponentiations: a fixed schedule, the same in every lane
// a^e for an exponent the same in every lane (a constant): left to right with 3-bit sliding windows over a, a^3, a^5, a^7 —
// fr_pow_limbs (kernels_te.hip.h) for this field.  The branches depend on e only, never on a.
DR_DEV Fbn bn_pow(const Fbn& a, const uint32_t (&e)[8]) {
    const Fbn a2 = sqr(a), a3 = mul(a, a2), a5 = mul(a3, a2), a7 = mul(a5, a2);
    auto bit = [&](int i) -> uint32_t { return (e[i >> 5] >> (i & 31)) & 1u; };
    int i = 255;
    while (i >= 0 && !bit(i)) i--;
    if (i < 0) return bn_one();
    Fbn r = bn_one();
    bool started = false;
#pragma unroll 1
    while (i >= 0) {
        if (!bit(i)) { r = sqr(r); i--; continue; }
        int l = i >= 2 ? 3 : i + 1;
        while (!bit(i - l + 1)) l--;
        uint32_t v = 0;
        for (int k = 0; k < l; k++) v = (v << 1) | bit(i - k);
        if (started) {
#pragma unroll 1
            for (int k = 0; k < l; k++) r = sqr(r);
        }
        Fbn m;
#pragma unroll
        for (int t = 0; t < LIMBS29; t++) m.l[t] = v == 1 ? a.l[t] : v == 3 ? a3.l[t] : v == 5 ? a5.l[t] : a7.l[t];
        r = started ? mul(r, m) : m;
        started = true;
        i -= l;
    }
    return r;
}
// z^(p - 2) = z^-1 (0 -> 0): Fermat, 253 squarings and about 60 products
DR_DEV Fbn bn_inv(const Fbn& z) {
    uint32_t e[8];
#pragma unroll
    for (int i = 0; i < 8; i++) e[i] = FbnConsts::PM2[i];
    return bn_pow(z, e);
}

}  // namespace dr
