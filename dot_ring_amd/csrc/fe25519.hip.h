// The field of Ed25519, p = 2^255 - 19, for gfx950: 9 signed limbs of 29 bits, 64-bit column accumulators, lazy reduction by
// folding (2^255 = 19 mod p), no Montgomery form — an element is its plain value, so nothing converts at the boundary.
//
// Radix.  9 x 29 bits rather than 10 limbs of radix 2^25.5: a product is 81 partial products instead of 100, the limbs have the
// shape fr29.hip.h gives the other curves (the same unpack / LDS / shuffle layouts), and limb 8 holds only bits 232..254, so the
// columns that touch it are 2^6 smaller and leave the headroom the group law uses to skip carries.  Counted in the gfx950 code
// object (one operation between loads and stores, minus the same kernel without it): mul 150 instructions (81 v_mad_i64_i32 + 10
// v_mad_u64_u32 for the fold), sqr 115 (45 + 10), mul2 (a b + c d, one reduction) 245, carry 33.  fr29.hip.h's Montgomery
// product is 206 / 178 / 287: the fold by 1216 replaces the 81 multiply-adds of a Montgomery reduction.
//
// The element type, the limb-wise operations, the column products over reduce() below, the word layout and the predicates on the
// canonical words are limb29.hip.h's; this header holds the constants, the fold, carry, the canonicalisation of pack and the chains.
//
// Value of an element: sum l[i] 2^(29 i), limbs SIGNED.  Reduction of a product: columns c_0..c_16 (int64), the high columns
// carried into 29-bit digits h_0..h_7 and a top carry t; c_k += 1216 h_k (2^261 = 2^6 19 = 1216 mod p), c_8 += 1216 t; one carry
// chain over c_0..c_8; the bits of c_8 from 23 up (>= 2^255) come back into limb 0 times 19, and that limb's carry into limb 1.
// Contract (limb bounds; values never need a bound — the fold accepts any):
//   "normal"  : limbs 0, 2..7 in [0, 2^29), limb 1 in (-2^17, 2^29 + 2^17), limb 8 in [0, 2^23) — what mul / sqr / mul2 / carry
//               return; value in (-2^46, 2^255 + 2^46)
//   mul(a, b) : max|a_i| max|b_j| <= 2^59.9 over i, j < 8, |a_8|, |b_8| <= 2^26, every limb below 2^31 in magnitude.  Column 7 sums
//               8 products of limbs 0..7 (< 2^62.9) and column 8 seven of them and two with a top limb; the fold adds below 2^40.
//               Normal x normal, normal x (sum or difference of two normals) qualify (2^29.01 x 2^30.01); three normals summed do not
//   sqr(a)    : |a_i| <= 2^29.95 for i < 8 (column 7: four doubled cross products), |a_8| <= 2^26
//   mul2(a, b, c, d) = a b + c d, one reduction: every limb of all four at most 2^29.45 in magnitude (16 products per column)
//   add / sub / neg / dbl / cneg: limb-wise, no carry; the caller keeps the operands of the next product within the bounds above
//   carry(a)  : any limbs below 2^30 in magnitude -> normal, value unchanged mod p
//   pack(a)   : any limbs below 2^30 in magnitude -> the canonical representative in [0, p) as 8 little-endian words (all of
//               [p, 2^255) — the 19 values just below 2^255 — and negative values are reduced)
//   unpack(w) : 8 words (any value below 2^256) -> limbs 0..7 in [0, 2^29), limb 8 < 2^24: a valid operand of every operation
#pragma once
#include "limb29.hip.h"

namespace dr {

constexpr uint32_t FE_M23 = 0x007fffffu;

struct Fe25519Consts {
    // d = -121665 / 121666 and sqrt(-1) = 2^((p-1)/4), in 29-bit limbs
    static constexpr uint32_t D[9] = {0x135978a3u, 0x0f5a6e50u, 0x10762addu, 0x00149a82u, 0x1e898007u, 0x003cbbbcu, 0x19ce331du, 0x1dc56dffu, 0x0052036cu};
    static constexpr uint32_t SQRT_M1[9] = {0x0a0ea0b0u, 0x0770d93au, 0x0bf91e31u, 0x06300d5au, 0x1d7a72f4u, 0x004c9efdu, 0x1c2cad34u, 0x1009f83bu, 0x002b8324u};
    // (p - 1) / 2 = 2^254 - 10, little-endian words: x is "the larger root" iff x > (p - 1) / 2
    static constexpr uint32_t HALF_P[8] = {0xfffffff6u, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0x3fffffffu};
    DR_DEV static Limb29<Fe25519Consts> reduce(int64_t (&c)[17]);
    DR_DEV static void pack(const Limb29<Fe25519Consts>& a, uint32_t (&w)[8]);
};
using F25 = Limb29<Fe25519Consts>;     // an element of GF(2^255 - 19) in signed 29-bit limbs

// limbs 0..7 into [0, 2^29); bits 255 and up of limb 8 folded into limb 0 times 19, its carry into limb 1
DR_DEV F25 carry(const F25& a) {
    F25 r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29 - 1; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = t & (int32_t)MASK29;
        c = t >> 29;
    }
    const int32_t top = a.l[LIMBS29 - 1] + c;
    r.l[LIMBS29 - 1] = top & (int32_t)FE_M23;
    const int32_t v = r.l[0] + 19 * (top >> 23);
    r.l[0] = v & (int32_t)MASK29;
    r.l[1] += v >> 29;
    return r;
}

// columns c_0..c_16 of a product (|c_k| < 2^63 - 2^41) -> a normal element
DR_DEV F25 Fe25519Consts::reduce(int64_t (&c)[17]) {
    int64_t t = c[9];
#pragma unroll
    for (int k = 0; k < 8; k++) {                    // high columns -> 29-bit digits; digit k has weight 2^(29 (k + 9)) = 1216 2^(29 k)
        const uint32_t h = (uint32_t)t & MASK29;
        t = (t >> 29) + (k < 7 ? c[10 + k] : 0);
        c[k] += (int64_t)((uint64_t)h * 1216u);
    }
    c[8] += t * 1216;                                // the carry out of column 16: weight 2^(29 17) = 1216 2^(29 8)
    F25 r;
    int64_t u = c[0];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        r.l[k] = (int32_t)((uint32_t)u & MASK29);
        u = c[k + 1] + (u >> 29);
    }
    r.l[8] = (int32_t)((uint32_t)u & FE_M23);
    const int64_t v = (int64_t)r.l[0] + (u >> 23) * 19;
    r.l[0] = (int32_t)((uint32_t)v & MASK29);
    r.l[1] += (int32_t)(v >> 29);
    return r;
}

// ---------------------------------------------------------------- 8 x u32 words <-> limbs
DR_DEV F25 fe_unpack(const uint32_t (&w)[8]) { return limbs_of_words<Fe25519Consts>(w); }
// canonical little-endian words of a (limbs below 2^30 in magnitude)
DR_DEV void Fe25519Consts::pack(const F25& a, uint32_t (&w)[8]) {
    // carried: value in [-2^232, 2^255 + 2^232); + 2p (limbs 2^29 - 38, 2^29 - 1 (x 7), 2^24 - 1) makes it positive
    const F25 c = carry(a);
    uint32_t u[LIMBS29];
    uint32_t cy = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        const uint32_t p2 = i == 0 ? MASK29 - 37u : i == LIMBS29 - 1 ? 0x00ffffffu : MASK29;
        u[i] = (uint32_t)c.l[i] + p2 + cy;
        if (i < LIMBS29 - 1) { cy = u[i] >> 29; u[i] &= MASK29; }
    }
    // fold bits 255.. (value < 2^257): value in [0, 2^255 + 57]
    uint32_t q = u[LIMBS29 - 1] >> 23;
    u[LIMBS29 - 1] &= FE_M23;
    cy = 19u * q;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        u[i] += cy;
        if (i < LIMBS29 - 1) { cy = u[i] >> 29; u[i] &= MASK29; }
    }
    // value >= p iff value + 19 >= 2^255: then subtract p = add 19, drop bit 255
    cy = 19u;
#pragma unroll
    for (int i = 0; i < LIMBS29 - 1; i++) cy = (u[i] + cy) >> 29;
    q = (u[LIMBS29 - 1] + cy) >> 23;
    cy = 19u * q;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        u[i] += cy;
        if (i < LIMBS29 - 1) { cy = u[i] >> 29; u[i] &= MASK29; }
    }
    u[LIMBS29 - 1] &= FE_M23;
    words_of_limbs(u, w);
}
DR_DEV void fe_pack(const F25& a, uint32_t (&w)[8]) { Fe25519Consts::pack(a, w); }

// ---------------------------------------------------------------- exponentiations (the fixed chains of ref10)
// z^(2^250 - 1), and z^11 on the side
DR_DEV F25 fe_pow_2_250_1(const F25& z, F25& z11) {
    const F25 z2 = sqr(z);
    const F25 z9 = mul(sqr_n(z2, 2), z);
    z11 = mul(z9, z2);
    const F25 z5_0 = mul(sqr(z11), z9);                       // 2^5 - 1
    const F25 z10_0 = mul(sqr_n(z5_0, 5), z5_0);
    const F25 z20_0 = mul(sqr_n(z10_0, 10), z10_0);
    const F25 z40_0 = mul(sqr_n(z20_0, 20), z20_0);
    const F25 z50_0 = mul(sqr_n(z40_0, 10), z10_0);
    const F25 z100_0 = mul(sqr_n(z50_0, 50), z50_0);
    const F25 z200_0 = mul(sqr_n(z100_0, 100), z100_0);
    return mul(sqr_n(z200_0, 50), z50_0);
}
// z^(p - 2) = z^-1 (0 -> 0); 254 squarings and 11 products, the same in every lane
DR_DEV F25 fe_inv(const F25& z) {
    F25 z11;
    const F25 t = fe_pow_2_250_1(z, z11);
    return mul(sqr_n(t, 5), z11);
}
// sqrt(u / v) for p = 5 mod 8: b = u v^3 (u v^7)^((p - 5) / 8); v b^2 = u -> b, v b^2 = -u -> b sqrt(-1), otherwise no root.
// u = 0 gives 0 (a root).  Which of the two roots comes out is unspecified: callers fix the sign.
DR_DEV bool fe_sqrt_ratio(const F25& u, const F25& v, F25& root) {
    const F25 v2 = sqr(v);
    const F25 uv3 = mul(u, mul(v2, v));
    const F25 uv7 = mul(uv3, sqr(v2));                  // u v^7
    F25 z11;
    const F25 p58 = mul(sqr_n(fe_pow_2_250_1(uv7, z11), 2), uv7);     // (u v^7)^(2^252 - 3)
    F25 b = mul(uv3, p58);
    const F25 vb2 = mul(v, sqr(b));
    if (equal(vb2, u)) { root = b; return true; }
    if (is_zero(add(vb2, u))) { root = mul(b, F25::constant<Fe25519Consts::SQRT_M1>()); return true; }
    root = F25::zero();
    return false;
}

}  // namespace dr
