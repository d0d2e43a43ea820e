// The field of secp256k1, p = 2^256 - 2^32 - 977, for gfx950: 9 signed limbs of 29 bits, 64-bit column accumulators, lazy reduction
// by folding, no Montgomery form — an element is its plain value, so nothing converts at the boundary (the shape of fe25519.hip.h).
//
// Why a fold and not a Montgomery step.  In radix B = 2^29, 2^261 = B^9 = 2^5 (2^32 + 977) = 2^8 B + 31264 (mod p): a digit h of a
// high column k + 9 comes back as 31264 h into column k and h 2^8 into column k + 1 — the constant does not fit one limb, so the fold
// has two limbs, one multiply-add and one shift-add per digit.  A Montgomery step with R = 2^261 as in fp256.hip.h would need
// -p^-1 mod 2^29 = 977^-1, which is not 1 as it is for P-256: a 32-bit product for the quotient digit and a multiply-add by 977 in each
// of the nine steps, 18 multiplications against the fold's 9, and conversions at the ABI.  Counted in gfx950 code (one operation
// between loads and a store with four operands live, minus the same kernel without it): mul 193 instructions
// (81 + 11 multiply-adds), sqr 162 (45 + 11), mul2 284, carry 47, mul_small 54 — P-256's Montgomery product in the same harness is
// 182 / 162 / 289; the figures recorded with the older harness are 150 / 115 for Ed25519 and 206 / 178 for fr29.  The fold is thus
// no cheaper than P-256's shift-only step (each digit's 64-bit shift-add is two instructions); it saves the conversions.
//
// The element type, the limb-wise operations, the column products over reduce() below, the word layout and the predicates on the
// canonical words are limb29.hip.h's; this header holds the constants, the fold, fk_fold_top / carry / mul_small, the canonicalisation
// of pack and the chains.
//
// Value of an element: sum l[i] 2^(29 i), limbs SIGNED.  Reduction of a product: columns c_0..c_16 (int64), the high columns carried
// into 29-bit digits h_0..h_7 and a top carry t (weight B^17 = B^8 B^9); c_k += 31264 h_k, c_(k+1) += h_k 2^8; c_8 += 31264 t, and t's
// second limb, t 2^8 B^9, folds once more: c_1 += t 2^16, c_0 += 31264 2^8 t.  One carry chain over c_0..c_8; the bits of c_8 from 24 up
// (q, weight 2^256 = 2^32 + 977 = 8 B + 977) come back as 977 q into limb 0 and 8 q into limb 1, carried on into limb 2.
// Contract (limb bounds; values never need a bound — the fold accepts any):
//   "normal"  : limbs 0, 1, 3..7 in [0, 2^29), limb 2 in (-2^15, 2^29 + 2^15), limb 8 in [0, 2^24) — what mul / sqr / mul2 / mul_small /
//               carry return; value in (-2^73, 2^256 + 2^73)
//   mul(a, b) : max|a_i| max|b_j| <= 2^59.9 over i, j < 8, |a_8|, |b_8| <= 2^26, every limb below 2^31 in magnitude.  Column 7 sums 8
//               products of limbs 0..7 (< 2^62.9), column 8 seven of them and two with a top limb; |t| < 2^25, the fold adds below 2^46.
//               Normal x normal and normal x (sum or difference of two normals) qualify; two sums need one of them carried first
//   sqr(a)    : |a_i| <= 2^29.95 for i < 8, |a_8| <= 2^26 (a normal, not a sum)
//   mul2(a, b, c, d) = a b + c d, one reduction: every limb of all four at most 2^29.45 in magnitude (normals and their negations)
//   mul_small(a, k): a k for 0 <= k < 2^15, limbs of a below 2^31 in magnitude (any sum of up to three normals) -> normal
//   add / sub / neg / dbl / cneg: limb-wise, no carry; the caller keeps the operands of the next product within the bounds above
//   carry(a)  : limbs below 2^31 - 8 in magnitude (any sum or difference of up to three normals) -> normal, value unchanged mod p
//   pack(a)   : limbs as for carry -> the canonical representative in [0, p) as 8 little-endian words
//   unpack(w) : 8 words (any value below 2^256) -> limbs 0..7 in [0, 2^29), limb 8 < 2^24: normal
#pragma once
#include "limb29.hip.h"

namespace dr {

constexpr uint32_t FK_M24 = 0x00ffffffu;
constexpr uint32_t FK_FOLD = 31264u;               // 2^5 977: 2^261 = 2^8 B + FK_FOLD (mod p)

struct FsecpConsts {
    // p in 29-bit limbs; p and the group order n as little-endian words
    static constexpr uint32_t P[9] = {0x1ffffc2fu, 0x1ffffff7u, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x00ffffffu};
    static constexpr uint32_t PW[8] = {0xfffffc2fu, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    static constexpr uint32_t NW[8] = {0xd0364141u, 0xbfd25e8cu, 0xaf48a03bu, 0xbaaedce6u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu};
    DR_DEV static Limb29<FsecpConsts> reduce(int64_t (&c)[17]);
    DR_DEV static void pack(const Limb29<FsecpConsts>& a, uint32_t (&w)[8]);
};
using FK = Limb29<FsecpConsts>;        // an element of GF(2^256 - 2^32 - 977) in signed 29-bit limbs

// the end of every reduction: limbs 0..7 in [0, 2^29) and u = limb 8 with everything above it (|u| < 2^63); the bits of u from 24 up
// fold into limbs 0 and 1 (2^256 = 8 B + 977), their carry into limb 2.  The masked limb 8 leaves through an empty asm statement, as
// fp_reduce's limbs do in fp256.hip.h (a gfx950 compiler once squared the unmasked register there); record 11 of the selftest,
// sqr(carry(a)), drives the case.
DR_DEV void fk_fold_top(FK& r, int64_t u) {
    r.l[8] = (int32_t)((uint32_t)u & FK_M24);
    asm volatile("" : "+v"(r.l[8]));
    const int64_t q = u >> 24;
    const int64_t v0 = (int64_t)r.l[0] + q * 977;
    r.l[0] = (int32_t)((uint32_t)v0 & MASK29);
    const int64_t v1 = (int64_t)r.l[1] + q * 8 + (v0 >> 29);
    r.l[1] = (int32_t)((uint32_t)v1 & MASK29);
    r.l[2] += (int32_t)(v1 >> 29);
}
DR_DEV FK carry(const FK& a) {
    FK r;
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29 - 1; i++) {
        const int32_t t = a.l[i] + c;
        r.l[i] = t & (int32_t)MASK29;
        c = t >> 29;
    }
    fk_fold_top(r, (int64_t)(a.l[LIMBS29 - 1] + c));
    return r;
}
// a k for a small non-negative k (the curve's 21 = 3 b, the map's B' = 1771 and |Z| = 11)
DR_DEV FK mul_small(const FK& a, uint32_t k) {
    FK r;
    int64_t u = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29 - 1; i++) {
        u += (int64_t)a.l[i] * (int64_t)k;
        r.l[i] = (int32_t)((uint32_t)u & MASK29);
        u >>= 29;
    }
    fk_fold_top(r, u + (int64_t)a.l[LIMBS29 - 1] * (int64_t)k);
    return r;
}

// columns c_0..c_16 of a product (|c_k| < 2^63 - 2^47) -> a normal element
DR_DEV FK FsecpConsts::reduce(int64_t (&c)[17]) {
    int64_t t = c[9];
#pragma unroll
    for (int k = 0; k < 8; k++) {                    // high columns -> 29-bit digits; digit k has weight B^(k + 9) = (2^8 B + 31264) B^k
        const uint32_t h = (uint32_t)t & MASK29;
        t = (t >> 29) + (k < 7 ? c[10 + k] : 0);
        c[k] += (int64_t)((uint64_t)h * FK_FOLD);
        c[k + 1] += (int64_t)((uint64_t)h << 8);
    }
    c[8] += t * (int64_t)FK_FOLD;                    // the carry out of column 16: weight B^17 = (2^8 B + 31264) B^8, and B^9 folds again
    c[1] += t * 65536;
    c[0] += t * (int64_t)(FK_FOLD * 256u);
    FK r;
    int64_t u = c[0];
#pragma unroll
    for (int k = 0; k < 8; k++) {
        r.l[k] = (int32_t)((uint32_t)u & MASK29);
        u = c[k + 1] + (u >> 29);
    }
    fk_fold_top(r, u);
    return r;
}

// ---------------------------------------------------------------- 8 x u32 words <-> limbs
DR_DEV FK fk_unpack(const uint32_t (&w)[8]) { return limbs_of_words<FsecpConsts>(w); }
// canonical little-endian words of a (limbs below 2^31 - 8 in magnitude)
DR_DEV void FsecpConsts::pack(const FK& a, uint32_t (&w)[8]) {
    // carried: value in (-2^73, 2^256 + 2^73); + p makes it positive and below 2^257
    const FK c = carry(a);
    uint32_t u[LIMBS29];
    uint32_t cy = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        u[i] = (uint32_t)c.l[i] + FsecpConsts::P[i] + cy;           // (two's complement: a negative limb 2 borrows through cy below)
        if (i < LIMBS29 - 1) { cy = (uint32_t)((int32_t)u[i] >> 29); u[i] &= MASK29; }
    }
    // fold bit 256, twice: the first fold takes p away again, and a carried value of 2^256 or more (limb 2 can exceed 2^29) then
    // still has the bit; after the second the value is in [0, 2^256)
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        const uint32_t q = u[LIMBS29 - 1] >> 24;
        u[LIMBS29 - 1] &= FK_M24;
        u[0] += 977u * q;
        u[1] += 8u * q;
        cy = 0;
#pragma unroll
        for (int i = 0; i < LIMBS29; i++) {
            u[i] += cy;
            if (i < LIMBS29 - 1) { cy = u[i] >> 29; u[i] &= MASK29; }
        }
    }
    words_of_limbs(u, w);
    sub_p_if_ge<FsecpConsts>(w);                        // below 2^256 < 2 p: one conditional subtraction
}
DR_DEV void fk_pack(const FK& a, uint32_t (&w)[8]) { FsecpConsts::pack(a, w); }

// ---------------------------------------------------------------- exponentiations: fixed chains, the same in every lane
// p = [223 ones] 0 [22 ones] 0000101111 in binary.  z^(2^223 - 1) shifted by 23 bits times z^(2^22 - 1) is the head every exponent
// below shares: 246 squarings and 11 products; z^(2^2 - 1) on the side
DR_DEV FK fk_pow_head(const FK& z, FK& x2) {
    x2 = mul(sqr(z), z);
    const FK x3 = mul(sqr(x2), z);
    const FK x6 = mul(sqr_n(x3, 3), x3);
    const FK x9 = mul(sqr_n(x6, 3), x3);
    const FK x11 = mul(sqr_n(x9, 2), x2);
    const FK x22 = mul(sqr_n(x11, 11), x11);
    const FK x44 = mul(sqr_n(x22, 22), x22);
    const FK x88 = mul(sqr_n(x44, 44), x44);
    const FK x176 = mul(sqr_n(x88, 88), x88);
    const FK x220 = mul(sqr_n(x176, 44), x44);
    const FK x223 = mul(sqr_n(x220, 3), x3);
    return mul(sqr_n(x223, 23), x22);
}
// z^((p - 3) / 4), tail 00001011: the one exponentiation of sqrt_ratio (RFC 9380 F.2.1.2)
DR_DEV FK fk_pow_p34(const FK& z) {
    FK x2;
    FK r = fk_pow_head(z, x2);
    r = mul(sqr_n(r, 5), z);
    return mul(sqr_n(r, 3), x2);
}
// z^(p - 2) = z^-1 (0 -> 0), tail 0000101101; 256 squarings and 14 products
DR_DEV FK fk_inv(const FK& z) {
    FK x2;
    FK r = fk_pow_head(z, x2);
    r = mul(sqr_n(r, 5), z);
    r = mul(sqr_n(r, 3), x2);
    return mul(sqr_n(r, 2), z);
}
// a square root of v (p = 3 mod 4: v^((p + 1) / 4), tail 00001100), checked by squaring back — "is a square" is that check, not a
// second exponentiation; false (root = 0) if v is not a square.  Which of the two roots comes out is unspecified: callers fix the sign.
DR_DEV bool fk_sqrt(const FK& v, FK& root) {
    FK x2;
    FK r = fk_pow_head(v, x2);
    r = sqr_n(mul(sqr_n(r, 6), x2), 2);
    const bool ok = equal(sqr(r), v);
    root = ok ? r : FK::zero();
    return ok;
}

}  // namespace dr
