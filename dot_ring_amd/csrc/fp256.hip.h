// The field of P-256, p = 2^256 - 2^224 + 2^192 + 2^96 - 1, for gfx950: 9 signed limbs of 29 bits, 64-bit column accumulators,
// Montgomery form with R = 2^261 (an element a is held as a R mod p; conversions happen where points cross the ABI).
//
// Why Montgomery here.  In radix B = 2^29, p = -1 + 2^9 B^3 + 2^18 B^6 - 2^21 B^7 + 2^24 B^8, so p = -1 mod 2^29 and
// -p^-1 = 1 (mod 2^29): the quotient digit of each reduction step is the low 29 bits of the current column itself, and adding
// m p is m subtracted from that column (which only leaves the carry) plus four multiply-adds by powers of two into the columns
// 3, 6, 7 and 8 places up — no multiplication by a full-width modulus.  The 9 x 29 radix is the one fe25519.hip.h uses, so the
// limb layouts of the Ed25519 kernels (LDS tables, shuffles) carry over.  Counted in the gfx950 code object (one operation
// between loads and stores, minus the same kernel without it): see DESIGN.md section 8c.
//
// The element type, the limb-wise operations, the column products over reduce() below, the word layout and the predicates on the
// canonical words are limb29.hip.h's; this header holds the constants, the Montgomery step, carry / fp_reduce, the canonicalisation
// of pack and the chains.
//
// Value of an element: sum l[i] 2^(29 i), limbs SIGNED; the element it stands for is that value times R^-1 mod p.
// Reduction of a product (columns c_0..c_16, int64): nine steps k = 0..8 take m = c_k mod 2^29, carry c_k >> 29 into c_(k+1) and
// add m 2^9, m 2^18, -m 2^21, m 2^24 to c_(k+3), c_(k+6), c_(k+7), c_(k+8); the result is c_9..c_16 carried into 9 limbs.
// Its value is T = (a b + M p) / 2^261 with 0 <= M < 2^261, so |T| < p + |a b| / 2^261.
// Contract (limb bounds and value bounds):
//   "normal"  : limbs 0..7 in [0, 2^29), limb 8 in (-2^26, 2^26); |value| < 2^258 — what mul / sqr / mul2 return
//   mul(a, b) : max|a_i| max|b_j| <= 2^59.9 over i, j < 8 (column 7 sums eight such products: < 2^62.9), |a_8|, |b_8| <= 2^29,
//               and |value(a)| |value(b)| < 3 2^517 (then |T| < 2^258).  So: normal x normal, normal x (a sum or difference of up
//               to three normals), normal x carry(sum of up to five normals); two sums need one of them carried first
//   sqr(a)    : |a_i| <= 2^29.95 for i < 8, |a_8| <= 2^29, |value| < 2^259.2 (a normal, or a carried sum of two)
//   mul2(a, b, c, d) = a b + c d, one reduction: all four normal (16 products per column, < 2^62.9)
//   add / sub / neg: limb-wise, no carry; the caller keeps the operands of the next product within the bounds above
//   carry(a)  : limbs below 2^30 in magnitude -> limbs 0..7 in [0, 2^29), limb 8 = value >> 232; the value is unchanged
//   reduce(a) : limbs below 2^31 - 8, |value| < 2^262 -> "reduced" (limbs within 2^29.33, value within 2^256.01): a carry plus one
//               fold of the bits above 2^256.  Reduced x reduced and reduced x (sum of two reduced) qualify for mul
//   pack(a)   : limbs below 2^30 in magnitude, |value| < 2^263 -> the canonical element in [0, p) as 8 little-endian words
//   unpack(w) : 8 words (any value below 2^256) -> the element w in Montgomery form, normal
#pragma once
#include "limb29.hip.h"

namespace dr {

struct Fp256Consts {
    // p, R mod p (the Montgomery one), R^2 mod p and b R mod p (b of y^2 = x^3 - 3 x + b), in 29-bit limbs
    static constexpr uint32_t P[9] = {0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x000001ffu, 0x00000000u, 0x00000000u, 0x00040000u, 0x1fe00000u, 0x00ffffffu};
    static constexpr uint32_t ONE[9] = {0x00000020u, 0x00000000u, 0x00000000u, 0x1fffc000u, 0x1fffffffu, 0x1fffffffu, 0x1f7fffffu, 0x03ffffffu, 0x00000000u};
    static constexpr uint32_t R2[9] = {0x00000c00u, 0x00000000u, 0x1fff0000u, 0x1fdfffffu, 0x1fbfffffu, 0x1fffffffu, 0x1fffffffu, 0x1ffffffeu, 0x00000013u};
    static constexpr uint32_t B[9] = {0x1897bbfbu, 0x1cdf6229u, 0x018486c4u, 0x01732821u, 0x1dad59e0u, 0x0abf7212u, 0x1a06d110u, 0x17721d20u, 0x008600c3u};
    // p and (p - 1) / 2 as little-endian words
    static constexpr uint32_t PW[8] = {0xffffffffu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0x00000000u, 0x00000000u, 0x00000001u, 0xffffffffu};
    static constexpr uint32_t HALF_P[8] = {0xffffffffu, 0xffffffffu, 0x7fffffffu, 0x00000000u, 0x00000000u, 0x80000000u, 0x80000000u, 0x7fffffffu};
    DR_DEV static Limb29<Fp256Consts> reduce(int64_t (&c)[17]);
    DR_DEV static void pack(const Limb29<Fp256Consts>& a, uint32_t (&w)[8]);
};
using F256 = Limb29<Fp256Consts>;      // an element of GF(p256) in Montgomery form, signed 29-bit limbs

DR_DEV F256 fp_one() { return F256::constant<Fp256Consts::ONE>(); }

// limbs 0..7 into [0, 2^29), the rest into limb 8 (signed)
DR_DEV F256 carry(const F256& a) {
    F256 r;
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
// carry, then the bits of limb 8 from 2^256 up (h, signed) folded back with 2^256 = 2^224 - 2^192 - 2^96 + 1 (mod p):
// limbs below 2^31 - 8 in magnitude -> "reduced": limbs 0..7 in (-2^27, 2^29 + 2^27), limb 8 in [0, 2^24), |value| < 2^256 + 2^231
// (for |value| < 2^262 before).  The group law reduces every sum of products with it before the sum meets another product.
// The limbs leave through an empty asm statement: the value is unchanged, but the compiler can no longer tie the masked limb 8 to
// the register it was masked from.  Without it, ROCm 7.2's gfx950 backend (AMD clang 22.0.0git, roc-7.2.0 26014 7b800a19) squared
// the UNMASKED register for the top column of sqr(fp_reduce(x)) (v_mad_u64_u32 vN, vN on l8 + carry instead of its low 24 bits)
// whenever h != 0: the columns written out and the reduction run on them from memory were right, the fused code was not.
// k_p256_field_selftest's record 11, sqr(reduce(a)), drives exactly that case (tests/test_gpu_p256.py).
DR_DEV F256 fp_reduce(const F256& a) {
    F256 r = carry(a);
    const uint32_t h = (uint32_t)(r.l[LIMBS29 - 1] >> 24);          // (two's complement: the fold below wraps as signed arithmetic would)
    r.l[LIMBS29 - 1] = (int32_t)((uint32_t)r.l[LIMBS29 - 1] & 0x00ffffffu);
    r.l[0] = (int32_t)((uint32_t)r.l[0] + h);
    r.l[3] = (int32_t)((uint32_t)r.l[3] - (h << 9));
    r.l[6] = (int32_t)((uint32_t)r.l[6] - (h << 18));
    r.l[7] = (int32_t)((uint32_t)r.l[7] + (h << 21));
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) asm volatile("" : "+v"(r.l[i]));
    return r;
}

// columns c_0..c_16 -> (sum c_k 2^(29 k)) / 2^261 mod p, carried (the Montgomery reduction of the header)
DR_DEV F256 Fp256Consts::reduce(int64_t (&c)[17]) {
#pragma unroll
    for (int k = 0; k < LIMBS29; k++) {
        const int64_t v = c[k];
        const uint32_t m = (uint32_t)v & MASK29;
        c[k + 1] += v >> 29;                                   // (v - m) / 2^29: the column itself cancels against -m
        c[k + 3] += (int64_t)((uint64_t)m << 9);
        c[k + 6] += (int64_t)((uint64_t)m << 18);
        c[k + 7] -= (int64_t)((uint64_t)m << 21);
        c[k + 8] += (int64_t)((uint64_t)m << 24);
    }
    F256 r;
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
// (the layout loops of fp_unpack and fp_pack are limb29.hip.h's limbs_of_words / words_of_limbs, kept in place: through the shared
// routines the compiler orders the code of P-256 and Baby JubJub kernels differently — same counts; DESIGN.md section 8j lists them)
DR_DEV F256 fp_unpack(const uint32_t (&w)[8]) {
    F256 r;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        const int bit = 29 * i, j = bit >> 5, sh = bit & 31;
        uint32_t v = w[j] >> sh;
        if (sh > 3 && j + 1 < 8) v |= w[j + 1] << (32 - sh);
        r.l[i] = (int32_t)(i < LIMBS29 - 1 ? v & MASK29 : v);
    }
    return mul(r, F256::constant<Fp256Consts::R2>());   // w R mod p
}
// canonical little-endian words of the element a stands for (a R^-1 mod p)
DR_DEV void Fp256Consts::pack(const F256& a, uint32_t (&w)[8]) {
    int64_t c[17];
#pragma unroll
    for (int k = 0; k < 17; k++) c[k] = k < LIMBS29 ? (int64_t)a.l[k] : 0;
    // |value| < 2^263: T = (value + M p) / 2^261 lies in (-4, p + 4) — one conditional addition and one subtraction of p
    F256 t = reduce(c);
    const bool negative = t.l[LIMBS29 - 1] < 0;
    t = carry(select(negative, add(t, F256::constant<Fp256Consts::P>()), t));
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        const uint32_t u = (uint32_t)t.l[i];
        const int bit = 29 * i, j = bit >> 5, sh = bit & 31;
        w[j] |= u << sh;
        if (sh > 3 && j + 1 < 8) w[j + 1] |= u >> (32 - sh);
    }
    sub_p_if_ge<Fp256Consts>(w);
}
DR_DEV void fp_pack(const F256& a, uint32_t (&w)[8]) { Fp256Consts::pack(a, w); }

// ---------------------------------------------------------------- exponentiations: fixed chains, the same in every lane
// z^(2^32 - 1), and z^(2^2 - 1), z^(2^30 - 1) on the side
DR_DEV F256 fp_pow_2_32_1(const F256& z, F256& x2, F256& x30) {
    x2 = mul(sqr(z), z);
    const F256 x3 = mul(sqr(x2), z);
    const F256 x6 = mul(sqr_n(x3, 3), x3);
    const F256 x12 = mul(sqr_n(x6, 6), x6);
    const F256 x15 = mul(sqr_n(x12, 3), x3);
    x30 = mul(sqr_n(x15, 15), x15);
    return mul(sqr_n(x30, 2), x2);
}
// z^(p - 2) = z^-1 (0 -> 0): p - 2 = ffffffff 00000001 [96 zero bits] ffffffff ffffffff fffffffd; 255 squarings, 12 products
DR_DEV F256 fp_inv(const F256& z) {
    F256 x2, x30;
    const F256 x32 = fp_pow_2_32_1(z, x2, x30);
    F256 r = mul(sqr_n(x32, 32), z);
    r = mul(sqr_n(r, 128), x32);
    r = mul(sqr_n(r, 32), x32);
    r = mul(sqr_n(r, 30), x30);
    return mul(sqr_n(r, 2), z);
}
// a square root of v (p = 3 mod 4: v^((p + 1) / 4), (p + 1) / 4 = 2^254 - 2^222 + 2^190 + 2^94), checked by squaring back;
// false (root = 0) if v is not a square.  Which of the two roots comes out is unspecified: callers fix the sign.
DR_DEV bool fp_sqrt(const F256& v, F256& root) {
    F256 x2, x30;
    const F256 x32 = fp_pow_2_32_1(v, x2, x30);
    F256 r = mul(sqr_n(x32, 32), v);
    r = mul(sqr_n(r, 96), v);
    r = sqr_n(r, 94);
    const bool ok = equal(sqr(r), v);
    root = ok ? r : F256::zero();
    return ok;
}

// z^((p - 3) / 4), (p - 3) / 4 = 2^254 - 2^222 + 2^190 + 2^94 - 1: the exponent of RFC 9380's sqrt_ratio for p = 3 mod 4.  The head
// is fp_sqrt's (z^(2^32 - 1), then z^(2^64 - 2^32 + 1)); where the root's chain ends in 2^94 z^... this one appends 94 one bits
// (32 + 32 + 30).  254 squarings, 13 products.
DR_DEV F256 fp_pow_p34(const F256& z) {
    F256 x2, x30;
    const F256 x32 = fp_pow_2_32_1(z, x2, x30);
    F256 r = mul(sqr_n(x32, 32), z);
    r = mul(sqr_n(r, 128), x32);
    r = mul(sqr_n(r, 32), x32);
    return mul(sqr_n(r, 30), x30);
}

}  // namespace dr
