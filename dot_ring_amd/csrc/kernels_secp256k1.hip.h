// secp256k1 kernels (DR_CURVE_SECP256K1 and DR_CURVE_SECP256K1_NU; the reference's specs/secp256k1.py, Secp256k1_RO / Secp256k1_NU): the
// short Weierstrass group law with a = 0, b = 7 over GF(2^256 - 2^32 - 977) (fsecp256k1.hip.h) and the kernels that fill, for this
// curve, the roles kernels_p256.hip.h fills for P-256 — variable-base scalar multiplication on a fixed schedule, grouped MSMs, point
// decoding (plain SEC1 compressed) — and, new with this curve, the map of RFC 9380 hashing to the curve: simplified SWU onto an
// isogenous curve, the 3-isogeny back, and for the uniform (RO) variant the sum of two images.  The existing kernels stay as they are.
//
// Points cross the ABI as affine x || y little-endian; 64 zero bytes are the identity ((0, 0) is not on the curve).  Inside: homogeneous
// projective (X : Y : Z), identity (0 : 1 : 0).  The group law is the complete one of Renes, Costello and Batina (2016), algorithms 7
// (addition) and 9 (doubling) for a = 0 with b3 = 3 b = 21: no exceptional cases and no branches.  The comments give the limb class of
// every intermediate against fsecp256k1.hip.h's contract: n = normal, sK = a sum or difference of K normals.
#pragma once
#include "fsecp256k1.hip.h"
#include "sswu.hip.h"
#include "wave_curve.hip.h"
#include "wave_msm.hip.h"

namespace dr {

constexpr int K1_BLOCK = 64;          // one wave per workgroup, as k_p256_scalar_mul
constexpr uint32_t K1_B3 = 21;

struct K1Point {
    FK x, y, z;
};

DR_DEV K1Point k1_identity() {
    K1Point p;
    p.x = FK::zero(); p.y = FK::small(1); p.z = FK::zero();
    return p;
}

// algorithm 9, a = 0: 2 squarings, 4 products, one fused pair, two products by 21 / 8; coordinates n in, n out
DR_DEV K1Point k1_dbl(const K1Point& p) {
    const FK t0 = sqr(p.y);                                      // n
    const FK z8 = mul_small(t0, 8);                              // 8 Y^2: n
    const FK t1 = mul(p.y, p.z);                                 // n
    const FK t2 = mul_small(sqr(p.z), K1_B3);                    // 21 Z^2: n
    const FK y3a = carry(add(t0, t2));                           // Y^2 + 21 Z^2: n
    const FK t0b = carry(sub(t0, add(t2, dbl(t2))));             // Y^2 - 63 Z^2: n - s3 -> n
    K1Point r;
    r.x = mul(dbl(t0b), mul(p.x, p.y));                          // 2 (Y^2 - 63 Z^2) X Y: s2 x n
    r.y = mul2(t0b, y3a, t2, z8);                                // t0b y3a + 8 . 21 Y^2 Z^2: n
    r.z = mul(t1, z8);                                           // 8 Y^3 Z: n
    return r;
}

// algorithm 7, a = 0: 6 products, 3 fused pairs, two products by 21; coordinates n in, n out
DR_DEV K1Point k1_add(const K1Point& p, const K1Point& q) {
    const FK t0 = mul(p.x, q.x), t1 = mul(p.y, q.y), t2 = mul(p.z, q.z);                      // n
    const FK t3 = carry(sub(mul(carry(add(p.x, p.y)), add(q.x, q.y)), add(t0, t1)));          // X1 Y2 + X2 Y1: n x s2 - s2 -> n
    const FK t4 = carry(sub(mul(carry(add(p.y, p.z)), add(q.y, q.z)), add(t1, t2)));          // Y1 Z2 + Y2 Z1: n
    const FK y3 = mul_small(carry(sub(mul(carry(add(p.x, p.z)), add(q.x, q.z)), add(t0, t2))), K1_B3);   // 21 (X1 Z2 + X2 Z1): n
    const FK t0b = carry(add(t0, dbl(t0)));                                                    // 3 X1 X2: n
    const FK t2b = mul_small(t2, K1_B3);                                                       // 21 Z1 Z2: n
    const FK z3 = carry(add(t1, t2b)), t1b = carry(sub(t1, t2b));                              // n
    K1Point r;
    r.x = mul2(t3, t1b, neg(t4), y3);                                                          // n
    r.y = mul2(t1b, z3, y3, t0b);                                                              // n
    r.z = mul2(z3, t4, t0b, t3);                                                               // n
    return r;
}

DR_DEV K1Point k1_cneg(const K1Point& p, bool negate) {
    K1Point r = p;
    r.y = carry(cneg(p.y, negate));
    return r;
}

// k mod n for a 256-bit k: 2 n > 2^256, so one conditional subtraction (in every lane)
DR_DEV void k1_load_scalar(const uint32_t* p, uint32_t (&k)[8]) {
    wave_load8(p, k);
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = subb(k[i], FsecpConsts::NW[i], borrow);
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = borrow ? k[i] : d[i];
}
// words below p?
DR_DEV bool k1_below_p(const uint32_t (&w)[8]) {
    uint32_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) (void)subb(w[j], FsecpConsts::PW[j], borrow);
    return borrow != 0;
}
// y^2 = x^3 + 7: ok and a root (either one) if it exists (y = 0 cannot happen: -7 is not a cube mod p)
DR_DEV bool k1_y_of_x(const FK& x, FK& y) { return fk_sqrt(carry(add(mul(sqr(x), x), FK::small(7))), y); }

// wave_curve.hip.h's description of secp256k1: canonical words at the ABI (64 zero bytes: the identity), the limb images of the
// (normal) coordinates in the LDS table (27 words a point: no packing), 65 windows (n has 256 bits)
struct Secp256k1Curve {
    using Fe = FK;
    using Point = K1Point;
    static constexpr int WORDS = 8, SCALAR_WORDS = 8, BLOCK = K1_BLOCK, WINDOWS = 65, LDS_WORDS = 9;
    static constexpr bool EXTENDED = false, ZERO_IS_IDENTITY = true;
    DR_DEV static FK unpack(const uint32_t (&w)[8]) { return fk_unpack(w); }
    DR_DEV static void pack(const FK& a, uint32_t (&w)[8]) { fk_pack(a, w); }
    DR_DEV static FK inv(const FK& a) { return fk_inv(a); }
    DR_DEV static void to_lds(const FK& a, uint32_t (&w)[9]) { wave_limbs_to_words(a, w); }
    DR_DEV static FK from_lds(const uint32_t (&w)[9]) { return wave_words_to_limbs<FK>(w); }
    DR_DEV static K1Point identity() { return k1_identity(); }
    DR_DEV static K1Point from_affine(const FK& x, const FK& y) {
        K1Point P;
        P.x = x; P.y = y; P.z = FK::small(1);
        return P;
    }
    DR_DEV static K1Point add(const K1Point& p, const K1Point& q) { return k1_add(p, q); }
    DR_DEV static K1Point dbl(const K1Point& p) { return k1_dbl(p); }
    DR_DEV static K1Point cneg(const K1Point& p, bool negate) { return k1_cneg(p, negate); }
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[8]) { k1_load_scalar(p, k); }
    DR_DEV static bool below_p(const uint32_t (&w)[8]) { return k1_below_p(w); }
    DR_DEV static bool y_of_x(const FK& x, FK& y) { return k1_y_of_x(x, y); }
    DR_DEV static bool is_odd(const FK& x) { return dr::is_odd(x); }
};

// out[i] = k[i] P[i]: wave_curve.hip.h's kernel bodies for this curve
__global__ __launch_bounds__(K1_BLOCK) void k_secp256k1_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                   uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<Secp256k1Curve>(pts, ks, out, n);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j]
__global__ __launch_bounds__(K1_BLOCK) void k_secp256k1_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                   uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<Secp256k1Curve>(pts, ks, out, groups, m, mpad);
}
// the bucket method from NARROW_PIP_FROM terms on (wave_msm.hip.h): the stages over Secp256k1Curve, set sums out as affine x || y
DR_WAVE_MSM_KERNELS(secp256k1, Secp256k1Curve)

// Decoding (the reference's SWAffinePoint.string_to_point for a compressed string), one lane per 33-byte SEC1 encoding padded to 9
// words (bytes 33..35 zero): byte 0 is 0x02 or 0x03, x = bytes 1..32 BIG-endian, x < p, x^3 + 7 a square, y the root of byte 0's
// parity.  No string encodes the identity, so K1_DEC_CODEC (the codec alone) and K1_DEC_CHECK (also not the identity; the cofactor is
// 1, so that is all valid_point asks) accept the same strings; both exist because the shared host templates name both.  There is no
// try-and-increment mode: these suites hash to the curve with k_secp256k1_map_to_curve.
enum { K1_DEC_CODEC = 0, K1_DEC_CHECK = 1 };
template <int MODE>
__global__ __launch_bounds__(K1_BLOCK) void k_secp256k1_decode_points(const uint32_t* __restrict__ enc /* n*9 */, uint32_t* __restrict__ out_xy /* n*16 */,
                                                                      uint32_t* __restrict__ ok, uint32_t n) {
    sec1_decode<Secp256k1Curve>(enc, out_xy, ok, n);
}

// ---------------------------------------------------------------- hashing to the curve: simplified SWU and an isogeny (RFC 9380)
// The map itself is sswu.hip.h, a template over a description of the target curve; this is secp256k1's.  E': y^2 = x^3 + A x + B with
// B and |Z| small (Z negative), sqrt(-Z), and the isogeny E' -> E as four coefficient lists, highest degree first (the leading 1 of
// the denominators is implied), all as compile-time limbs — nothing is indexed at run time, so nothing goes to scratch.  P-256, whose
// SSWU needs no isogeny, has its description (ISOGENY = false) in kernels_p256.hip.h.
struct Secp256k1Sswu : Secp256k1Curve {
    static constexpr bool ISOGENY = true;
    static constexpr uint32_t B = 1771, NEG_Z = 11;
    static constexpr uint32_t A[9] = {0x1a444533u, 0x02a23e00u, 0x1bc39750u, 0x07a6c796u, 0x1d272e95u, 0x0aac787au, 0x0b728229u, 0x157bacc3u, 0x003f8731u};
    static constexpr uint32_t SQRT_NEG_Z[9] = {0x103c4a59u, 0x03394e41u, 0x11e2774au, 0x109e014eu, 0x02afeec1u, 0x1fd9c7c2u, 0x0f95eb44u, 0x004e4802u, 0x0031fdf3u};
    // RFC 9380 appendix E.1: x_num k_(1,3..0), x_den k_(2,1..0), y_num k_(3,3..0), y_den k_(4,2..0)
    static constexpr uint32_t XN3[9] = {0x0aaaa88cu, 0x11c71c6du, 0x038e38e3u, 0x071c71c7u, 0x0e38e38eu, 0x1c71c71cu, 0x18e38e38u, 0x11c71c71u, 0x008e38e3u};
    static constexpr uint32_t XN2[9] = {0x1d9dd262u, 0x165e85a9u, 0x1f100c53u, 0x00c28806u, 0x1caece45u, 0x09ef6512u, 0x139b8a90u, 0x11a47e46u, 0x00534c32u};
    static constexpr uint32_t XN1[9] = {0x117c6581u, 0x1ff88227u, 0x1d8ee4b7u, 0x0ba5f817u, 0x144c5d59u, 0x0ae753feu, 0x0756e7ccu, 0x19017864u, 0x0007d3d4u};
    static constexpr uint32_t XN0[9] = {0x0aaaa8c7u, 0x11c71c6du, 0x038e38e3u, 0x071c71c7u, 0x0e38e38eu, 0x1c71c71cu, 0x18e38e38u, 0x11c71c71u, 0x008e38e3u};
    static constexpr uint32_t XD1[9] = {0x0a8c6d14u, 0x0952b309u, 0x17906ef1u, 0x06d6c83eu, 0x0225406du, 0x196a8daau, 0x1077df12u, 0x1ec8707bu, 0x00edadc6u};
    static constexpr uint32_t XD0[9] = {0x181eb49bu, 0x1f35ba2bu, 0x1e121f67u, 0x1a812a85u, 0x040dd86cu, 0x0665dbdbu, 0x062a728du, 0x0327b292u, 0x00d35771u};
    static constexpr uint32_t YN3[9] = {0x18e38d84u, 0x05ed0979u, 0x1684bda1u, 0x025ed097u, 0x0f684bdau, 0x1425ed09u, 0x12f684bdu, 0x1b425ed0u, 0x002f684bu};
    static constexpr uint32_t YN2[9] = {0x1ecee931u, 0x1b2f42d4u, 0x0f880629u, 0x10614403u, 0x0e576722u, 0x04f7b289u, 0x09cdc548u, 0x08d23f23u, 0x0029a619u};
    static constexpr uint32_t YN1[9] = {0x001d71a3u, 0x1fe487e1u, 0x01b69bf7u, 0x15608dadu, 0x0a6d5647u, 0x12a58950u, 0x103ea742u, 0x065ab96fu, 0x00c75e0cu};
    static constexpr uint32_t YN0[9] = {0x0e38e23cu, 0x097b425cu, 0x1da12f68u, 0x1097b425u, 0x0bda12f6u, 0x0d097b42u, 0x04bda12fu, 0x1ed097b4u, 0x004bda12u};
    static constexpr uint32_t YD2[9] = {0x1fd2a76fu, 0x1dfc0c95u, 0x0358a669u, 0x1a422c5eu, 0x0337e0a3u, 0x061fd47fu, 0x08b3ce9cu, 0x0e2ca8b9u, 0x006484aau};
    static constexpr uint32_t YD1[9] = {0x085c2573u, 0x1da12e93u, 0x1a365e37u, 0x0f837f91u, 0x0c298946u, 0x13319391u, 0x127f57a7u, 0x097717b6u, 0x007a0653u};
    static constexpr uint32_t YD0[9] = {0x1ffff93bu, 0x1ffffff7u, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x1fffffffu, 0x00ffffffu};
    // the field's forms of what sswu.hip.h asks for beyond Secp256k1Curve: B and |Z| are small here, so their products are mul_small
    DR_DEV static FK a() { return FK::constant<A>(); }
    DR_DEV static FK z() { return FK::small(-(int32_t)NEG_Z); }
    DR_DEV static FK sqrt_neg_z() { return FK::constant<SQRT_NEG_Z>(); }
    DR_DEV static FK one() { return FK::small(1); }
    DR_DEV static FK mul_neg_z(const FK& x) { return mul_small(x, NEG_Z); }
    DR_DEV static FK mul_b(const FK& x) { return mul_small(x, B); }
    DR_DEV static FK norm(const FK& x) { return carry(x); }
    DR_DEV static bool is_zero(const FK& x) { return dr::is_zero(x); }
    DR_DEV static bool equal(const FK& x, const FK& y) { return dr::equal(x, y); }
    DR_DEV static FK pow_p34(const FK& x) { return fk_pow_p34(x); }
};

// out[i] = the sum of the images of item i's `per_item` field elements: sswu.hip.h's map, isogeny and loop for this curve
__global__ __launch_bounds__(K1_BLOCK) void k_secp256k1_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy,
                                                                     uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item) {
    sswu_map_to_curve<Secp256k1Sswu>(us, out_xy, ok, n, per_item);
}

// Diagnostic (dr_secp256k1_field_selftest): fsecp256k1.hip.h's operations on raw limb images, one lane per (a, b) pair of 9 int32 limbs
// each, so that tests can drive every operation at the limb bounds its contract allows.  out[i] = twelve canonical 32-byte records:
// a b, a^2, a + b, a - b, -a, carry(a), a b + b a (mul2), a^-1 (0 for 0), sqrt(a) or 0, a itself (pack), 21 a (mul_small),
// sqr(carry(a)) (the fused case fk_fold_top's note is about).  flags[i]: bit 0 a is a square, bit 1 the canonical a is odd.
constexpr int K1_SELFTEST_RECORDS = 12;
__global__ __launch_bounds__(64) void k_secp256k1_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                                uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    FK a, b;
#pragma unroll
    for (int t = 0; t < LIMBS29; t++) { a.l[t] = a_limbs[(size_t)i * LIMBS29 + t]; b.l[t] = b_limbs[(size_t)i * LIMBS29 + t]; }
    uint32_t* o = out + (size_t)i * K1_SELFTEST_RECORDS * 8;
    wave_store_fe<Secp256k1Curve>(o + 0, mul(a, b));
    wave_store_fe<Secp256k1Curve>(o + 8, sqr(a));
    wave_store_fe<Secp256k1Curve>(o + 16, add(a, b));
    wave_store_fe<Secp256k1Curve>(o + 24, sub(a, b));
    wave_store_fe<Secp256k1Curve>(o + 32, neg(a));
    wave_store_fe<Secp256k1Curve>(o + 40, carry(a));
    wave_store_fe<Secp256k1Curve>(o + 48, mul2(a, b, b, a));
    wave_store_fe<Secp256k1Curve>(o + 56, fk_inv(carry(a)));
    FK r;
    const bool sq = fk_sqrt(carry(a), r);
    wave_store_fe<Secp256k1Curve>(o + 64, r);
    uint32_t w[8];
    fk_pack(a, w);
    wave_store8(o + 72, w);
    wave_store_fe<Secp256k1Curve>(o + 80, mul_small(a, K1_B3));
    wave_store_fe<Secp256k1Curve>(o + 88, sqr(carry(a)));
    flags[i] = (sq ? 1u : 0u) | ((w[0] & 1u) ? 2u : 0u);
}

// Diagnostic (dr_secp256k1_law_selftest): wave_curve.hip.h's wave_law_selftest over Secp256k1Curve, the law on raw limb images
__global__ __launch_bounds__(64) void k_secp256k1_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<Secp256k1Curve>(pts, ctl, n, out);
}

}  // namespace dr
