// P-256 kernels (DR_CURVE_P256; the reference's specs/p256.py, P256_TAI): the short Weierstrass group law with a = -3 over
// GF(p256) (fp256.hip.h) and the kernels that fill, for this curve, the roles kernels_ed25519.hip.h fills for Ed25519: variable-base
// scalar multiplication on a fixed schedule, grouped MSMs, point decoding (with the reference's SEC1 fallback) and the device half
// of try-and-increment.  The existing kernels stay as they are; no other curve includes this header's field.
//
// Points cross the ABI as affine x || y little-endian, standard form; 64 zero bytes are the identity ((0, 0) is not on the curve).
// Inside: homogeneous projective (X : Y : Z), x = X / Z, y = Y / Z, identity (0 : 1 : 0), coordinates in Montgomery form.  The
// group law is the complete one of Renes, Costello and Batina (2016), algorithms 4 (addition) and 6 (doubling) for a = -3: no
// exceptional cases (P + P, P + (-P), the identity on either side) and no branches.  The comments give the limb class of every
// intermediate against fp256.hip.h's contract: n = normal, r = reduced, sK = a sum or difference of K such.
#pragma once
#include "fp256.hip.h"
#include "sswu.hip.h"
#include "wave_curve.hip.h"
#include "wave_msm.hip.h"

namespace dr {

constexpr int P256_BLOCK = 64;        // one wave per workgroup, as k_ed_scalar_mul

struct P256Point {
    F256 x, y, z;
};

DR_DEV P256Point p256_identity() {
    P256Point p;
    p.x = F256::zero(); p.y = fp_one(); p.z = F256::zero();
    return p;
}

// algorithm 6, a = -3 (8M + 3S + 2 products by b, here 7 products, 3 squarings and one fused pair); coordinates n or r (y possibly
// negated by p256_cneg: it meets products, squares and sums of two only) in, n out
DR_DEV P256Point p256_dbl(const P256Point& p) {
    const F256 b = F256::constant<Fp256Consts::B>();
    const F256 t0 = sqr(p.x), t1 = sqr(p.y), t2 = sqr(p.z);                    // n
    const F256 xy = mul(p.x, p.y), xz = mul(p.x, p.z), yz = mul(p.y, p.z);     // n
    const F256 xz2 = dbl(xz);                                                    // s2
    F256 y3 = fp_reduce(sub(mul(b, t2), xz2));                                   // b Z^2 - 2 X Z: r
    y3 = fp_reduce(add(y3, dbl(y3)));                                            // 3 (...): r
    const F256 xa = fp_reduce(sub(t1, y3)), ya = fp_reduce(add(t1, y3));          // Y^2 -+ y3: r
    const F256 t2b = add(t2, dbl(t2));                                           // 3 Z^2: s3
    F256 z3 = fp_reduce(sub(mul(b, xz2), t2b));                                  // 2 b X Z - 3 Z^2: r
    z3 = fp_reduce(sub(z3, t0));                                                 // r
    z3 = fp_reduce(add(z3, dbl(z3)));                                            // 3 (...): r
    const F256 t0b = fp_reduce(sub(add(t0, dbl(t0)), t2b));                      // 3 X^2 - 3 Z^2: r
    P256Point r;
    r.x = carry(dbl(mul2(xy, xa, neg(yz), z3)));                                 // 2 X Y xa - 2 Y Z z3: n
    r.y = mul2(xa, ya, t0b, z3);                                                 // xa ya + t0b z3: n
    r.z = mul(carry(dbl(carry(dbl(yz)))), dbl(t1));                              // 4 Y Z x 2 Y^2 = 8 Y^3 Z: n
    return r;
}

// algorithm 4, a = -3 (12M + 2 products by b; here 8 products and 3 fused pairs); coordinates n or r (y possibly negated by
// p256_cneg, in either point) in, n out
DR_DEV P256Point p256_add(const P256Point& p, const P256Point& q) {
    const F256 b = F256::constant<Fp256Consts::B>();
    const F256 t0 = mul(p.x, q.x), t1 = mul(p.y, q.y), t2 = mul(p.z, q.z);      // n
    const F256 t3 = fp_reduce(sub(mul(fp_reduce(add(p.x, p.y)), add(q.x, q.y)), add(t0, t1)));   // X1 Y2 + X2 Y1: r
    const F256 t4 = fp_reduce(sub(mul(fp_reduce(add(p.y, p.z)), add(q.y, q.z)), add(t1, t2)));   // Y1 Z2 + Y2 Z1: r
    const F256 u = sub(mul(fp_reduce(add(p.x, p.z)), add(q.x, q.z)), add(t0, t2));              // X1 Z2 + X2 Z1: s3
    const F256 x3a = fp_reduce(sub(u, mul(b, t2)));                              // u - b t2: r
    const F256 x3b = fp_reduce(add(x3a, dbl(x3a)));                              // 3 (...): r
    const F256 z3 = fp_reduce(sub(t1, x3b)), x3 = fp_reduce(add(t1, x3b));       // r
    const F256 t2b = add(t2, dbl(t2));                                           // 3 t2: s3
    F256 y3 = fp_reduce(sub(mul(b, u), t2b));                                    // b u - 3 t2: r
    y3 = fp_reduce(sub(y3, t0));                                                 // r
    y3 = fp_reduce(add(y3, dbl(y3)));                                            // 3 (...): r
    const F256 t0b = fp_reduce(sub(add(t0, dbl(t0)), t2b));                      // 3 t0 - 3 t2: r
    P256Point r;
    r.x = mul2(x3, t3, neg(t4), y3);                                             // n
    r.y = mul2(x3, z3, t0b, y3);                                                 // n
    r.z = mul2(t4, z3, t3, t0b);                                                 // n
    return r;
}

DR_DEV P256Point p256_cneg(const P256Point& p, bool negate) {
    P256Point r = p;
    r.y = cneg(p.y, negate);
    return r;
}

// k mod n for a 256-bit k: 2 n > 2^256, so one conditional subtraction (in every lane)
DR_DEV void p256_load_scalar(const uint32_t* p, uint32_t (&k)[8]) {
    constexpr uint32_t N[8] = {0xfc632551u, 0xf3b9cac2u, 0xa7179e84u, 0xbce6faadu, 0xffffffffu, 0xffffffffu, 0x00000000u, 0xffffffffu};
    wave_load8(p, k);
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int i = 0; i < 8; i++) d[i] = subb(k[i], N[i], borrow);
#pragma unroll
    for (int i = 0; i < 8; i++) k[i] = borrow ? k[i] : d[i];
}
// y^2 = x^3 - 3 x + b for x in Montgomery form; ok and a root (either one) if it exists
DR_DEV bool p256_y_of_x(const F256& x, F256& y) {
    const F256 x3 = mul(sqr(x), x);
    const F256 rhs = fp_reduce(add(sub(x3, add(x, dbl(x))), F256::constant<Fp256Consts::B>()));     // n - s3 + n: r
    return fp_sqrt(rhs, y);
}
// words below p?
DR_DEV bool p256_below_p(const uint32_t (&w)[8]) {
    uint32_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) (void)subb(w[j], Fp256Consts::PW[j], borrow);
    return borrow != 0;
}

// wave_curve.hip.h's description of P-256: standard-form words at the ABI (64 zero bytes: the identity), Montgomery limbs inside, the
// limb images of the (normal) coordinates in the LDS table (27 words a point: no packing), 65 windows (n has 256 bits)
struct P256Curve {
    using Fe = F256;
    using Point = P256Point;
    static constexpr int WORDS = 8, SCALAR_WORDS = 8, BLOCK = P256_BLOCK, WINDOWS = 65, LDS_WORDS = 9;
    static constexpr bool EXTENDED = false, ZERO_IS_IDENTITY = true;
    DR_DEV static F256 unpack(const uint32_t (&w)[8]) { return fp_unpack(w); }
    DR_DEV static void pack(const F256& a, uint32_t (&w)[8]) { fp_pack(a, w); }
    DR_DEV static F256 inv(const F256& a) { return fp_inv(a); }
    DR_DEV static void to_lds(const F256& a, uint32_t (&w)[9]) { wave_limbs_to_words(a, w); }
    DR_DEV static F256 from_lds(const uint32_t (&w)[9]) { return wave_words_to_limbs<F256>(w); }
    DR_DEV static P256Point identity() { return p256_identity(); }
    DR_DEV static P256Point from_affine(const F256& x, const F256& y) {
        P256Point P;
        P.x = x; P.y = y; P.z = fp_one();
        return P;
    }
    DR_DEV static P256Point add(const P256Point& p, const P256Point& q) { return p256_add(p, q); }
    DR_DEV static P256Point dbl(const P256Point& p) { return p256_dbl(p); }
    DR_DEV static P256Point cneg(const P256Point& p, bool negate) { return p256_cneg(p, negate); }
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[8]) { p256_load_scalar(p, k); }
    DR_DEV static bool below_p(const uint32_t (&w)[8]) { return p256_below_p(w); }
    DR_DEV static bool y_of_x(const F256& x, F256& y) { return p256_y_of_x(x, y); }
    DR_DEV static bool is_odd(const F256& x) { return dr::is_odd(x); }
};

// out[i] = k[i] P[i]: wave_curve.hip.h's kernel bodies for this curve
__global__ __launch_bounds__(P256_BLOCK) void k_p256_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<P256Curve>(pts, ks, out, n);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j]
__global__ __launch_bounds__(P256_BLOCK) void k_p256_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<P256Curve>(pts, ks, out, groups, m, mpad);
}
// the bucket method from NARROW_PIP_FROM terms on (wave_msm.hip.h): the stages over P256Curve, set sums out as affine x || y
DR_WAVE_MSM_KERNELS(p256, P256Curve)

// Decoding (the reference's P256Point.string_to_point / _string_to_canonical_point and, for strings that start with 0x02 or 0x03,
// SWAffinePoint.string_to_point as the fallback), one lane per 33-byte encoding padded to 9 words (bytes 33..35 zero):
//   canonical: x = bytes 0..31 little-endian, flag = byte 32; flag bits 0..5 set -> rejected; bit 6 (infinity): the identity iff
//              x = 0 and bit 7 clear, otherwise rejected; else x < p and x^3 - 3 x + b a square, y the larger root iff bit 7;
//   fallback : when byte 0 is 0x02 or 0x03 and the canonical decoding failed: x = bytes 1..32 BIG-endian (the flag byte included),
//              x < p and a root, y of the parity byte 0 & 1 (SEC1 compressed).
// MODE: P256_DEC_CODEC the codec alone (the identity is accepted, out = 64 zero bytes); P256_DEC_CHECK also rejects the identity
// (the cofactor is 1: a decoded point other than O is a valid point); P256_DEC_TAI the device half of try-and-increment, whose
// candidates (32 squeezed bytes and the flag 0x80) are accepted on the same terms — no cofactor to clear, so it is CHECK again.
// P256_DEC_SEC1: the codec of the RFC 9380 variants (P256_RO / P256_NU: SWAffinePoint.string_to_point), plain SEC1 compressed as
// k_secp256k1_decode_points reads it — byte 0 is 0x02 or 0x03, x = bytes 1..32 big-endian, x < p, a root, y of byte 0's parity; nothing
// else, so a P256_TAI string is read as SEC1 or refused, never by the canonical rules.  No string encodes the identity, so the codec
// alone and the checking decoder are this one mode.
enum { P256_DEC_CODEC = 0, P256_DEC_CHECK = 1, P256_DEC_TAI = 2, P256_DEC_SEC1 = 3 };
template <int MODE>
__global__ __launch_bounds__(P256_BLOCK) void k_p256_decode_points(const uint32_t* __restrict__ enc /* n*9 */, uint32_t* __restrict__ out_xy /* n*16 */,
                                                                   uint32_t* __restrict__ ok, uint32_t n) {
    if constexpr (MODE == P256_DEC_SEC1) {
        sec1_decode<P256Curve>(enc, out_xy, ok, n);
        return;
    }
    uint32_t i = blockIdx.x * P256_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t w[9];
#pragma unroll
    for (int j = 0; j < 9; j++) w[j] = enc[(size_t)i * 9 + j];
    const uint32_t flag = w[8] & 0xffu, first = w[0] & 0xffu;
    uint32_t xs[8];
#pragma unroll
    for (int j = 0; j < 8; j++) xs[j] = w[j];
    // canonical
    uint32_t xzero = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) xzero |= xs[j];
    const bool infinity = (flag & 0x40u) != 0, larger = (flag & 0x80u) != 0;
    bool valid = (flag & 0x3fu) == 0 && p256_below_p(xs);
    bool is_identity = false;
    F256 x = fp_unpack(xs), y;
    const bool root = p256_y_of_x(x, y);
    if (infinity) {
        is_identity = valid && xzero == 0 && !larger;
        valid = is_identity;
    } else {
        valid = valid && root;
    }
    uint32_t yw[8];
    fp_pack(y, yw);
    bool want_larger = larger, by_parity = false;
    // the SEC1 fallback: x = BE(bytes 1..32)
    if (!valid && (first == 0x02u || first == 0x03u)) {
        uint32_t xb[8];
        sec1_x_words(w, xb);
        x = fp_unpack(xb);
        valid = p256_below_p(xb) && p256_y_of_x(x, y);
        fp_pack(y, yw);
        by_parity = true;
        is_identity = false;
    }
    // choose the root: the larger iff the flag's bit 7 (canonical), the parity of byte 0 (SEC1)
    const bool flip = by_parity ? ((yw[0] & 1u) != (first & 1u)) : (is_larger_words<Fp256Consts>(yw) != want_larger);
    if (flip) y = neg(y);
    if constexpr (MODE != P256_DEC_CODEC) valid = valid && !is_identity;
    if (live) {
        if (valid && !is_identity) {
            wave_store_fe<P256Curve>(out_xy + (size_t)i * 16, x);
            wave_store_fe<P256Curve>(out_xy + (size_t)i * 16 + 8, y);
        } else {
            wave_store_zero8(out_xy + (size_t)i * 16);
            wave_store_zero8(out_xy + (size_t)i * 16 + 8);
        }
        ok[i] = valid ? 1u : 0u;
    }
}

// ---------------------------------------------------------------- hashing to the curve (RFC 9380, P256_XMD:SHA-256_SSWU_RO_ / _NU_)
// sswu.hip.h's description of P-256: the simplified SWU map straight onto the curve (A = -3, B = b, Z = -10, no isogeny).  The field is
// in Montgomery form, so A, Z, |Z| = 10 and sqrt(-Z) = sqrt(10) are compile-time limbs of v 2^261 mod p, B is Fp256Consts::B, and the
// products by |Z| and B are full products by those constants (neither is small in this form).  sgn0 and equality are taken on the
// canonical value (fp_pack).  The field, the point, its addition and the ABI forms are P256Curve's.
struct P256Sswu : P256Curve {
    static constexpr bool ISOGENY = false;
    static constexpr uint32_t A[9] = {0x1fffff9fu, 0x1fffffffu, 0x1fffffffu, 0x0000c1ffu, 0x00000000u, 0x00000000u, 0x01840000u, 0x13e00000u, 0x00ffffffu};
    static constexpr uint32_t Z[9] = {0x1ffffebfu, 0x1fffffffu, 0x1fffffffu, 0x000281ffu, 0x00000000u, 0x00000000u, 0x05040000u, 0x17e00000u, 0x00fffffeu};
    static constexpr uint32_t NEG_Z[9] = {0x00000140u, 0x00000000u, 0x00000000u, 0x1ffd8000u, 0x1fffffffu, 0x1fffffffu, 0x1affffffu, 0x07ffffffu, 0x00000001u};
    static constexpr uint32_t SQRT_NEG_Z[9] = {0x1432bfb2u, 0x1d38ee98u, 0x0e7b850fu, 0x02b5ac8fu, 0x1fdcf080u, 0x08f9ea8du, 0x01ec89e4u, 0x1a8aa3ccu, 0x000a3a4du};
    DR_DEV static F256 a() { return F256::constant<A>(); }
    DR_DEV static F256 z() { return F256::constant<Z>(); }
    DR_DEV static F256 sqrt_neg_z() { return F256::constant<SQRT_NEG_Z>(); }
    DR_DEV static F256 one() { return fp_one(); }
    DR_DEV static F256 mul_neg_z(const F256& x) { return mul(F256::constant<NEG_Z>(), x); }            // n x (n or s2): n
    DR_DEV static F256 mul_b(const F256& x) { return mul(F256::constant<Fp256Consts::B>(), x); }
    DR_DEV static F256 norm(const F256& x) { return fp_reduce(x); }
    DR_DEV static bool is_zero(const F256& x) { return dr::is_zero(x); }
    DR_DEV static bool equal(const F256& x, const F256& y) { return dr::equal(x, y); }
    DR_DEV static F256 pow_p34(const F256& x) { return fp_pow_p34(x); }
};
// out[i] = the sum of the images of item i's `per_item` (1: NU, 2: RO) field elements, as k_secp256k1_map_to_curve: us n x per_item x 8
// words (canonical, checked by the host), out n x 16 words affine x || y (64 zero bytes if the two images cancel), ok[i] = 1 always
// (no isogeny, no denominator that can vanish).  One lane per item.
__global__ __launch_bounds__(P256_BLOCK) void k_p256_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy,
                                                                  uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item) {
    sswu_map_to_curve<P256Sswu>(us, out_xy, ok, n, per_item);
}

// Diagnostic (dr_p256_field_ops_selftest): fp256.hip.h's operations on raw limb images, one lane per (a, b) pair of 9 int32 limbs each
// (Montgomery images: the element of an image is its value times 2^-261 mod p), so that tests can drive every operation at the limb
// bounds its contract allows.  out[i] = ten canonical 32-byte records: a b, a^2, a + b, a - b, -a, carry(a), a b + b a (mul2),
// a^-1 (0 for 0), sqrt(a) or 0, a itself (pack); then reduce(a) (record 10) and sqr(reduce(a)) (record 11, the case fp_reduce's
// note in fp256.hip.h is about).  flags[i]: bit 0 a is a square, bit 1 a > p - a,
// bit 2 the canonical a is odd.
constexpr int P256_SELFTEST_RECORDS = 12;
__global__ __launch_bounds__(64) void k_p256_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                           uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F256 a, b;
#pragma unroll
    for (int t = 0; t < LIMBS29; t++) { a.l[t] = a_limbs[(size_t)i * LIMBS29 + t]; b.l[t] = b_limbs[(size_t)i * LIMBS29 + t]; }
    uint32_t* o = out + (size_t)i * P256_SELFTEST_RECORDS * 8;
    wave_store_fe<P256Curve>(o + 0, mul(a, b));
    wave_store_fe<P256Curve>(o + 8, sqr(a));
    wave_store_fe<P256Curve>(o + 16, add(a, b));
    wave_store_fe<P256Curve>(o + 24, sub(a, b));
    wave_store_fe<P256Curve>(o + 32, neg(a));
    wave_store_fe<P256Curve>(o + 40, carry(a));
    wave_store_fe<P256Curve>(o + 48, mul2(a, b, b, a));
    wave_store_fe<P256Curve>(o + 56, fp_inv(a));
    F256 r;
    const bool sq = fp_sqrt(a, r);
    wave_store_fe<P256Curve>(o + 64, r);
    uint32_t w[8];
    fp_pack(a, w);
    wave_store8(o + 72, w);
    wave_store_fe<P256Curve>(o + 80, fp_reduce(a));
    wave_store_fe<P256Curve>(o + 88, sqr(fp_reduce(a)));
    flags[i] = (sq ? 1u : 0u) | (is_larger_words<Fp256Consts>(w) ? 2u : 0u) | ((w[0] & 1u) ? 4u : 0u);
}

// Diagnostic (dr_p256_law_selftest): wave_curve.hip.h's wave_law_selftest over P256Curve, the law on raw limb images
__global__ __launch_bounds__(64) void k_p256_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<P256Curve>(pts, ctl, n, out);
}

}  // namespace dr
