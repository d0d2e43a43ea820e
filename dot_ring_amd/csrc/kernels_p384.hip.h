// P-384 kernels (DR_CURVE_P384_RO / DR_CURVE_P384_NU; the reference's specs/p384.py): the complete a = -3 law of p384_law.hip.h over
// GF(2^384 - 2^128 - 2^96 + 2^32 - 1) (fp384.hip.h, Montgomery form) under the kernels every suite has: scalar multiplication on a fixed
// schedule, grouped MSMs, RFC 9380's simplified SWU map straight onto the curve (sswu.hip.h's sswu_map, no isogeny), a SEC1 decoder and
// a diagnostic of the field.
//
// Points cross the ABI as affine x || y, 12 + 12 words little-endian, canonical; 96 zero bytes are the identity, in and out ((0, 0) is
// not on the curve: b != 0).  A coordinate is 48 bytes, three uint4, so points move coordinate by coordinate as BLS12-381 G1's do, and
// 49-byte SEC1 strings go through wave_curve.hip.h's sec1_decode as its do.  Scalars are 48 bytes used AS THEY ARE: every 384-bit value
// has its 97 windows, so the host refuses none.
//
// The schedule, the memory forms and the two kernel bodies are wave_curve.hip.h's over P384Curve: 12 scalar words, 97 windows (96 digits
// and the carry out of the top one).  The table keeps limb images: 8 x 3 x 14 words x 64 lanes x 4 = 86 016 bytes of the CU's 160 KiB,
// one workgroup (one wave) per CU.
#pragma once
#include "p384_law.hip.h"
#include "sswu.hip.h"
#include "wave_curve.hip.h"
#include "wave_msm.hip.h"

namespace dr {

constexpr int P384_BLOCK = 64;        // one wave per workgroup
constexpr int P384_PT_WORDS = 2 * W384;

// wave_curve.hip.h's description of P-384: canonical words at the ABI (12 per coordinate; 96 zero bytes: the identity, which has Z = 0
// and so stores them by 0^-1 = 0), the limb images (Montgomery form) in the LDS table, and 97 windows over the scalar AS IT IS.  The
// law members are sw3_law.hip.h's Sw3Curve.
struct P384Curve : Sw3Curve<P384Sw3> {
    static constexpr int SCALAR_WORDS = W384, BLOCK = P384_BLOCK, WINDOWS = P384_WINDOWS;
    DR_DEV static F384 inv(const F384& a) { return dr::inv(a); }     // n; stays here: Limb28Curve supplies no inv
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[W384]) { wave_load_words(p, k); }    // no reduction
    // for sec1_decode: a root of x^3 - 3 x + b (n - 3 n + n, carried), the range of x and the parity of the canonical y
    DR_DEV static bool below_p(const uint32_t (&w)[W384]) { return dr::below_p(w); }
    DR_DEV static bool y_of_x(const F384& x, F384& y) {
        const F384 x3 = mul(sqr(x), x);
        const F384 x_3 = dr::add(x, dr::dbl(x));             // (dr::: the description's own add and dbl are the points')
        return f384_sqrt(carry(dr::add(sub(x3, x_3), P384Sw3::b())), y);
    }
    DR_DEV static bool is_odd(const F384& y) { return dr::is_odd(y); }
};

// out[i] = k[i] P[i].  pts: n x 24 words (x || y), ks: n x 12, out: n x 24.  One lane per multiplication.
__global__ __launch_bounds__(P384_BLOCK) void k_p384_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<P384Curve>(pts, ks, out, n);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64 padded to mpad: one lane per term, folded with shuffles by the complete addition
__global__ __launch_bounds__(P384_BLOCK) void k_p384_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<P384Curve>(pts, ks, out, groups, m, mpad);
}


// ---------------------------------------------------------------- the bucket method (dr_wide_msm): wave_msm.hip.h over P384Curve
// One MSM of n >= WIDE_PIP_FROM terms; the stages, their operands and the plan are that header's.  W384 scalar words, as they are; the
// set sums leave as records of limb images (k_p384_msm_prepare, _sort, _accumulate, _accumulate_heavy, _reduce, _fold).
DR_WAVE_MSM_KERNELS_RECORDS(p384, P384Curve)

// ---------------------------------------------------------------- hashing to the curve (RFC 9380, P384_XMD:SHA-384_SSWU_RO_ / _NU_)
// (the map's description, P384Sswu, is p384_law.hip.h's.  The body below and k_p521_map_to_curve's are the same text and stay two: as
// one template over the two descriptions both kernels change)
// out[i] = the sum of the images of item i's `per_item` field elements (2: the uniform (RO) encoding, 1: the nonuniform one).  us: n x
// per_item x 12 words (canonical, checked by the host), out: n x 24 words affine x || y (96 zero bytes if the two images cancel),
// ok[i] = 1 always: the map has no isogeny and no denominator that can vanish (its exceptional branch, u in {0, s, p - s} with
// s^2 = 1 / 12, lands on x1 = B / (Z A), a point).  The cofactor is 1, so `clear` changes nothing; the parameter is the suites' common
// signature.  One lane per item; one exponentiation per element and one inversion per item.
__global__ __launch_bounds__(P384_BLOCK) void k_p384_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy,
                                                                  uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item, uint32_t clear) {
    (void)clear;
    uint32_t i = blockIdx.x * P384_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    P384Point acc = p384_identity();
    bool good = true;
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++) {
        uint32_t w[W384];
        wave_load_words(us + ((size_t)i * per_item + e) * W384, w);
        F384 xn, xd, y;
        sswu_map<P384Sswu>(unpack(w), (w[0] & 1u) != 0, xn, xd, y);
        bool ok_e;
        const P384Point pt = sswu_iso_map<P384Sswu>(xn, xd, y, ok_e);        // (xn : y xd : xd): n, n, n
        good = good && ok_e;
        acc = p384_add(acc, pt);
    }
    if (live) {
        wave_store_affine<P384Curve>(out_xy + (size_t)i * P384_PT_WORDS, acc);
        ok[i] = good ? 1u : 0u;
    }
}

// ---------------------------------------------------------------- SEC1 compressed points
// One lane per SEC1 compressed encoding (49 bytes padded to 13 words): wave_curve.hip.h's sec1_decode over P384Curve.  No string
// encodes the identity and the cofactor is 1, so the codec alone (check = 0) and the checking decoder (check = 1) are this one kernel.
// out = x || y and ok = 1, or 96 zero bytes and ok = 0.
__global__ __launch_bounds__(P384_BLOCK) void k_p384_decode_points(const uint32_t* __restrict__ enc /* n*13 */, uint32_t* __restrict__ out_xy /* n*24 */,
                                                                   uint32_t* __restrict__ ok, uint32_t n) {
    sec1_decode<P384Curve>(enc, out_xy, ok, n);
}

// Diagnostic (dr_p384_field_selftest): fp384.hip.h's operations on RAW limb images, one lane per (a, b) pair of 14 int32 limbs each, so
// that tests can drive every operation at the limb bounds its contract allows (a <= 2 n for the square, ka kb <= 8 for the product).  An
// image stands for its value times 2^-392 mod p.  out[i] = thirteen canonical 48-byte records: a b, a^2, a + b, a - b, -a, carry(a), 4 a,
// a^-1 (0 for 0), carry(a)^((p + 1) / 4) (a root of a when a is a square), a itself (pack), -(2^28 - 1) a, carry(a)^2 (a square whose
// operand is the fold's output) and mul2(carry(a), b, a, carry(b)) = 2 a b;  flags[i]: bit 0 a is a square, bit 1 the canonical a is odd,
// bit 2 a is zero, bit 3 a = b.
constexpr int P384_SELFTEST_RECORDS = 13;
__global__ __launch_bounds__(64) void k_p384_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                           uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F384 a, b;
#pragma unroll
    for (int t = 0; t < L384; t++) { a.l[t] = a_limbs[(size_t)i * L384 + t]; b.l[t] = b_limbs[(size_t)i * L384 + t]; }   // (in place: DESIGN.md section 8x)
    uint32_t* o = out + (size_t)i * P384_SELFTEST_RECORDS * W384;
    auto put = [&](int r, const F384& v) { field_selftest_put(o, r, v); };
    const F384 ca = carry(a);
    put(0, mul(a, b));
    put(1, sqr(a));
    put(2, add(a, b));
    put(3, sub(a, b));
    put(4, neg(a));
    put(5, ca);
    put(6, mul_small(a, 4));
    put(7, inv(a));
    F384 root;
    const bool sq = f384_sqrt(ca, root);
    put(8, root);
    put(9, a);
    put(10, mul_small(a, -M384));
    put(11, sqr(ca));
    put(12, mul2(ca, b, a, carry(b)));
    flags[i] = (sq ? 1u : 0u) | (is_odd(a) ? 2u : 0u) | (is_zero(a) ? 4u : 0u) | (equal(a, b) ? 8u : 0u);
}

// Diagnostic (dr_p384_law_selftest): wave_curve.hip.h's wave_law_selftest over P384Curve, the law on raw limb images
__global__ __launch_bounds__(64) void k_p384_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<P384Curve>(pts, ctl, n, out);
}

}  // namespace dr
