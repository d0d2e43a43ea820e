// P-521 kernels (DR_CURVE_P521_RO / DR_CURVE_P521_NU; the reference's specs/p521.py): the complete a = -3 law of p521_law.hip.h over
// GF(2^521 - 1) (fp521.hip.h) under the kernels every suite has: scalar multiplication on a fixed schedule, grouped MSMs, RFC 9380's
// simplified SWU map straight onto the curve (sswu.hip.h's sswu_map, no isogeny), a SEC1 decoder and a diagnostic of the field.
//
// Points cross the ABI as affine x || y, 17 + 17 words little-endian, canonical; 136 zero bytes are the identity, in and out ((0, 0) is
// not on the curve: b != 0).  A point is 136 bytes, a multiple of 8, so it moves as seventeen uint2; a 68-byte element or scalar moves
// as words.  Scalars are 68 bytes below 2^521 (the host refuses others) used AS THEY ARE.
//
// The schedule, the memory forms and the two kernel bodies are wave_curve.hip.h's over P521Curve: 17 scalar words, 131 windows
// (p521_law.hip.h: why 131 and no window for a carry out).  The table keeps limb images: 8 x 3 x 19 words x 64 lanes x 4 = 116 736
// bytes of the CU's 160 KiB, one workgroup (one wave) per CU.
#pragma once
#include "p521_law.hip.h"
#include "sswu.hip.h"
#include "wave_curve.hip.h"
#include "wave_msm.hip.h"

namespace dr {

constexpr int P521_BLOCK = 64;        // one wave per workgroup
constexpr int P521_PT_WORDS = 2 * W521;

// wave_curve.hip.h's description of P-521: canonical words at the ABI (17 per coordinate; 136 zero bytes: the identity, which has Z = 0
// and so stores them by 0^-1 = 0), the limb images in the LDS table, and 131 windows over the scalar AS IT IS (k < 2^521).  The law
// members are sw3_law.hip.h's Sw3Curve.
struct P521Curve : Sw3Curve<P521Sw3> {
    static constexpr int SCALAR_WORDS = W521, BLOCK = P521_BLOCK, WINDOWS = P521_WINDOWS;
    DR_DEV static F521 inv(const F521& a) { return dr::inv(a); }     // 1 n; stays here: Limb28Curve supplies no inv
    DR_DEV static void load_scalar(const uint32_t* p, uint32_t (&k)[W521]) { wave_load_words(p, k); }    // no reduction
};

// out[i] = k[i] P[i].  pts: n x 34 words (x || y), ks: n x 17, out: n x 34.  One lane per multiplication.
__global__ __launch_bounds__(P521_BLOCK) void k_p521_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<P521Curve>(pts, ks, out, n);
}
// out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64 padded to mpad: one lane per term, folded with shuffles by the complete addition
__global__ __launch_bounds__(P521_BLOCK) void k_p521_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<P521Curve>(pts, ks, out, groups, m, mpad);
}


// ---------------------------------------------------------------- the bucket method (dr_wide_msm): wave_msm.hip.h over P521Curve
// One MSM of n >= WIDE_PIP_FROM terms; the stages, their operands and the plan are that header's.  W521 scalar words, as they are; the
// set sums leave as records of limb images (k_p521_msm_prepare, _sort, _accumulate, _accumulate_heavy, _reduce, _fold).
DR_WAVE_MSM_KERNELS_RECORDS(p521, P521Curve)

// ---------------------------------------------------------------- hashing to the curve (RFC 9380, P521_XMD:SHA-512_SSWU_RO_ / _NU_)
// (the map's description, P521Sswu, is p521_law.hip.h's.  The body below and k_p384_map_to_curve's are the same text and stay two: as
// one template over the two descriptions both kernels change)
// out[i] = the sum of the images of item i's `per_item` field elements (2: the uniform (RO) encoding, 1: the nonuniform one).  us: n x
// per_item x 17 words (canonical, checked by the host), out: n x 34 words affine x || y (136 zero bytes if the two images cancel),
// ok[i] = 1 always: the map has no isogeny and no denominator that can vanish (its exceptional branch, u in {0, 2^520, 2^520 - 1},
// lands on x1 = B / (Z A), a point).  The cofactor is 1, so `clear` changes nothing; the parameter is the suites' common signature.
// One lane per item; one exponentiation per element and one inversion per item.
__global__ __launch_bounds__(P521_BLOCK) void k_p521_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy,
                                                                  uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item, uint32_t clear) {
    (void)clear;
    uint32_t i = blockIdx.x * P521_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    P521Point acc = p521_identity();
    bool good = true;
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++) {
        uint32_t w[W521];
        wave_load_words(us + ((size_t)i * per_item + e) * W521, w);
        F521 xn, xd, y;
        sswu_map<P521Sswu>(unpack(w), (w[0] & 1u) != 0, xn, xd, y);
        bool ok_e;
        const P521Point pt = sswu_iso_map<P521Sswu>(xn, xd, y, ok_e);        // (xn : y xd : xd): n, n, n
        good = good && ok_e;
        acc = p521_add(acc, pt);
    }
    if (live) {
        wave_store_affine<P521Curve>(out_xy + (size_t)i * P521_PT_WORDS, acc);
        ok[i] = good ? 1u : 0u;
    }
}

// ---------------------------------------------------------------- SEC1 compressed points
// x = bytes 1..66 of a 67-byte string (17 words, the last byte zero) read BIG-endian.  wave_curve.hip.h's sec1_x_words reads bytes
// 1..4 W, a whole number of words; here the top word is the two bytes 1 and 2 and the sixteen below it are the byte swaps of the
// (unaligned) words at bytes 63 - 4 q.
// (in place, with the kernel below: through sec1_decode<P521Curve> over a 66-byte x k_p521_decode_points differs)
DR_DEV void p521_sec1_x_words(const uint32_t (&w)[W521], uint32_t (&xb)[W521]) {
#pragma unroll
    for (int q = 0; q < W521 - 1; q++) {
        const int m = W521 - 2 - q;
        xb[q] = __builtin_bswap32((w[m] >> 24) | (w[m + 1] << 8));
    }
    xb[W521 - 1] = ((w[0] >> 16) & 0xffu) | (((w[0] >> 8) & 0xffu) << 8);
}
// One lane per SEC1 compressed encoding (67 bytes padded to 17 words): byte 0 is 0x02 or 0x03, x < p, x^3 - 3 x + b is a square, y the
// root of byte 0's parity (y = 0 cannot happen: the group order is odd).  No string encodes the identity and the cofactor is 1, so the
// codec alone (check = 0) and the checking decoder (check = 1) are this one kernel.  out = x || y and ok = 1, or 136 zero bytes and ok = 0.
__global__ __launch_bounds__(P521_BLOCK) void k_p521_decode_points(const uint32_t* __restrict__ enc /* n*17 */, uint32_t* __restrict__ out_xy /* n*34 */,
                                                                   uint32_t* __restrict__ ok, uint32_t n) {
    uint32_t i = blockIdx.x * P521_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t w[W521];
    wave_load_words(enc + (size_t)i * W521, w);
    const uint32_t first = w[0] & 0xffu;
    uint32_t xb[W521];
    p521_sec1_x_words(w, xb);
    const F521 x = unpack(xb);                                               // 528 bits: 1 n
    const F521 x3 = mul(sqr(x), x);
    const F521 rhs = carry(add(sub(x3, add(x, dbl(x))), P521Sw3::b()));          // x^3 - 3 x + b: n - 3 n + n, carried
    F521 y;
    const bool root = f521_sqrt(rhs, y);
    const bool valid = (first == 0x02u || first == 0x03u) && below_p(xb) && root;
    y = cneg(y, is_odd(y) != ((first & 1u) != 0));
    if (live) {
        if (valid) {
            uint32_t yw[W521];
            pack(y, yw);
            wave_store_point_words(out_xy + (size_t)i * P521_PT_WORDS, xb, yw);
        } else {
            wave_store_zero_words<P521_PT_WORDS>(out_xy + (size_t)i * P521_PT_WORDS);
        }
        ok[i] = valid ? 1u : 0u;
    }
}

// Diagnostic (dr_p521_field_selftest): fp521.hip.h's operations on RAW limb images, one lane per (a, b) pair of 19 int32 limbs each, so
// that tests can drive every operation at the limb bounds its contract allows (a <= 2 n for the square, ka kb <= 6 for the product).
// out[i] = eleven canonical 68-byte records: a b, a^2, a + b, a - b, -a, carry(a), 4 a, a^-1 (0 for 0), carry(a)^((p + 1) / 4) (a root
// of a when a is a square), a itself (pack), -(2^28 - 1) a;  flags[i]: bit 0 a is a square, bit 1 the canonical a is odd, bit 2 a is
// zero, bit 3 a = b.
constexpr int P521_SELFTEST_RECORDS = 11;
__global__ __launch_bounds__(64) void k_p521_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                           uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    F521 a, b;
#pragma unroll
    for (int t = 0; t < L521; t++) { a.l[t] = a_limbs[(size_t)i * L521 + t]; b.l[t] = b_limbs[(size_t)i * L521 + t]; }   // (in place: DESIGN.md section 8x)
    uint32_t* o = out + (size_t)i * P521_SELFTEST_RECORDS * W521;
    auto put = [&](int r, const F521& v) { field_selftest_put(o, r, v); };
    put(0, mul(a, b));
    put(1, sqr(a));
    put(2, add(a, b));
    put(3, sub(a, b));
    put(4, neg(a));
    put(5, carry(a));
    put(6, mul_small(a, 4));
    put(7, inv(a));
    F521 root;
    const bool sq = f521_sqrt(carry(a), root);
    put(8, root);
    put(9, a);
    put(10, mul_small(a, -M521));
    flags[i] = (sq ? 1u : 0u) | (is_odd(a) ? 2u : 0u) | (is_zero(a) ? 4u : 0u) | (equal(a, b) ? 8u : 0u);
}

// Diagnostic (dr_p521_law_selftest): wave_curve.hip.h's wave_law_selftest over P521Curve, the law on raw limb images
__global__ __launch_bounds__(64) void k_p521_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<P521Curve>(pts, ctl, n, out);
}

}  // namespace dr
