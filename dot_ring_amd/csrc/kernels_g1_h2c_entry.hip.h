// The kernels of the BLS12_381_G1 suites over kernels_g1_h2c.hip.h's device functions: the map, scalar multiplication, grouped MSM, SEC1
// decoding and the field diagnostic.  Included by capi_blsg1.hip alone (a kernel is defined in one translation unit);
// kernels_g1_h2c.hip.h itself is shared with the G2 unit.
#pragma once
#include "kernels_g1_h2c.hip.h"
#include "wave_msm.hip.h"

namespace dr {

// out[i] = the sum of the images of item i's `per_item` field elements (2: the uniform (RO) encoding, 1: the nonuniform one), times h_eff
// if clear.  us: n x per_item x 12 words (canonical, checked by the host), out: n x 24 words affine x || y (zeros: the identity), ok[i] =
// 0 where an isogeny denominator vanished.  One lane per item; one exponentiation per element and one inversion per item.  clear = 0 is
// the reference's map_to_curve_simple_swu (and the Q0 / Q1 / Q of the RFC's vectors).
__global__ __launch_bounds__(G1H_BLOCK) void k_blsg1_map_to_curve(const uint32_t* __restrict__ us, uint32_t* __restrict__ out_xy,
                                                                  uint32_t* __restrict__ ok, uint32_t n, uint32_t per_item, uint32_t clear) {
    uint32_t i = blockIdx.x * G1H_BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;            // keep the wave converged; the duplicate result is not stored
    G1hPoint acc = g1h_identity();
    bool good = true;
#pragma unroll 1
    for (uint32_t e = 0; e < per_item; e++) {
        uint32_t w[12];
        load_words12(us + ((size_t)i * per_item + e) * 12, w);
        Fq28 xn, xd, y;
        sswu_map<G1hSswu>(to_mont28(w), (w[0] & 1u) != 0, xn, xd, y);
        bool ok_e;
        const G1hPoint pt = g1h_iso_map(xn, xd, y, ok_e);
        good = good && ok_e;
        acc = g1h_add(acc, pt);
    }
    if (clear) acc = g1h_mul_public(acc, G1H_H_EFF, 63);
    if (live) {
        g1h_store_affine(out_xy + (size_t)i * 24, acc);
        ok[i] = good ? 1u : 0u;
    }
}

// out[i] = k[i] P[i] and out[g] = sum_{j<m} k[g m + j] P[g m + j]: wave_curve.hip.h's kernel bodies for this curve (points 24 words)
__global__ __launch_bounds__(G1H_BLOCK) void k_blsg1_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t n) {
    wave_scalar_mul<G1hCurve>(pts, ks, out, n);
}
__global__ __launch_bounds__(G1H_BLOCK) void k_blsg1_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    wave_msm_groups<G1hCurve>(pts, ks, out, groups, m, mpad);
}
// the bucket method from NARROW_PIP_FROM terms on (wave_msm.hip.h): the stages over G1hCurve, set sums out as affine x || y (dr_blsg1_msm)
DR_WAVE_MSM_KERNELS(blsg1, G1hCurve)
// Decoding (the reference's SWAffinePoint.string_to_point for a compressed string), one lane per 49-byte SEC1 encoding padded to 13
// words (bytes 49..51 zero): byte 0 is 0x02 or 0x03, x = bytes 1..48 BIG-endian, x < p, x^3 + 4 a square, y the root of byte 0's parity.
// G1H_DEC_CODEC accepts every point of E(Fq), as the reference's codec does; G1H_DEC_CHECK also demands r P = O (valid_point).
enum { G1H_DEC_CODEC = 0, G1H_DEC_CHECK = 1 };
template <int MODE>
__global__ __launch_bounds__(G1H_BLOCK) void k_blsg1_decode_points(const uint32_t* __restrict__ enc /* n*13 */, uint32_t* __restrict__ out_xy /* n*24 */,
                                                                   uint32_t* __restrict__ ok, uint32_t n) {
    sec1_decode<G1hCurve, MODE == G1H_DEC_CHECK>(enc, out_xy, ok, n);
}

// Diagnostic (dr_blsg1_field_selftest): what this file adds to fq28.hip.h, on raw limb images, one lane per (a, b) pair of 14 int32 limbs
// each, so that tests can drive it at the limb bounds the map and the law feed.  out[i] = five records of 12 words, each the canonical
// standard-form value of the result r (r R^-1 mod p, as the ABI's coordinates are made): a^((p - 3) / 4); the root a a^((p - 3) / 4) if
// its square is a, else 0; select(i odd, a, b); 12 a as the law computes it; a b + b a (mul2).  flags[i]: bit 0 a is a square, bit 1
// sgn0 (the parity of a's canonical standard-form value), bit 2 a is zero.
constexpr int G1H_SELFTEST_RECORDS = 5;
__global__ __launch_bounds__(64) void k_blsg1_field_selftest(const int32_t* __restrict__ a_limbs, const int32_t* __restrict__ b_limbs, uint32_t n,
                                                            uint32_t* __restrict__ out, uint32_t* __restrict__ flags) {
    const uint32_t i = blockIdx.x * 64 + threadIdx.x;
    if (i >= n) return;
    Fq28 a, b;
#pragma unroll
    for (int t = 0; t < L28; t++) { a.l[t] = a_limbs[(size_t)i * L28 + t]; b.l[t] = b_limbs[(size_t)i * L28 + t]; }
    uint32_t* o = out + (size_t)i * G1H_SELFTEST_RECORDS * 12;
    uint32_t w[12];
    const Fq28 pw = g1h_pow_p34(a);
    from_mont28(pw, w); store_words12(o, w);
    const Fq28 root = mul(pw, a);
    const bool sq = G1hSswu::equal(sqr(root), a);
    from_mont28(select(sq, root, Fq28::zero()), w); store_words12(o + 12, w);
    from_mont28(select((i & 1u) != 0, a, b), w); store_words12(o + 24, w);
    from_mont28(g1h_mul12(a), w); store_words12(o + 36, w);
    from_mont28(mul2(a, b, b, a), w); store_words12(o + 48, w);
    flags[i] = (sq ? 1u : 0u) | (g1h_is_odd(a) ? 2u : 0u) | (g1h_is_zero(a) ? 4u : 0u);
}

// Diagnostic (dr_blsg1_law_selftest): wave_curve.hip.h's wave_law_selftest over G1hCurve, the law on raw limb images
__global__ __launch_bounds__(64) void k_blsg1_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    wave_law_selftest<G1hCurve>(pts, ctl, n, out);
}

}  // namespace dr
