// Sums of scalar multiples on BLS12-381's E(Fq2) (dr_blsg2_msm, dr_blsg2_msm_groups) and the diagnostic of its law on raw limb images
// (dr_blsg2_law_selftest), over kernels_g2_h2c.hip.h's complete law — none of that header's kernels or device functions changes.
//
// G2hCurve is a description of the curve AS FAR AS wave_msm.hip.h ASKS FOR ONE (Fe, Point, WORDS, SCALAR_WORDS, LDS_WORDS, EXTENDED, ZERO_IS_IDENTITY,
// unpack / pack / inv, to_lds / from_lds, identity / from_affine / add / dbl / cneg), so that DR_WAVE_MSM_KERNELS expands over it with
// wave_curve.hip.h and wave_msm.hip.h as they are.  Those templates read a coordinate as ONE array of limbs (wave_shfl_down) and multiply
// coordinates by an unqualified mul (wave_store_affine); an Fq2 is two arrays.  So the description's Fe is the 28 limbs of c0 then c1 and
// its Point three of them, and every member forwards to the Fq2 law by copying limbs, which costs no instruction once inlined.
//   the record    3 x 28 = 84 words, a whole number of uint4: x.c0, x.c1, y.c0, y.c1, z.c0, z.c1 — the order of g2h_store_limbs
//   the classes   a record is from_affine of the ABI's point (coordinates n, Z = 1), the identity (0 : 1 : 0) or what g2h_add returned:
//                 three mul_add, each the carried sum of two n — c2.1 while a row stays below 50 p^2, c2.9 at fq2_28.hip.h's limit of
//                 1024 p^2, which the law's rows (up to 561 p^2) stay under; c2.9 is what is relied on here.  The walk negates a record
//                 by g2h_neg (a carried negation of a c2.9: inside c3) and adds it to what g2h_add returned; the reduction adds and
//                 doubles what g2h_add and g2h_dbl returned (n, or c2.9 for Y).  All of it is inside c3, the class kernels_g2_h2c.hip.h
//                 documents for a coordinate the law takes.
// What the description does NOT have is a scalar: wave_scalar_mul_core's LDS window table would need 8 x 3 x 28 x 64 x 4 = 172 032 bytes
// (k_blsg2_scalar_mul), so msm_groups and the law diagnostic are kernels of their own below, on k_blsg2_scalar_mul's walk.
// Scalars on this curve are PUBLIC (there is no VRF over it): walk lengths, skipped additions and bucket lists depend on them.
#pragma once
#include "kernels_g2_h2c.hip.h"
#include "wave_msm.hip.h"

namespace dr {

struct G2hFe {
    int32_t l[2 * L28];               // c0's limbs, then c1's
};
struct G2hWavePoint {
    G2hFe x, y, z;
};
DR_DEV Fq2 g2w_fq2(const G2hFe& a) {
    Fq2 r;
#pragma unroll
    for (int t = 0; t < L28; t++) { r.c0.l[t] = a.l[t]; r.c1.l[t] = a.l[L28 + t]; }
    return r;
}
DR_DEV G2hFe g2w_fe(const Fq2& a) {
    G2hFe r;
#pragma unroll
    for (int t = 0; t < L28; t++) { r.l[t] = a.c0.l[t]; r.l[L28 + t] = a.c1.l[t]; }
    return r;
}
DR_DEV G2hPoint g2w_point(const G2hWavePoint& p) { return {g2w_fq2(p.x), g2w_fq2(p.y), g2w_fq2(p.z)}; }
DR_DEV G2hWavePoint g2w_wave(const G2hPoint& p) { return {g2w_fe(p.x), g2w_fe(p.y), g2w_fe(p.z)}; }
// what wave_store_affine multiplies coordinates by (found by argument-dependent lookup)
DR_DEV G2hFe mul(const G2hFe& a, const G2hFe& b) { return g2w_fe(mul(g2w_fq2(a), g2w_fq2(b))); }

struct G2hCurve {
    using Fe = G2hFe;
    using Point = G2hWavePoint;
    static constexpr int WORDS = 24, BLOCK = G2H_BLOCK, LDS_WORDS = 2 * L28;
    static constexpr int SCALAR_WORDS = 8;        // (for the stages' sort alone: there is no schedule over them, the head of the file)
    static constexpr bool EXTENDED = false, ZERO_IS_IDENTITY = true;
    DR_DEV static G2hFe unpack(const uint32_t (&w)[24]) {
        uint32_t w0[12], w1[12];
#pragma unroll
        for (int j = 0; j < 12; j++) { w0[j] = w[j]; w1[j] = w[12 + j]; }
        return g2w_fe({to_mont28(w0), to_mont28(w1)});
    }
    DR_DEV static void pack(const G2hFe& a, uint32_t (&w)[24]) {
        const Fq2 v = g2w_fq2(a);
        uint32_t w0[12], w1[12];
        from_mont28(v.c0, w0);
        from_mont28(v.c1, w1);
#pragma unroll
        for (int j = 0; j < 12; j++) { w[j] = w0[j]; w[12 + j] = w1[j]; }
    }
    DR_DEV static G2hFe inv(const G2hFe& a) { return g2w_fe(dr::inv(g2w_fq2(a))); }
    DR_DEV static void to_lds(const G2hFe& a, uint32_t (&w)[2 * L28]) { wave_limbs_to_words(a, w); }
    DR_DEV static G2hFe from_lds(const uint32_t (&w)[2 * L28]) { return wave_words_to_limbs<G2hFe>(w); }
    DR_DEV static G2hWavePoint identity() { return g2w_wave(g2h_identity()); }
    DR_DEV static G2hWavePoint from_affine(const G2hFe& x, const G2hFe& y) { return g2w_wave(g2h_from_affine(g2w_fq2(x), g2w_fq2(y))); }
    DR_DEV static G2hWavePoint add(const G2hWavePoint& p, const G2hWavePoint& q) { return g2w_wave(g2h_add(g2w_point(p), g2w_point(q))); }
    DR_DEV static G2hWavePoint dbl(const G2hWavePoint& p) { return g2w_wave(g2h_dbl(g2w_point(p))); }
    DR_DEV static G2hWavePoint cneg(const G2hWavePoint& p, bool negate) {
        const G2hPoint q = g2w_point(p);
        return g2w_wave(g2h_select(negate, g2h_neg(q), q));
    }
};

// the bucket method from BLSG2_PIP_FROM terms on (wave_msm.hip.h): the stages over G2hCurve, 32-byte scalars used as they are, set sums
// out as affine x || y (dr_blsg2_msm)
DR_WAVE_MSM_KERNELS(blsg2, G2hCurve)

// out[g] = sum_{j<m} k[g m + j] P[g m + j]: one lane per term (m padded to mpad, a power of two <= 64).  The walk is k_blsg2_scalar_mul's:
// from the top set bit of the wave's largest scalar, the addition under a wave-uniform ballot, P loaded again for every addition so that
// the walk holds one point.  A dead lane (padding, or a group past the last) stays converged on term 0 with every bit clear, so it ends
// as the identity.  Then the lanes of a group are folded with shuffles of the 84 limbs by the complete addition (terms that coincide or
// cancel need nothing special) and lane j = 0 stores the affine sum.  KW = the words of a scalar: 24 under dr_blsg2_msm_groups, 8 under
// dr_blsg2_msm below its threshold.
template <int KW>
__global__ __launch_bounds__(G2H_BLOCK) void k_blsg2_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks,
                                                                uint32_t* __restrict__ out, uint32_t groups, uint32_t m, uint32_t mpad) {
    const uint32_t lane = threadIdx.x;
    const uint32_t per_block = G2H_BLOCK / mpad;
    const uint32_t g = blockIdx.x * per_block + lane / mpad;
    const uint32_t j = lane % mpad;
    const bool live = g < groups && j < m;
    const size_t idx = live ? (size_t)g * m + j : 0;
    const uint32_t* k = ks + idx * KW;
    int top = -1;
#pragma unroll
    for (int q = 0; q < KW; q++) {
        const uint32_t w = live ? k[q] : 0u;
        if (w) top = 32 * q + 31 - __clz((int)w);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) top = max(top, __shfl_xor(top, off));
    top = __builtin_amdgcn_readfirstlane(top);
    G2hPoint acc = g2h_identity();
#pragma unroll 1
    for (int b = top; b >= 0; b--) {
        acc = g2h_dbl(acc);
        const bool bit = live && ((k[b >> 5] >> (b & 31)) & 1u) != 0;
        if (__builtin_amdgcn_ballot_w64(bit) != 0) {
            asm volatile("" ::: "memory");
            bool identity;
            const G2hPoint P = g2h_load_affine(pts + idx * 48, identity);
            acc = g2h_add(acc, g2h_select(bit, P, g2h_identity()));
        }
    }
    G2hWavePoint sum = g2w_wave(acc);
#pragma unroll 1
    for (uint32_t s = mpad >> 1; s > 0; s >>= 1) sum = G2hCurve::add(sum, wave_shfl_down<G2hCurve>(sum, s));
    if (g < groups && j == 0) g2h_store_affine(out + (size_t)g * 48, g2w_point(sum));
}

// Diagnostic (dr_blsg2_law_selftest): the law on RAW limb images, one lane per record, with wave_law_selftest's ABI shape and slot
// numbers.  pts: n records of P then Q, each x, y, z of 28 int32 limbs (c0 then c1); ctl: n control words; out: n x WAVE_LAW_SLOTS points
// in the same form; recs: one record of the bucket method per LANE of the launch (84 words each).  The slots:
//   0  add(P, Q)       1  add(P, -Q)       2  dbl(P)       3  not written       4  cneg(P, true)       6  cneg(P, false)
//   5  slot 0's point after wave_msm_put into the lane's record and wave_msm_get back: the path the bucket walk reads, where the other
//      curves' diagnostic goes through the LDS table
//   7 + w, w = 0..5    a chain run as the bit walk runs a step: acc = dbl(acc), then acc = add(acc, T), T that record loaded again,
//                      negated when bit w of the control word is set and the identity when bit 8 + w is; the chain starts at acc = P
// A lane past n recomputes record n - 1 and stores nothing (its record in recs is its own).
__global__ __launch_bounds__(64) void k_blsg2_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n,
                                                          int32_t* __restrict__ out, uint32_t* __restrict__ recs) {
    using C = G2hCurve;
    constexpr int L = 2 * L28, PT = 3 * L;
    const size_t slot = (size_t)blockIdx.x * 64 + threadIdx.x;
    uint32_t i = (uint32_t)slot;
    const bool live = i < n;
    if (!live) i = n - 1;
    auto load = [&](const int32_t* p) {
        G2hWavePoint r;
#pragma unroll
        for (int t = 0; t < L; t++) { r.x.l[t] = p[t]; r.y.l[t] = p[L + t]; r.z.l[t] = p[2 * L + t]; }
        return r;
    };
    int32_t* const o = out + (size_t)i * (WAVE_LAW_SLOTS * PT);
    auto put = [&](int s, const G2hWavePoint& r) {
        if (!live) return;
        int32_t* q = o + s * PT;
#pragma unroll
        for (int t = 0; t < L; t++) { q[t] = r.x.l[t]; q[L + t] = r.y.l[t]; q[2 * L + t] = r.z.l[t]; }
    };
    const int32_t* const rec = pts + (size_t)i * (2 * PT);
    const uint32_t cw = ctl[i];
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const G2hWavePoint R = C::add(load(rec), C::cneg(load(rec + PT), s != 0));
        put(s, R);
        if (s == 0) wave_msm_put<C>(recs, slot, R);
    }
    put(2, C::dbl(load(rec)));
#pragma unroll 1
    for (int s = 0; s < 2; s++) put(s == 0 ? 4 : 6, C::cneg(load(rec), s == 0));
    asm volatile("" ::: "memory");
    put(5, wave_msm_get<C>(recs, slot));
    G2hWavePoint acc = load(rec);
#pragma unroll 1
    for (int w = 0; w < WAVE_LAW_WINDOWS; w++) {
        acc = C::dbl(acc);
        asm volatile("" ::: "memory");
        G2hWavePoint T = C::cneg(wave_msm_get<C>(recs, slot), ((cw >> w) & 1u) != 0);
        if (((cw >> (8 + w)) & 1u) != 0) T = C::identity();
        acc = C::add(acc, T);
        put(7 + w, acc);
    }
}

}  // namespace dr
