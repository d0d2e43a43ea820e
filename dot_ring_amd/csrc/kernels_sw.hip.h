// Bandersnatch in short Weierstrass form (DR_CURVE_BANDERSNATCH_SW; the reference's specs/bandersnatch_sw.py): the same group as the
// twisted Edwards curve of the other kernels, reached through its Montgomery model (ring_proof/ring_curve.py:10-23).  Only the suite's
// boundary is new: the 33-byte point codec, the device half of its try-and-increment hash-to-curve and the two maps.  Every group
// operation stays on the twisted Edwards kernels.
//   SW -> TE:  s = MB x - A3, t = MB y;  v = s / t, w = (s - 1) / (s + 1)
//   TE -> SW:  s = (1 + w) / (1 - w), t = s / v;  x = (s + A3) / MB, y = t / MB
// The rational torsion is Z/2 x Z/2, so the only points on which a map divides by zero are the identity (mapped explicitly: SW (0, 0)
// <-> TE (0, 1)) and the three points with y = 0, which decoding rejects.
#pragma once
#include "kernels_bsn.hip.h"

namespace dr {

// standard-form little-endian words (bandersnatch_sw.py:17-30, ring_curve.py:10-11)
struct SwConsts {
    static constexpr uint32_t A[8] = {0x33267935u, 0xe0720f80u, 0x4f20541du, 0xe32913d2u, 0x26da26e5u, 0x8c4a118eu, 0xe9f0fc8bu, 0x17d15ecbu};
    static constexpr uint32_t B[8] = {0xd5e8bbbfu, 0x07bb3d28u, 0xab8c2569u, 0xfa2d24f0u, 0x4d5d4625u, 0x11194e6bu, 0xd12e60a8u, 0x415fcb20u};
    static constexpr uint32_t MONT_B[8] = {0x6fa86d15u, 0x926c66ebu, 0x6bd74122u, 0xbd025b63u, 0xc340cf6au, 0x316b96e5u, 0x3c878eeau, 0x384d1c15u};
    static constexpr uint32_t A3[8] = {0x9b3c9f88u, 0x614b5476u, 0x4c4244c5u, 0x18b9b65du, 0x198b28feu, 0xe0dbdc89u, 0x6f6639c1u, 0x1617cddau};
    static constexpr uint32_t INV_MONT_B[8] = {0xb9dca9c6u, 0x53258341u, 0xa205081au, 0x20e40a26u, 0xeea8ea4fu, 0x419e4909u, 0x9cace355u, 0x5b0b3709u};
    static constexpr uint32_t A3_OVER_MONT_B[8] = {0x84178ed1u, 0xc891a87du, 0xe94fca97u, 0xaf0f7e94u, 0xc311d927u, 0x188e44aeu, 0xcf0964d2u, 0x5de00fbdu};
};
template <const uint32_t (&W)[8]>
DR_DEV Fs sw_const() {
    Fr w;
#pragma unroll
    for (int i = 0; i < 8; i++) w.l[i] = W[i];
    return fs_from_std(w);
}

// y is the larger of (y, p - y)
DR_DEV bool fs_is_larger(const Fs& y) {
    const Fr ys = fs_to_std(y), nys = fs_to_std(neg(y));
    bool larger = false;
#pragma unroll
    for (int j = 7; j >= 0; j--) {
        if (ys.l[j] != nys.l[j]) { larger = ys.l[j] > nys.l[j]; break; }
    }
    return larger;
}

// up to SW_MAP_MAX points per lane share ONE inversion (Montgomery's trick): a proof's few points cost one inversion, not one each
constexpr int SW_MAP_MAX = 4;

// out[i] = map(in[i]) for n points (16 standard-form words each), `per` consecutive points per lane.  TO_TE: SW -> TE, else TE -> SW.
template <bool TO_TE>
__global__ __launch_bounds__(64) void k_sw_map(const uint32_t* __restrict__ in, uint32_t* __restrict__ out, uint32_t n, uint32_t per) {
    const uint32_t lane = blockIdx.x * 64 + threadIdx.x;
    const uint32_t first = lane * per;
    if (first >= n) return;
    const uint32_t cnt = min(per, n - first);
    const Fs one = Fs::one();
    const Fs mb = sw_const<SwConsts::MONT_B>(), a3 = sw_const<SwConsts::A3>();
    const Fs imb = sw_const<SwConsts::INV_MONT_B>(), a3mb = sw_const<SwConsts::A3_OVER_MONT_B>();
    Fs num[SW_MAP_MAX], aux[SW_MAP_MAX], sp1[SW_MAP_MAX], den[SW_MAP_MAX], pref[SW_MAP_MAX];
    bool idn[SW_MAP_MAX];
    Fs run = one;
#pragma unroll
    for (uint32_t k = 0; k < SW_MAP_MAX; k++) {
        idn[k] = true;
        num[k] = aux[k] = sp1[k] = den[k] = one;
        if (k < cnt) {
            const Fs x = fs_from_std(load_fr_std(in + (size_t)(first + k) * 16));
            const Fs y = fs_from_std(load_fr_std(in + (size_t)(first + k) * 16 + 8));
            if (TO_TE) {                      // v = s (s + 1) / (t (s + 1)),  w = (s - 1) t / (t (s + 1))
                idn[k] = is_zero(x) && is_zero(y);
                num[k] = carry(sub(mul(mb, x), a3));
                aux[k] = mul(mb, y);
                sp1[k] = carry(add(num[k], one));
                const Fs d = mul(aux[k], sp1[k]);
                if (!idn[k] && !is_zero(d)) den[k] = d;
            } else {                          // t = (1 + w) / ((1 - w) v),  s = t v
                idn[k] = is_zero(x) && equal(y, one);
                num[k] = carry(add(one, y));
                aux[k] = x;
                const Fs d = mul(carry(sub(one, y)), x);
                if (!idn[k] && !is_zero(d)) den[k] = d;
            }
        }
        pref[k] = run;
        run = mul(run, den[k]);
    }
    Fs inv_acc = inv(run);                    // 1 / (den[0] ... den[per-1]); a zero denominator (no point of the curve) counts as 1
#pragma unroll
    for (int k = SW_MAP_MAX - 1; k >= 0; k--) {
        const Fs d_inv = mul(inv_acc, pref[k]);
        inv_acc = mul(inv_acc, den[k]);
        if ((uint32_t)k >= cnt) continue;
        Fs ox, oy;
        if (TO_TE) {
            ox = mul(mul(num[k], sp1[k]), d_inv);
            oy = mul(mul(carry(sub(num[k], one)), aux[k]), d_inv);
            if (idn[k]) { ox = Fs::zero(); oy = one; }
        } else {
            const Fs t = mul(num[k], d_inv);
            ox = carry(add(mul(mul(t, aux[k]), imb), a3mb));
            oy = mul(t, imb);
            if (idn[k]) { ox = Fs::zero(); oy = Fs::zero(); }
        }
        store_fr_std(out + (size_t)(first + k) * 16, fs_to_std(ox));
        store_fr_std(out + (size_t)(first + k) * 16 + 8, fs_to_std(oy));
    }
}

// dec_point of the SW suite for a batch (bandersnatch_sw.py: string_to_point, _y_recover; vrf/codec.py dec_point), one lane per point.
// enc: 9 words per point — x (8 words, little-endian) and the flag byte in word 8.  Rejected: the infinity flag 0x40, any of the low six
// flag bits, x >= p, x^3 + a x + b not a square, y = 0, a point outside the prime-order subgroup (the cofactor check of
// te_cofactor_check on the TE image).  OUT_SW: out_xy = the SW point (dr_te_decode_points), else its TE image (internal callers).
// TAI: the device half of try-and-increment (point.py:252-296 for an SW curve): enc is the 32 squeezed bytes (8 words per candidate),
// bit 255 cleared, the larger root taken; out = 4 P on TE and ok = "decoded and 4 P is not the identity".
template <bool OUT_SW, bool TAI>
__global__ __launch_bounds__(BSN_BLOCK) void k_sw_decode_points(const uint32_t* __restrict__ enc, uint32_t* __restrict__ out_xy /* n*16 std */,
                                                                uint32_t* __restrict__ ok, uint32_t n) {
    __shared__ uint32_t tab[BSN_TABLE * BSN_PT_WORDS * BSN_BLOCK];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * BSN_BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;
    constexpr int STRIDE = TAI ? 8 : 9;
    Fr xs;
#pragma unroll
    for (int j = 0; j < 8; j++) xs.l[j] = enc[(size_t)i * STRIDE + j];
    uint32_t flag = 0x80u;
    if (TAI) xs.l[7] &= 0x7fffffffu;
    else flag = enc[(size_t)i * STRIDE + 8];
    bool valid = (flag & 0x7fu) == 0;                     // neither the infinity flag nor a low bit
    {   // x < p
        uint32_t borrow = 0;
#pragma unroll
        for (int j = 0; j < 8; j++) (void)subb(xs.l[j], FrParams::P[j], borrow);
        if (!borrow) { valid = false; xs = Fr::zero(); }
    }
    const Fs one = Fs::one();
    const Fs x = fs_from_std(xs);
    const Fs rhs = carry(add(mul(carry(add(sqr(x), sw_const<SwConsts::A>())), x), sw_const<SwConsts::B>()));
    Fs y;
    if (!fr_sqrt(rhs, y)) { valid = false; y = one; }
    if (is_zero(y)) { valid = false; y = one; }
    if (fs_is_larger(y) != ((flag & 0x80u) != 0)) y = neg(y);
    // to TE (the identity cannot occur here: (0, 0) is not on the curve)
    const Fs s = carry(sub(mul(sw_const<SwConsts::MONT_B>(), x), sw_const<SwConsts::A3>())), t = mul(sw_const<SwConsts::MONT_B>(), y);
    const Fs sp1 = carry(add(s, one));
    Fs d = mul(t, sp1);
    if (is_zero(d)) { valid = false; d = one; }
    const Fs di = inv(d);
    const Fs v = mul(mul(s, sp1), di), w = mul(mul(carry(sub(s, one)), t), di);
    Fs ox, oy;
    te_cofactor_check<CV_BANDERSNATCH, TAI>(tab, lane, v, w, valid, ox, oy);
    if (OUT_SW && !TAI) { ox = x; oy = y; }
    if (live) {
        store_fr_std(out_xy + (size_t)i * 16, fs_to_std(ox));
        store_fr_std(out_xy + (size_t)i * 16 + 8, fs_to_std(oy));
        ok[i] = valid ? 1u : 0u;
    }
}

}  // namespace dr
