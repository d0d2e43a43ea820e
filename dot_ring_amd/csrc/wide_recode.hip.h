// How a scalar of the wide suites (12, 14 or 17 words: P-384, Ed448 / Curve448, P-521) becomes bucket entries of wave_msm.hip.h: the
// tiling of its bits by windows and the signed digit of one window.  WindowTable (dev_types.hpp) keeps bit positions in uint8_t and
// for_each_digit (msm_recode.hip.h) reads 9 words, so neither reaches 522 bits; here a tiling is four integers and a window's start and
// width are closed forms of them.
//
// The digit of a window is Booth's: with raw = the window's bits, lo = the bit below the window and top = the window's highest bit,
//     d = raw + lo - top 2^width,   |d| <= 2^(width - 1).
// top of one window is lo of the next, so the terms -top 2^(start + width) and +lo 2^(next start) cancel and sum_w d_w 2^start_w = k
// whenever the highest tiled bit of k is 0.  A tiling therefore covers ONE BIT MORE than the scalars can have — 8 scalar_bytes + 1 (385,
// 449), 522 for P-521's k < 2^521 — and what a carry chain would carry out of the top digit is that bit's window.  No digit depends on
// another one: a workgroup that sorts one window reads the two words its window touches and nothing else, and no scalar is reduced.
// Plain integer C++: compiles for the device and, with g++, for the host (tests/native/wide_msm_plan_check.cpp runs these functions
// against big integers).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DR_WIDE_FN __host__ __device__ __forceinline__
#else
#define DR_WIDE_FN static inline
#endif

namespace dr {

// `bits` bits tiled by W windows: the lowest W - rem are `base` bits wide, the rem on top base + 1 (near-equal widths: a narrow top
// window would funnel every term into a few buckets)
struct WideTiling {
    int bits, W, base, rem;
};
DR_WIDE_FN WideTiling make_wide_tiling(int c, int bits) {
    WideTiling t;
    t.bits = bits, t.W = (bits + c - 1) / c;
    t.base = bits / t.W, t.rem = bits % t.W;
    return t;
}
DR_WIDE_FN int wide_cmax(const WideTiling& t) { return t.base + (t.rem ? 1 : 0); }
DR_WIDE_FN int wide_width(const WideTiling& t, int w) { return t.base + (w >= t.W - t.rem ? 1 : 0); }
DR_WIDE_FN int wide_start(const WideTiling& t, int w) { return w * t.base + (w > t.W - t.rem ? w - (t.W - t.rem) : 0); }

// the signed digit of the window [start, start + width) of the scalar of kw words at k (bits from 32 kw up are 0); width <= 24
DR_WIDE_FN int32_t wide_digit(const uint32_t* k, int kw, int start, int width) {
    const uint32_t mask = (1u << (width + 1)) - 1u;
    uint32_t v;                                            // bits start - 1 .. start + width - 1
    if (start == 0) {
        v = (k[0] << 1) & mask;
    } else {
        const int lo = start - 1, wi = lo >> 5;
        const uint64_t two = (uint64_t)(wi < kw ? k[wi] : 0u) | ((uint64_t)(wi + 1 < kw ? k[wi + 1] : 0u) << 32);
        v = (uint32_t)(two >> (lo & 31)) & mask;
    }
    return (int32_t)(v >> 1) + (int32_t)(v & 1u) - (int32_t)(((v >> width) & 1u) << width);
}

}  // namespace dr
