// The scalar recoding of wave_curve.hip.h's fixed schedule: signed 4-bit digits of a scalar of KW words, k = sum d_w 16^w + c 16^(8 KW)
// with d_w in [-8, 7] and c, the carry out of the top nibble, 0 or 1.  dig[w / 8] holds d_w + 8 in its nibble w % 8.
// Plain integer C++: compiles for the device and, with g++, for the host (tests/native/wave_recode_check.cpp, p521_host_check.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DR_RECODE_FN __host__ __device__ __forceinline__
#else
#define DR_RECODE_FN static inline
#endif

namespace dr {

// the eight digits of one word: carry is the carry into its lowest nibble on entry and out of its top nibble on return
DR_RECODE_FN uint32_t wave_recode_word(uint32_t kw, uint32_t& carry) {
    uint32_t packed = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t v = ((kw >> (4 * j)) & 15u) + carry;
        carry = v >= 8u ? 1u : 0u;
        packed |= ((v + 8u) & 15u) << (4 * j);
    }
    return packed;
}
// all of them; returns c
template <int KW>
DR_RECODE_FN uint32_t wave_recode(const uint32_t (&k)[KW], uint32_t (&dig)[KW]) {
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < KW; w++) dig[w] = wave_recode_word(k[w], carry);
    return carry;
}
// digit w as it is stored, d_w + 8 in [0, 15], and as itself
template <int KW>
DR_RECODE_FN uint32_t wave_nibble(const uint32_t (&dig)[KW], int w) { return (dig[w >> 3] >> (4 * (w & 7))) & 15u; }
template <int KW>
DR_RECODE_FN int wave_digit(const uint32_t (&dig)[KW], int w) { return (int)wave_nibble(dig, w) - 8; }

}  // namespace dr
