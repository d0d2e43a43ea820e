// How a scalar becomes bucket entries of the G1 / twisted Edwards Pippenger kernels: signed window digits (for_each_digit) and,
// over tables with a row per bit, the width-w non-adjacent form (for_each_wnaf_digit).  Plain C++ over uint32_t words: compiles for
// the device (hipcc, kernels_g1.hip.h) and for the host (g++, tests/native/recode_check.cpp runs these very functions against big integers).
#pragma once
#include <cstdint>

#include "dev_types.hpp"

#if defined(__HIPCC__)
#define DR_RECODE_FN __device__ __forceinline__
#else
#define DR_RECODE_FN static inline
#endif

namespace dr {

// visit the signed digits of scalar k: f(window, digit) for windows [w_lo, w_hi) (the carry chain always starts at 0).
// The scalar words are indexed only by the unrolled outer loop: a run-time index (k[start >> 5]) would put the array in
// scratch memory and cost one memory round trip per digit (measured: 5.4 -> 1.x ms for the prover's sort kernel).
template <bool WITH_ZEROS = false, class F>
DR_RECODE_FN void for_each_digit(const uint32_t (&k)[9], const WindowTable& wt, int w_lo, int w_hi, F&& f) {
    uint32_t carry = 0;
    int w = 0;
#pragma unroll
    for (int li = 0; li < 8; li++) {
        const uint64_t two = (uint64_t)k[li] | ((uint64_t)k[li + 1] << 32);
        while (w < w_hi && (wt.start[w] >> 5) == li) {
            const int c = wt.width[w], sh = wt.start[w] & 31;
            const uint32_t half = 1u << (c - 1);
            uint32_t raw = ((uint32_t)(two >> sh) & ((1u << c) - 1)) + carry;
            int32_t d;
            if (raw > half) { d = (int32_t)raw - (int32_t)(1u << c); carry = 1; }
            else { d = (int32_t)raw; carry = 0; }
            if (w >= w_lo && (WITH_ZEROS || d != 0)) f(w, d);
            w++;
        }
    }
}

// Width-w non-adjacent form (WindowTable::odd == 2, w = wt.cmax) of a scalar k < 2^255, for tables with a row per bit: odd digits
// |d| < 2^(w-1) — 256 / (w + 1) non-zero digits on average where w-bit windows have 256 / w —, every one of them an odd multiple,
// i.e. a bucket of the set as it is.  Scanning up from bit 0 with a carry c: the next digit starts at the first position whose bit
// differs from c, takes a bits from there (+ c) as v, d = v or v - 2^a (then c = 1), and the scan resumes a positions on.
// The width a is w until the top comes near.  Left at that, the LAST digit would be whatever bits remain — one to w of them with equal
// probability, so a quarter of all scalars would end in +-1 and bucket 0 of every set would hold 25 times the average list (measured:
// 1400 entries against 57; 1 ms per dense launch in the long-list kernels).  So within WNAF_ZONE * w bits of the top the remaining R bits
// are shared evenly by the ceil(R / w) digits still to come: a = ceil(R / ceil(R / w)) — the last two or three digits have 9 .. 13 bits
// each (+0.7 % digits, lowest buckets at 4x the average instead of 25x).
// Positions are counted on K = k << (W w - 256), whose length is exactly W slots of w positions: a digit at K-position P has R = W w - P
// bits above it and ceil(R / w) = W - floor(P / w) digits to go including itself, and since a >= R / (W - j) the next digit starts in
// a later slot: slot j = K-positions [w j, w j + w) starts at most one digit.  f(j, o, d): the digit d at table row wt.row[j] + o
// (wt.row[0] = 0, wt.row[j] = w j - shift).  The words of K are indexed by the unrolled outer loop only (for_each_digit).
// WITH_ZEROS: f(j, 0, 0) for slots that start none.
constexpr uint32_t WNAF_EMPTY16 = 0x7800u;                // u16 digit rows: sign << 15 | offset << 11 | bucket; offset 15 = no digit
constexpr uint32_t WNAF_ZONE = 3;
template <bool WITH_ZEROS = false, class F>
DR_RECODE_FN void for_each_wnaf_digit(const uint32_t (&k)[9], const WindowTable& wt, F&& f) {
    const uint32_t w = (uint32_t)wt.cmax, wmask = (1u << w) - 1u, L = (uint32_t)wt.W * w, shift = L - 256u;      // shift < w <= 13
    uint32_t K[10];
    K[0] = k[0] << shift;
#pragma unroll
    for (int i = 1; i < 9; i++) K[i] = shift ? (k[i] << shift) | (k[i - 1] >> (32u - shift)) : k[i];
    K[9] = 0;
    uint32_t c = 0, r = 0;                                // carry; first offset of the slot at which a digit may start
    int j = 0;
#pragma unroll
    for (int li = 0; li < 9; li++) {
        const uint64_t two = (uint64_t)K[li] | ((uint64_t)K[li + 1] << 32);
        while (j < wt.W && (wt.start[j] >> 5) == li) {
            const uint32_t chunk = (uint32_t)(two >> (wt.start[j] & 31));          // 32 valid bits; offset + width <= 2 w - 1 <= 25 are used
            const uint32_t m = (((c ? ~chunk : chunk) & wmask) >> r) << r;
            if (m) {
                const uint32_t o = (uint32_t)__builtin_ctz(m);
                const uint32_t R = L - ((uint32_t)wt.start[j] + o);                  // bits from this position to the top
                uint32_t a = w;
                if (R <= WNAF_ZONE * w) {
                    const uint32_t q = (R + w - 1u) / w;                             // digits still to come (1 .. WNAF_ZONE)
                    a = (R + q - 1u) / q;
                }
                const uint32_t v = ((chunk >> o) & ((1u << a) - 1u)) + c;           // odd
                int32_t d;
                if (v > (1u << (a - 1))) { d = (int32_t)v - (int32_t)(1u << a); c = 1; }
                else { d = (int32_t)v; c = 0; }
                f(j, j == 0 ? o - shift : o, d);
                r = o + a - w;                                                       // >= 0: the next digit starts in a later slot
            } else {
                if (WITH_ZEROS) f(j, 0u, 0);
                r = 0;
            }
            j++;
        }
    }
}

// The same form over a table that also holds the rows of a few small odd multiples of every base (block t: 2^s ((2 t + 1) P_i), t < M):
// a digit may be written d = +-m b with m = 2 t + 1 and b the odd bucket value, |b| < 2^(w-1), so the recoder is free to pick, among the
// M multipliers, the one whose digit clears the most bits of what is left of the scalar — 17.3 digits per scalar at w = 13 with
// {1, 3, 5, 7} where m = 1 alone has 18.8.  f(j, o, t, b): sum +-(2 t + 1) b 2^(row[j] + o) = k exactly.
// With n = (K >> P) + c the value left at the position P of the next digit (n odd): for every m, b_m is the centred odd residue of
// n / m mod 2^w, the remainder n - m b_m is a multiple of 2^w, and the m whose remainder has the most trailing zeros wins (counted over
// the WNAF_LOOK bits after the w cleared ones, which is what the slot's 64-bit chunk always holds; ties go to the smaller m).  The scan
// resumes w positions on with the carry c = (low w bits of n - m b_m) >> w, a small SIGNED value now (|c| <= M), so the first position
// of a digit is found by adding the carry to the slot's bits rather than by complementing them.  Within WNAF_ZONE * w bits of the top the
// rule is for_each_wnaf_digit's, m = 1 and the remaining bits shared evenly: its digit takes any carry in and leaves 0 or 1, so the sum
// closes at the top as it does there, the top digits stay on rows <= 255 and the lowest buckets are no fuller.  As there: at most one
// digit per slot (a digit clears at least w positions), and the words of K are indexed by the unrolled loop only.
// How a multiplier is tried: with N = n + 2^w (the WNAF_LOOK bits above), taken mod 2^(w + WNAF_LOOK), and q = N m^-1, b_m is the low w
// bits of q, sign-extended, and (N - m b_m) / 2^w = m (q - b_m) / 2^w mod 2^WNAF_LOOK; m is odd and (q - b_m) / 2^w = (q + 2^(w-1)) >> w
// (the half added carries into bit w exactly when b_m is negative), so the zeros won are the trailing zeros of q + 2^(w-1) from bit w
// up.  N and the inverse (21 bits suffice: w + WNAF_LOOK <= 21) are below 2^24, so the product and the half are ONE full-rate 24-bit
// multiply-add; masking the low w bits off with a stop bit at w + WNAF_LOOK, counting, and folding (zeros, 31 - t) into one key whose
// maximum is the winner (more zeros first, then the smaller t) are four more instructions - against a dozen for the residue, the
// centring, the product, the carry and the look-ahead sum of every candidate.  Only the winner's inverse (Newton, at run time), b and
// carry are then worked out.
// Bounds for M <= 32 (m <= 63): |n - m b| < 2^w + 32 + 63 2^(w-1), so |c| <= 32 = M and every value fits an int32_t by far; a carry
// is ADDED to bits already taken from the chunk, so it uses none of the chunk's bits: the highest one read is that of the look-ahead,
// offset + w + WNAF_LOOK <= (w - 1) + w + 8 = 33 for w = 13, and a 64-bit chunk shifted by at most 31 holds 33.  In the top zone a digit
// has a >= 7 bits (w >= 9) and takes a carry in of -32 .. 32 > -2^(a-1): it leaves 0 or 1 as before.
constexpr int WNAF_MAX_MULTIPLES = 32;
constexpr uint32_t WNAF_LOOK = 8;
constexpr uint32_t WNAF_EMPTY32 = 0x7fffffffu;            // u32 digit rows of tables with multiples: sign << 31 | t << 16 | offset << 11 | bucket
// (2 t + 1)^-1 mod 2^32 by Newton's iteration: x = m is right to 3 bits (m m = 1 mod 8), every step doubles them
constexpr uint32_t wnaf_multiplier_inverse(uint32_t t) {
    const uint32_t m = 2u * t + 1u;
    uint32_t x = m;
    for (int i = 0; i < 4; i++) x *= 2u - m * x;
    return x;
}
// a b + c for a, b < 2^24 (mod 2^32): v_mad_u32_u24 on the device, four times the rate of the 32-bit multiplication
#if defined(__HIPCC__)
#define DR_MAD24(a, b, c) (__umul24((a), (b)) + (c))
#else
#define DR_MAD24(a, b, c) ((a) * (b) + (c))
#endif
template <int M, bool WITH_ZEROS = false, class F>
DR_RECODE_FN void for_each_wnaf_multiple_digit(const uint32_t (&k)[9], const WindowTable& wt, F&& f) {
    static_assert(M >= 1 && M <= WNAF_MAX_MULTIPLES && WNAF_MAX_MULTIPLES <= 32, "multiplier count (the selection key has 5 bits for t)");
    const uint32_t w = (uint32_t)wt.cmax, wmask = (1u << w) - 1u, L = (uint32_t)wt.W * w, shift = L - 256u;      // shift < w <= 13
    uint32_t K[10];
    K[0] = k[0] << shift;
#pragma unroll
    for (int i = 1; i < 9; i++) K[i] = shift ? (k[i] << shift) | (k[i - 1] >> (32u - shift)) : k[i];
    K[9] = 0;
    int32_t c = 0;                                        // signed carry
    uint32_t r = 0;                                       // first offset of the slot at which a digit may start
    int j = 0;
#pragma unroll
    for (int li = 0; li < 9; li++) {
        const uint64_t two = (uint64_t)K[li] | ((uint64_t)K[li + 1] << 32);
        while (j < wt.W && (wt.start[j] >> 5) == li) {
            const uint64_t chunk = two >> (wt.start[j] & 31);                       // >= 33 valid bits; offset + width + look <= 2 w - 1 + 8 = 33 are used
            const uint32_t rest = (uint32_t)(chunk >> r);
            const uint32_t live = (rest + (uint32_t)c) & ((1u << (w - r)) - 1u);    // the slot's positions from r on, carry added
            if (live) {
                const uint32_t z = (uint32_t)__builtin_ctz(live), o = r + z;
                const int32_t co = ((int32_t)(rest & ((1u << z) - 1u)) + c) >> z;   // carry into position o (exact: the bits below are zero)
                const uint32_t R = L - ((uint32_t)wt.start[j] + o);                  // bits from this position to the top
                const uint32_t at = (uint32_t)(chunk >> o);
                if (R <= WNAF_ZONE * w) {
                    const uint32_t q = (R + w - 1u) / w;                             // digits still to come (1 .. WNAF_ZONE)
                    const uint32_t a = (R + q - 1u) / q;
                    const int32_t n = (int32_t)(at & ((1u << a) - 1u)) + co;
                    const uint32_t v = (uint32_t)n & ((1u << a) - 1u);               // odd
                    const int32_t d = v > (1u << (a - 1)) ? (int32_t)v - (int32_t)(1u << a) : (int32_t)v;
                    c = (n - d) >> a;
                    f(j, j == 0 ? o - shift : o, 0u, d);
                    r = o + a - w;
                } else {
                    const uint32_t lmask = (1u << (w + WNAF_LOOK)) - 1u, half = 1u << (w - 1), stop = 1u << (w + WNAF_LOOK);
                    const uint32_t N = ((at & lmask) + (uint32_t)co) & lmask;       // w + WNAF_LOOK <= 21 bits
                    // key of multiplier t: (w + zeros won) << 5 | 31 - t
                    uint32_t best = ((uint32_t)__builtin_ctz(((N + half) & ~wmask) | stop) << 5) | 31u;   // m = 1: q = N
#pragma unroll
                    for (int t = 1; t < M; t++) {
                        const uint32_t qh = DR_MAD24(N, wnaf_multiplier_inverse((uint32_t)t) & 0x1fffffu, half);
                        const uint32_t key = ((uint32_t)__builtin_ctz((qh & ~wmask) | stop) << 5) | (uint32_t)(31 - t);
                        best = key > best ? key : best;
                    }
                    const uint32_t bt = 31u - (best & 31u), bq = N * wnaf_multiplier_inverse(bt);
                    const int32_t n = (int32_t)(at & wmask) + co;
                    const int32_t bb = (int32_t)(bq << (32u - w)) >> (32u - w);     // odd, |bb| < 2^(w-1)
                    const int32_t bc = (n - (2 * (int32_t)bt + 1) * bb) >> w;
                    c = bc;
                    f(j, j == 0 ? o - shift : o, bt, bb);
                    r = o;
                }
            } else {
                c = ((int32_t)(rest & ((1u << (w - r)) - 1u)) + c) >> (w - r);
                if (WITH_ZEROS) f(j, 0u, 0u, 0);
                r = 0;
            }
            j++;
        }
    }
}

// run-time multiplier count (2, 4, 8, 16 or 32) -> the instance
template <bool WITH_ZEROS = false, class F>
DR_RECODE_FN void for_each_wnaf_multiple_digit(uint32_t multiples, const uint32_t (&k)[9], const WindowTable& wt, F&& f) {
    if (multiples == 2) for_each_wnaf_multiple_digit<2, WITH_ZEROS>(k, wt, f);
    else if (multiples == 4) for_each_wnaf_multiple_digit<4, WITH_ZEROS>(k, wt, f);
    else if (multiples == 16) for_each_wnaf_multiple_digit<16, WITH_ZEROS>(k, wt, f);
    else if (multiples == 32) for_each_wnaf_multiple_digit<32, WITH_ZEROS>(k, wt, f);
    else for_each_wnaf_multiple_digit<8, WITH_ZEROS>(k, wt, f);
}

}  // namespace dr
