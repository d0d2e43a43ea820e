// Host check of for_each_wnaf_multiple_digit (dot_ring_amd/csrc/msm_recode.hip.h) with M = 16 and 32 multipliers — the instances the
// sort kernels of the batched G1 Pippenger run over an SRS table with 16 or 32 blocks of odd-multiple rows — against big integers, for
// w = 9 .. 13: sum +-(2 t + 1) b 2^row = k exactly, at most one digit per slot and the slots visited in order, rows <= 255, offsets within
// their 4-bit field, b odd and |b| < 2^(w-1), t < M, the run-time dispatcher and WITH_ZEROS = false give the same digits.
// The multiplier inverses: wnaf_multiplier_inverse(t) (2 t + 1) = 1 mod 2^32 for every t < WNAF_MAX_MULTIPLES = 32.
// Scalars: those of recode_check.cpp and recode_multiples_check.cpp (0, small values, r - 1 and its neighbours, runs of ones across every
// slot boundary, alternating patterns, 2^w - 1 and 2^(w-1) +- 1 at every position, sparse and dense random values), single bits
// +- 1 .. 64 (carries of either sign, up to the largest multiplier, into an empty top), and 20 000 uniformly random ones, over which the
// mean digit count of every width must lie within 0.1 of the planner's figure (msm_plan.hpp: NAF_MULTIPLE_DIGITS, columns 16 and 32), below
// the count with 8 multipliers, and 32 below 16; and over a vector of 6145 uniformly random scalars the fullest bucket of the set holds at
// most six times the mean list.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

#include "msm_plan.hpp"
#include "msm_recode.hip.h"

typedef unsigned __int128 u128;

struct Big {                    // 320-bit two's complement accumulator, enough for sums of +-digit * 2^pos with pos < 260
    uint32_t w[10];
    Big() { std::memset(w, 0, sizeof w); }
    void add_shifted(int64_t d, unsigned pos) {
        uint32_t t[10];
        std::memset(t, 0, sizeof t);
        const bool neg = d < 0;
        uint64_t mag = neg ? (uint64_t)(-d) : (uint64_t)d;
        unsigned word = pos / 32, sh = pos % 32;
        u128 v = (u128)mag << sh;
        for (int i = 0; i < 4 && word + i < 10; i++) t[word + i] = (uint32_t)(v >> (32 * i));
        if (!neg) {
            uint64_t carry = 0;
            for (int i = 0; i < 10; i++) { uint64_t s = (uint64_t)w[i] + t[i] + carry; w[i] = (uint32_t)s; carry = s >> 32; }
        } else {
            uint64_t borrow = 0;
            for (int i = 0; i < 10; i++) { uint64_t s = (uint64_t)w[i] - t[i] - borrow; w[i] = (uint32_t)s; borrow = (s >> 32) & 1; }
        }
    }
    bool equals(const uint32_t (&k)[9]) const {
        for (int i = 0; i < 8; i++) if (w[i] != k[i]) return false;
        return w[8] == 0 && w[9] == 0;
    }
};

static const uint32_t R[8] = {0x00000001u, 0xffffffffu, 0xfffe5bfeu, 0x53bda402u, 0x09a1d805u, 0x3339d808u, 0x299d7d48u, 0x73eda753u};

static bool below_r(const uint32_t (&k)[9]) {
    for (int i = 7; i >= 0; i--) if (k[i] != R[i]) return k[i] < R[i];
    return false;
}

static int failures = 0;
static void fail(const char* what, int w, int M, const uint32_t (&k)[9]) {
    if (failures++ < 10) {
        std::fprintf(stderr, "FAIL %s (w = %d, M = %d) k =", what, w, M);
        for (int i = 7; i >= 0; i--) std::fprintf(stderr, " %08x", k[i]);
        std::fprintf(stderr, "\n");
    }
}

static dr::WindowTable naf_table(int w) {         // msm_plan.hpp: msm_shape, the non-adjacent form
    dr::WindowTable wt{};
    wt.W = (256 + w - 1) / w;
    wt.cmax = w;
    const int shift = wt.W * w - 256;
    for (int j = 0; j < wt.W; j++) { wt.start[j] = (uint8_t)(w * j); wt.row[j] = (uint8_t)(j ? w * j - shift : 0); wt.width[j] = (uint8_t)w; }
    wt.odd = 2;
    return wt;
}

enum Mode { edges, uniform, vector6145 };
static Mode mode = edges;
static const int MS[3] = {8, 16, 32};             // (8: counted only, as the figure the wider ones must beat)
static unsigned long long total_digits[16][3], total_scalars[16][3];
static std::vector<unsigned long long> bin_load[16][3];

struct Digit { int j; uint32_t o, t; int32_t b; };

template <int M>
static void check_one(const uint32_t (&k)[9], int w, int mi) {
    const dr::WindowTable wt = naf_table(w);
    Big sum;
    int last_slot = -1, count = 0, slots_seen = 0;
    bool ok = true;
    std::vector<Digit> seen;
    dr::for_each_wnaf_multiple_digit<M, true>(k, wt, [&](int j, uint32_t o, uint32_t t, int32_t b) {
        slots_seen++;
        if (j != last_slot + 1) ok = false;                        // WITH_ZEROS visits every slot once, in order: one digit per slot
        last_slot = j;
        if (b == 0) return;
        const int pos = (int)wt.row[j] + (int)o;                   // table row within block t
        if (!(b & 1) || b >= (1 << (w - 1)) || b <= -(1 << (w - 1))) ok = false;
        if (o > 14u || pos > 255 || pos < 0 || t >= (uint32_t)M) ok = false;
        const uint32_t mag = (uint32_t)(b < 0 ? -b : b);
        if ((mag - 1u) >> 1 >= (1u << (w - 2))) ok = false;
        count++;
        sum.add_shifted((int64_t)(2 * (int)t + 1) * b, (unsigned)pos);
        seen.push_back(Digit{j, o, t, b});
        if (mode != edges) bin_load[w][mi][(mag - 1u) >> 1]++;
    });
    if (!ok || slots_seen != wt.W || !sum.equals(k)) fail("multiples form", w, M, k);
    // the same digits without the empty slots, through the run-time dispatcher
    size_t at = 0;
    bool same = true;
    dr::for_each_wnaf_multiple_digit((uint32_t)M, k, wt, [&](int j, uint32_t o, uint32_t t, int32_t b) {
        if (at >= seen.size() || seen[at].j != j || seen[at].o != o || seen[at].t != t || seen[at].b != b) same = false;
        at++;
    });
    if (!same || at != seen.size()) fail("multiples form, WITH_ZEROS = false", w, M, k);
    if (mode == uniform) { total_digits[w][mi] += (unsigned long long)count; total_scalars[w][mi]++; }
}

static void check(const uint32_t (&k)[9]) {
    if (!below_r(k)) return;
    for (int w = 9; w <= 13; w++) {
        if (mode == uniform) check_one<8>(k, w, 0);
        check_one<16>(k, w, 1);
        check_one<32>(k, w, 2);
    }
}

static void set_bits(uint32_t (&k)[9], int lo, int hi) {       // bits [lo, hi) set
    for (int b = lo; b < hi; b++) k[b / 32] |= 1u << (b % 32);
}

int main() {
    std::mt19937_64 rng(20261020);
    uint32_t k[9];
    auto clear = [&] { std::memset(k, 0, sizeof k); };
    // the inverses the recoder multiplies by
    static_assert(dr::WNAF_MAX_MULTIPLES == 32, "multiplier count");
    {
        uint32_t minv[dr::WNAF_MAX_MULTIPLES];
        for (uint32_t t = 0; t < (uint32_t)dr::WNAF_MAX_MULTIPLES; t++) minv[t] = dr::wnaf_multiplier_inverse(t);
        for (uint32_t t = 0; t < (uint32_t)dr::WNAF_MAX_MULTIPLES; t++)
            if ((uint32_t)((2 * t + 1) * minv[t]) != 1u) {
                std::fprintf(stderr, "FAIL: inverse of %u\n", 2 * t + 1);
                failures++;
            }
    }
    // zero, one, small values, r - 1, (r - 1) / 2 and neighbours
    clear(); check(k);
    for (uint32_t v = 1; v <= 300; v++) { clear(); k[0] = v; check(k); }
    for (int delta = 1; delta <= 40; delta++) {
        clear();
        uint64_t borrow = (uint64_t)delta;
        for (int i = 0; i < 8; i++) { uint64_t s = (uint64_t)R[i] - borrow; k[i] = (uint32_t)s; borrow = (s >> 32) & 1; }
        check(k);
        uint32_t h[9];
        std::memcpy(h, k, sizeof h);
        for (int i = 0; i < 8; i++) k[i] = (h[i] >> 1) | (i < 7 ? h[i + 1] << 31 : 0);
        check(k);
    }
    // single bits, single bits minus and plus 1 .. 64 (negative and positive carries as large as the largest multiplier into an empty
    // top), runs of ones from every start to every end (the carry crosses every slot boundary)
    for (int b = 0; b < 255; b++) {
        clear(); k[b / 32] = 1u << (b % 32); check(k);
        for (uint32_t delta = 1; delta <= 64; delta++) {
            if (b >= 7) {
                clear(); k[b / 32] = 1u << (b % 32);
                uint64_t borrow = delta;
                for (int i = 0; i < 8; i++) { uint64_t s = (uint64_t)k[i] - borrow; k[i] = (uint32_t)s; borrow = (s >> 32) & 1; }
                check(k);
            }
            if (b < 254) {
                clear(); k[b / 32] = 1u << (b % 32);
                uint64_t carry = delta;
                for (int i = 0; i < 8; i++) { uint64_t s = (uint64_t)k[i] + carry; k[i] = (uint32_t)s; carry = s >> 32; }
                check(k);
            }
        }
    }
    for (int lo = 0; lo < 255; lo += 1)
        for (int hi = lo + 1; hi <= 255; hi += (hi - lo < 30 ? 1 : 7)) { clear(); set_bits(k, lo, hi); check(k); }
    // alternating patterns at every shift
    for (int sh = 0; sh < 32; sh++)
        for (uint32_t pat : {0x55555555u, 0xaaaaaaaau, 0x33333333u, 0x0f0f0f0fu, 0xfffe0001u, 0x80000001u, 0x7fffffffu}) {
            clear();
            for (int i = 0; i < 8; i++) k[i] = pat;
            k[7] &= 0x3fffffffu;
            uint32_t t[9];
            std::memcpy(t, k, sizeof t);
            for (int i = 0; i < 8; i++) k[i] = (t[i] >> sh) | (sh && i < 7 ? t[i + 1] << (32 - sh) : 0);
            check(k);
        }
    // 2^w - 1, 2^(w-1) and 2^(w-1) +- 1 at every position: top digits on the last rows
    for (int w = 9; w <= 14; w++)
        for (int pos = 0; pos + w < 254; pos++)
            for (int v = 0; v < 4; v++) {
                clear();
                uint64_t val = v == 0 ? (1ull << w) - 1 : v == 1 ? (1ull << (w - 1)) : v == 2 ? (1ull << (w - 1)) + 1 : (1ull << (w - 1)) - 1;
                u128 sv = (u128)val << (pos % 32);
                for (int i = 0; i < 3 && pos / 32 + i < 8; i++) k[pos / 32 + i] = (uint32_t)(sv >> (32 * i));
                check(k);
            }
    // random values: sparse, dense, and random with the top cleared
    for (int it = 0; it < 30000; it++) {
        clear();
        const int m = it % 3;
        for (int i = 0; i < 8; i++) {
            uint32_t v = (uint32_t)rng();
            if (m == 0) v &= (uint32_t)rng();
            if (m == 1) v |= (uint32_t)rng();
            if (m == 2) v &= (uint32_t)rng() & (uint32_t)rng();
            k[i] = v;
        }
        k[7] &= 0x7fffffffu;
        check(k);
    }
    // 20 000 uniformly random scalars below r: digit counts
    for (int w = 9; w <= 13; w++) for (int mi = 0; mi < 3; mi++) bin_load[w][mi].assign((size_t)1 << (w - 2), 0);
    mode = uniform;
    for (int done = 0; done < 20000;) {
        clear();
        for (int i = 0; i < 8; i++) k[i] = (uint32_t)rng();
        k[7] &= 0x7fffffffu;
        if (!below_r(k)) continue;
        check(k);
        done++;
    }
    for (int w = 9; w <= 13; w++) {
        double mean[3];
        std::printf("w = %2d: digits per scalar", w);
        for (int mi = 0; mi < 3; mi++) {
            mean[mi] = (double)total_digits[w][mi] / (double)total_scalars[w][mi];
            std::printf("  M = %d %.3f", MS[mi], mean[mi]);
        }
        std::printf("\n");
        for (int mi = 0; mi < 3; mi++) {
            const double want = NAF_MULTIPLE_DIGITS[w - 9][mi + 2];                  // columns 2, 4, 8, 16, 32
            if (mean[mi] < want - 0.1 || mean[mi] > want + 0.1) {
                std::fprintf(stderr, "FAIL: %.3f digits per scalar at w = %d, M = %d, the plan has %.2f +- 0.1\n", mean[mi], w, MS[mi], want);
                failures++;
            }
            if (mi > 0 && mean[mi] >= mean[mi - 1]) { std::fprintf(stderr, "FAIL: no fewer digits at w = %d with M = %d than with %d\n", w, MS[mi], MS[mi - 1]); failures++; }
        }
    }
    // a vector of 6145 uniformly random scalars: the fullest bucket against the mean list
    for (int w = 9; w <= 13; w++) for (int mi = 0; mi < 3; mi++) bin_load[w][mi].assign((size_t)1 << (w - 2), 0);
    mode = vector6145;
    for (int done = 0; done < 6145;) {
        clear();
        for (int i = 0; i < 8; i++) k[i] = (uint32_t)rng();
        k[7] &= 0x7fffffffu;
        if (!below_r(k)) continue;
        check(k);
        done++;
    }
    for (int w = 9; w <= 13; w++)
        for (int mi = 1; mi < 3; mi++) {
            unsigned long long most = 0, all = 0;
            for (unsigned long long v : bin_load[w][mi]) { most = v > most ? v : most; all += v; }
            const double mean = (double)all / (double)bin_load[w][mi].size();
            std::printf("w = %2d, M = %d: fullest bucket %llu = %.2f x the mean list %.1f\n", w, MS[mi], most, (double)most / mean, mean);
            if ((double)most > 6.0 * mean) { std::fprintf(stderr, "FAIL: skewed buckets at w = %d, M = %d\n", w, MS[mi]); failures++; }
        }
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("recoding with 16 and 32 multiples ok\n");
    return 0;
}
