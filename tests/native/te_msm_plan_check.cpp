// Host check of the twisted Edwards Pippenger's plan (dr::plan_te_msm, msm_plan.hpp) and of the bucket lists its inputs make
// (dr::for_each_digit, msm_recode.hip.h) — both headers as the library compiles them.
//   te_msm_plan_check                 plan invariants over a sweep of sizes for the 253- and 252-bit orders, and the pinned
//                                     (c, W, H, groups) of every size the GPU tests and pedersen_verify_core's batches use
//   te_msm_plan_check hist <file>     <file>: blocks "case <name> <scalar_bits> <n>" + n reduced scalars (64 hex digits, big-endian).
//                                     Per case: the plan, and the bucket histogram of every (window, index group) set walked as
//                                     k_g1_sort_sets walks it with single == 0 — the longest list, lists longer than
//                                     TE_HEAVY_BUCKET (each with window, group, bucket, length, negative entries), lists of exactly
//                                     that length, entries in bucket H - 1 per window, scalars whose digits do not sum back to them.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "msm_plan.hpp"
#include "msm_recode.hip.h"

static int failures = 0;
#define CHECK(cond, ...)                                                  \
    do {                                                                  \
        if (!(cond)) {                                                    \
            if (failures++ < 20) {                                        \
                std::fprintf(stderr, "FAIL %s: ", #cond);                 \
                std::fprintf(stderr, __VA_ARGS__);                        \
                std::fprintf(stderr, "\n");                               \
            }                                                             \
        }                                                                 \
    } while (0)

// the index group bounds of k_g1_sort_sets: [ceil(g n / G), ceil((g + 1) n / G))
static uint32_t group_lo(uint64_t g, uint64_t n, uint64_t G) { return (uint32_t)((g * n + G - 1) / G); }

static void check_invariants(size_t n, int scalar_bits) {
    const dr::TeMsmPlan p = dr::plan_te_msm(n, scalar_bits);
    const dr::WindowTable& wt = p.wt;
    CHECK(wt.W >= 1 && wt.W <= dr::MAX_WINDOWS && wt.cmax <= p.c && wt.cmax >= dr::MIN_WINDOW && wt.odd == 0, "n=%zu bits=%d", n, scalar_bits);
    int sum = 0;
    for (int w = 0; w < wt.W; w++) {
        CHECK(wt.start[w] == sum, "n=%zu bits=%d window %d", n, scalar_bits, w);
        CHECK(wt.width[w] == wt.cmax || wt.width[w] == wt.cmax - 1, "n=%zu bits=%d window %d", n, scalar_bits, w);
        if (w) CHECK(wt.width[w] >= wt.width[w - 1], "n=%zu bits=%d window %d: the wider windows are on top", n, scalar_bits, w);
        sum += wt.width[w];
    }
    CHECK(sum == scalar_bits + 1, "n=%zu bits=%d: widths sum to %d", n, scalar_bits, sum);
    CHECK(wt.width[wt.W - 1] == wt.cmax, "n=%zu bits=%d", n, scalar_bits);
    CHECK(p.H == 1u << (wt.cmax - 1) && p.H <= dr::SORT_MAX_H, "n=%zu bits=%d H=%u", n, scalar_bits, p.H);
    CHECK(p.L > 0 && p.H % p.L == 0 && p.T * p.L == p.H, "n=%zu bits=%d H=%u L=%u", n, scalar_bits, p.H, p.L);
    CHECK(p.groups >= 1 && p.groups <= 64 && (p.groups & (p.groups - 1)) == 0, "n=%zu groups=%u", n, p.groups);
    CHECK(p.sets == (size_t)wt.W * p.groups && p.nbuckets == p.sets * p.H && p.nbuckets < (1ull << 31), "n=%zu", n);
    size_t covered = 0, largest = 0;
    for (uint32_t g = 0; g < p.groups; g++) {
        const uint32_t lo = group_lo(g, n, p.groups), hi = group_lo(g + 1, n, p.groups);
        CHECK(lo == covered && hi >= lo, "n=%zu group %u", n, g);
        covered = hi;
        largest = std::max<size_t>(largest, hi - lo);
    }
    CHECK(covered == n, "n=%zu: the groups cover %zu", n, covered);
    CHECK(p.per_set >= largest, "n=%zu per_set=%zu largest group %zu", n, p.per_set, largest);
    CHECK((uint64_t)p.sets * p.per_set < (1ull << 32), "n=%zu: set * capacity is computed in 32 bits", n);
}

static void pin(size_t n, int scalar_bits, int c, int W, uint32_t H, uint32_t groups) {
    const dr::TeMsmPlan p = dr::plan_te_msm(n, scalar_bits);
    if (!(p.c == c && p.wt.cmax == c && p.wt.W == W && p.H == H && p.groups == groups) && failures++ < 20)
        std::fprintf(stderr, "FAIL pin n=%zu bits=%d: c=%d cmax=%d W=%d H=%u groups=%u, expected %d %d %u %u\n", n, scalar_bits, p.c, p.wt.cmax,
                     p.wt.W, p.H, p.groups, c, W, H, groups);
}

static int plan_checks() {
    static_assert(dr::TE_HEAVY_BUCKET == 64, "a whole wave folds 64 lane sums: the tests' list lengths 64 / 65 are aimed at this");
    std::vector<size_t> ns = {1, 2, 63, 64, 255, 256, 257, 280, 300, 502, 511, 512, 513, 706, 1023, 1024, 1025, 1027, 1030, 2047, 2048, 2049,
                              4095, 4096, 4097, 5122, 8191, 8192, 16383, 16384, 16385, 20482, 32767, 32768, 65535, 65536, 65537};
    for (int e = 17; e <= 26; e++) ns.push_back(((size_t)1 << e) - 1), ns.push_back((size_t)1 << e), ns.push_back(((size_t)1 << e) + 1);
    ns.pop_back(), ns.pop_back();                       // te_msm_pippenger takes n < 2^26: the sweep ends at 2^26 - 1
    for (size_t n = 3; n < ((size_t)1 << 26); n = n * 3 + 7) ns.push_back(n);
    for (size_t n : ns)
        for (int bits : {253, 252}) check_invariants(n, bits);

    // ---- Bandersnatch (order of 253 bits: 254 bits tiled)
    // test_gpu_kernels.py: test_bsn_msm_pippenger_matches_oracle (5122 and 20482 = pedersen_verify_core's 5 B + 2 at B = 1024 and 4096) and
    // the all-zero case
    pin(256, 253, 7, 37, 64, 1), pin(257, 253, 7, 37, 64, 1), pin(300, 253, 7, 37, 64, 1), pin(1024, 253, 7, 37, 64, 2);
    pin(5122, 253, 8, 32, 128, 4), pin(20482, 253, 9, 29, 256, 8), pin(65536, 253, 10, 26, 512, 16);
    // test_gpu_te_msm.py: equal, lengths, cancel, verifier, top bucket, plan edges
    pin(1030, 253, 7, 37, 64, 2), pin(706, 253, 7, 37, 64, 1), pin(502, 253, 7, 37, 64, 1), pin(1027, 253, 7, 37, 64, 2);
    pin(4096, 253, 8, 32, 128, 4), pin(16384, 253, 9, 29, 256, 8);
    pin(1023, 253, 7, 37, 64, 1), pin(2047, 253, 7, 37, 64, 2), pin(2048, 253, 7, 37, 64, 4), pin(4095, 253, 7, 37, 64, 4);
    pin(16383, 253, 8, 32, 128, 8), pin(65535, 253, 9, 29, 256, 16);
    // ---- JubJub (order of 252 bits: 253 bits tiled): test_jubjub_scalar_mul_msm_and_groups_match_oracle's 280 terms, test_gpu_te_msm.py
    pin(280, 252, 7, 37, 64, 1), pin(256, 252, 7, 37, 64, 1), pin(300, 252, 7, 37, 64, 1), pin(706, 252, 7, 37, 64, 1);
    pin(1030, 252, 7, 37, 64, 2), pin(4096, 252, 8, 32, 128, 4);
    if (failures) {
        std::fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    std::printf("te msm plan ok: %zu sizes, heavy from %u\n", ns.size(), dr::TE_HEAVY_BUCKET + 1);
    return 0;
}

// ---- bucket histograms
static bool parse_scalar(const char* hex, uint32_t (&k)[9]) {
    if (std::strlen(hex) != 64) return false;
    for (int i = 0; i < 9; i++) k[i] = 0;
    for (int i = 0; i < 64; i++) {
        const char ch = hex[63 - i];                     // digit i from the low end
        const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
        if (v < 0) return false;
        k[i / 8] |= (uint32_t)v << (4 * (i % 8));
    }
    return true;
}

// acc (288 bits, two's complement) += d * 2^start
static void add_digit(uint32_t (&acc)[9], int32_t d, int start) {
    const uint64_t mag = (uint64_t)(d < 0 ? -(int64_t)d : (int64_t)d) << (start & 31);
    const uint32_t part[2] = {(uint32_t)mag, (uint32_t)(mag >> 32)};
    uint64_t carry = 0;
    for (int i = start >> 5, j = 0; i < 9; i++, j++) {
        const uint64_t v = j < 2 ? part[j] : 0;
        if (d >= 0) {
            const uint64_t s = (uint64_t)acc[i] + v + carry;
            acc[i] = (uint32_t)s, carry = s >> 32;
        } else {
            const uint64_t s = (uint64_t)acc[i] - v - carry;
            acc[i] = (uint32_t)s, carry = (s >> 32) & 1;
        }
    }
}

static int histograms(const char* path) {
    std::FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    char name[128], line[128];
    int bits;
    size_t n;
    while (std::fscanf(f, " case %127s %d %zu", name, &bits, &n) == 3) {
        std::vector<uint32_t> ks(n * 9);
        for (size_t i = 0; i < n; i++) {
            uint32_t k[9];
            if (std::fscanf(f, " %127s", line) != 1 || !parse_scalar(line, k)) { std::fprintf(stderr, "%s: bad scalar %zu\n", name, i); return 2; }
            std::memcpy(&ks[i * 9], k, sizeof k);
        }
        const dr::TeMsmPlan p = dr::plan_te_msm(n, bits);
        const dr::WindowTable& wt = p.wt;
        std::printf("case %s n=%zu c=%d W=%d H=%u groups=%u widths=", name, n, p.c, wt.W, p.H, p.groups);
        for (int w = 0; w < wt.W; w++) std::printf("%s%d", w ? "," : "", (int)wt.width[w]);
        // digits sum back to the scalar (all windows at once, as the reduced scalar is what every set's walk decodes)
        size_t bad = 0;
        for (size_t i = 0; i < n; i++) {
            uint32_t k[9], acc[9] = {0};
            std::memcpy(k, &ks[i * 9], sizeof k);
            dr::for_each_digit(k, wt, 0, wt.W, [&](int w, int32_t d) { add_digit(acc, d, wt.start[w]); });
            if (std::memcmp(acc, k, sizeof k) != 0) bad++;
        }
        size_t longest = 0, heavy = 0, exact = 0;
        std::vector<size_t> top(wt.W, 0);
        std::string heavy_lines;
        std::vector<uint32_t> bins(p.H), negs(p.H);
        for (int w = 0; w < wt.W; w++)
            for (uint32_t g = 0; g < p.groups; g++) {                 // set = w * groups + g
                std::fill(bins.begin(), bins.end(), 0u), std::fill(negs.begin(), negs.end(), 0u);
                const uint32_t lo = group_lo(g, n, p.groups), hi = group_lo(g + 1, n, p.groups);
                size_t entries = 0;
                for (uint32_t i = lo; i < hi; i++) {
                    uint32_t k[9];
                    std::memcpy(k, &ks[(size_t)i * 9], sizeof k);
                    dr::for_each_digit(k, wt, w, w + 1, [&](int, int32_t d) {
                        const uint32_t bin = (uint32_t)(d < 0 ? -d : d) - 1u;
                        if (bin >= p.H) { std::fprintf(stderr, "%s: digit %d outside the set\n", name, d); std::exit(2); }
                        bins[bin]++, negs[bin] += d < 0, entries++;
                    });
                }
                if (entries > p.per_set) { std::fprintf(stderr, "%s: set over capacity\n", name); return 2; }
                top[w] += bins[p.H - 1];
                for (uint32_t b = 0; b < p.H; b++) {
                    longest = std::max<size_t>(longest, bins[b]);
                    exact += bins[b] == dr::TE_HEAVY_BUCKET;
                    if (bins[b] > dr::TE_HEAVY_BUCKET) {
                        heavy++;
                        char buf[96];
                        std::snprintf(buf, sizeof buf, "heavy %d %u %u %u %u\n", w, g, b, bins[b], negs[b]);
                        heavy_lines += buf;
                    }
                }
            }
        std::printf(" heavy_from=%u longest=%zu heavy=%zu exact=%zu reconstruct_bad=%zu\ntop", dr::TE_HEAVY_BUCKET + 1, longest, heavy, exact, bad);
        for (int w = 0; w < wt.W; w++) std::printf(" %zu", top[w]);
        std::printf("\n%send\n", heavy_lines.c_str());
    }
    std::fclose(f);
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "hist") == 0) return histograms(argv[2]);
    if (argc != 1) { std::fprintf(stderr, "usage: %s [hist <file>]\n", argv[0]); return 2; }
    return plan_checks();
}
