// Host check of the wide suites' bucket method (dr_wide_msm): the plan (dr::plan_wide_msm, msm_plan.hpp), the digits
// (dr::wide_digit, wide_recode.hip.h) and the host's window combination (dr::wide_combine, wide_combine.hpp, over the four laws) — all
// headers as the library compiles them.
//   wide_msm_plan_check                   plan invariants over a sweep of sizes from WIDE_PIP_FROM to 2^20 for 385, 449 and 522 tiled bits,
//                                         and the pinned (c, W, H, groups) of the sizes the GPU tests use
//   wide_msm_plan_check hist <file>       <file>: blocks "case <name> <bits> <scalar words> <n of the plan> <count>" + count scalars (hex,
//                                         big-endian, the terms 0 .. count - 1 of an MSM of n; "<hex>*<times>" stands for that many
//                                         equal scalars in a row; <file> "-" is the standard input).  Per case: the plan, the scalars whose
//                                         digits do not sum back to them, and the bucket histogram of every (window, index group) set
//                                         walked as wave_msm_sort walks it: the longest list, every list of TE_HEAVY_BUCKET entries or
//                                         more (window, group, bucket, length, negative entries), entries in bucket H - 1 per window.
//   wide_msm_plan_check combine <file>    <file>: blocks "sums <suite> <n>" + W x groups set sums in the suite's ABI bytes (hex, as in
//                                         memory; window-major).  Per block: the combined point in ABI bytes.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "msm_plan.hpp"
#include "wide_combine.hpp"
#include "p384_law.hip.h"
#include "p521_law.hip.h"
#include "e448_law.hip.h"
#include "c448_law.hip.h"

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

// the index group bounds of wave_msm_sort: [ceil(g n / G), ceil((g + 1) n / G))
static uint32_t group_lo(uint64_t g, uint64_t n, uint64_t G) { return (uint32_t)((g * n + G - 1) / G); }

static void check_invariants(size_t n, int bits) {
    const dr::WideMsmPlan p = dr::plan_wide_msm(n, bits);
    const dr::WideTiling& wt = p.wt;
    const int cmax = dr::wide_cmax(wt);
    CHECK(wt.W >= 1 && cmax <= p.c && cmax >= 6 && wt.bits == bits, "n=%zu bits=%d", n, bits);
    int sum = 0;
    for (int w = 0; w < wt.W; w++) {
        const int width = dr::wide_width(wt, w);
        CHECK(dr::wide_start(wt, w) == sum, "n=%zu bits=%d window %d", n, bits, w);
        CHECK(width == cmax || width == cmax - 1, "n=%zu bits=%d window %d", n, bits, w);
        if (w) CHECK(width >= dr::wide_width(wt, w - 1), "n=%zu bits=%d window %d: the wider windows are on top", n, bits, w);
        sum += width;
    }
    CHECK(sum == bits, "n=%zu bits=%d: widths sum to %d", n, bits, sum);
    CHECK(dr::wide_width(wt, wt.W - 1) == cmax, "n=%zu bits=%d", n, bits);
    CHECK(p.H == 1u << (cmax - 1) && p.H <= dr::WIDE_MAX_H, "n=%zu bits=%d H=%u", n, bits, p.H);
    CHECK(p.L > 0 && p.H % p.L == 0 && p.T * p.L == p.H, "n=%zu bits=%d H=%u L=%u", n, bits, p.H, p.L);
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
    CHECK((uint64_t)p.sets * p.per_set < (1ull << 31), "n=%zu: set * capacity is computed in 32 bits", n);
}

static void pin(size_t n, int bits, int c, int W, uint32_t H, uint32_t groups) {
    const dr::WideMsmPlan p = dr::plan_wide_msm(n, bits);
    if (!(p.c == c && dr::wide_cmax(p.wt) == c && p.wt.W == W && p.H == H && p.groups == groups) && failures++ < 20)
        std::fprintf(stderr, "FAIL pin n=%zu bits=%d: c=%d cmax=%d W=%d H=%u groups=%u, expected %d %d %u %u\n", n, bits, p.c,
                     dr::wide_cmax(p.wt), p.wt.W, p.H, p.groups, c, W, H, groups);
}

static int plan_checks() {
    static_assert(dr::TE_HEAVY_BUCKET == 64, "a whole wave folds 64 lane sums: the tests' list lengths 64 / 65 are aimed at this");
    static_assert(dr::WIDE_PIP_FROM == 256, "the GPU tests' smallest size");
    std::vector<size_t> ns;
    for (size_t n = dr::WIDE_PIP_FROM; n <= 4200; n++) ns.push_back(n);
    for (int e = 13; e <= 20; e++) ns.push_back(((size_t)1 << e) - 1), ns.push_back((size_t)1 << e), ns.push_back(((size_t)1 << e) + 1);
    ns.pop_back();                                           // the sweep ends at 2^20
    for (size_t n = 4201; n < ((size_t)1 << 20); n = n * 3 / 2 + 7) ns.push_back(n);
    for (size_t n : ns)
        for (int bits : {385, 449, 522}) check_invariants(n, bits);
    // the sizes of tests/test_gpu_wide_msm.py: one index group, two, and the second window width
    pin(256, 385, 7, 55, 64, 1);  pin(1030, 385, 7, 55, 64, 2);  pin(4100, 385, 8, 49, 128, 4);
    pin(256, 449, 7, 65, 64, 1);  pin(1030, 449, 7, 65, 64, 2);  pin(4100, 449, 8, 57, 128, 4);
    pin(256, 522, 7, 75, 64, 1);  pin(1030, 522, 7, 75, 64, 2);  pin(4100, 522, 8, 66, 128, 4);
    pin(300, 385, 7, 55, 64, 1);  pin(320, 449, 7, 65, 64, 1);   pin(320, 522, 7, 75, 64, 1);      // point_type.msm, batch_verify of 64 proofs
    pin(1023, 522, 7, 75, 64, 1); pin(1024, 522, 7, 75, 64, 2);  pin(4095, 385, 7, 55, 64, 4);     // the thresholds themselves
    pin(16384, 449, 9, 50, 256, 8); pin(65536, 522, 10, 53, 512, 16);
    // the sizes of tests/test_gpu_wide_msm_plans.py: widths 9 and 10, 8 to 64 index groups, and no size a multiple of its group count
    struct Upper { size_t n; int c, w385, w449, w522; uint32_t H, groups; };
    for (const Upper& u : {Upper{1031, 7, 55, 65, 75, 64, 2}, Upper{4103, 8, 49, 57, 66, 128, 4}, Upper{16383, 8, 49, 57, 66, 128, 8},
                           Upper{16387, 9, 43, 50, 58, 256, 8}, Upper{65535, 9, 43, 50, 58, 256, 16}, Upper{65539, 10, 39, 45, 53, 512, 16},
                           Upper{131075, 10, 39, 45, 53, 512, 32}, Upper{262147, 10, 39, 45, 53, 512, 64}}) {
        pin(u.n, 385, u.c, u.w385, u.H, u.groups); pin(u.n, 449, u.c, u.w449, u.H, u.groups); pin(u.n, 522, u.c, u.w522, u.H, u.groups);
        CHECK(u.n % u.groups != 0, "n=%zu: the group bounds are to be ceilings that differ from the floors", u.n);
    }
    CHECK(dr::plan_wide_msm(16387, 522).wt.rem == 0 && dr::plan_wide_msm(65535, 522).wt.rem == 0, "522 = 58 x 9: every window of full width");
    CHECK(dr::plan_wide_msm(65539, 522).H == dr::WIDE_MAX_H && dr::plan_wide_msm(262147, 385).groups == 64, "the largest set and the group cap");
    if (failures == 0) std::printf("wide msm plan ok: %zu sizes, heavy from %u\n", ns.size(), dr::TE_HEAVY_BUCKET + 1);
    return failures ? 1 : 0;
}

// ---------------------------------------------------------------- digits and histograms
static bool hex_words(const char* hex, int kw, std::vector<uint32_t>& k) {
    const size_t len = std::strlen(hex);
    k.assign(kw, 0);
    for (size_t i = 0; i < len; i++) {
        const char ch = hex[len - 1 - i];
        const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
        if (v < 0 || (v && i / 8 >= (size_t)kw)) return false;
        if (i / 8 < (size_t)kw) k[i / 8] |= (uint32_t)v << (4 * (i % 8));
    }
    return true;
}

// sum_w d_w 2^start_w == k, with nothing left above the scalar's words
static bool reconstructs(const std::vector<uint32_t>& k, int kw, const dr::WideTiling& wt) {
    std::vector<int64_t> acc(kw + 2, 0);
    for (int w = 0; w < wt.W; w++) {
        const int start = dr::wide_start(wt, w);
        const int64_t d = dr::wide_digit(k.data(), kw, start, dr::wide_width(wt, w));
        acc[start >> 5] += d * ((int64_t)1 << (start & 31));
    }
    int64_t carry = 0;
    for (int i = 0; i < kw + 2; i++) {
        const int64_t v = acc[i] + carry;
        const int64_t low = v & 0xffffffffll;
        carry = (v - low) / ((int64_t)1 << 32);
        if (low != (i < kw ? (int64_t)k[i] : 0)) return false;
    }
    return carry == 0;
}

static int histograms(const char* path) {
    FILE* f = std::strcmp(path, "-") == 0 ? stdin : std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    char name[128];
    int bits, kw;
    size_t n, count;
    std::vector<char> line(4096);
    while (std::fscanf(f, " case %127s %d %d %zu %zu", name, &bits, &kw, &n, &count) == 5) {
        std::vector<std::vector<uint32_t>> ks(count);
        for (size_t i = 0; i < count;) {
            if (std::fscanf(f, " %4095s", line.data()) != 1) { std::fprintf(stderr, "%s: scalar %zu is missing\n", name, i); return 2; }
            size_t times = 1;
            if (char* star = std::strchr(line.data(), '*')) {
                *star = 0;
                times = std::strtoull(star + 1, nullptr, 10);
            }
            if (times == 0 || times > count - i || !hex_words(line.data(), kw, ks[i])) {
                std::fprintf(stderr, "%s: bad scalar %zu\n", name, i);
                return 2;
            }
            for (size_t j = 1; j < times; j++) ks[i + j] = ks[i];
            i += times;
        }
        if (count > n) { std::fprintf(stderr, "%s: more scalars than terms\n", name); return 2; }
        const dr::WideMsmPlan p = dr::plan_wide_msm(n, bits);
        const dr::WideTiling& wt = p.wt;
        size_t bad = 0;
        for (size_t i = 0; i < count; i++) bad += reconstructs(ks[i], kw, wt) ? 0 : 1;
        uint32_t longest = 0;
        size_t heavy = 0;
        std::vector<uint32_t> top(wt.W, 0);
        std::string lists;
        for (int w = 0; w < wt.W; w++) {
            const int start = dr::wide_start(wt, w), width = dr::wide_width(wt, w);
            for (uint32_t g = 0; g < p.groups; g++) {
                std::vector<uint32_t> len(p.H, 0), negs(p.H, 0);
                const uint32_t lo = group_lo(g, n, p.groups), hi = group_lo(g + 1, n, p.groups);
                for (uint32_t i = lo; i < hi && i < count; i++) {
                    const int32_t d = dr::wide_digit(ks[i].data(), kw, start, width);
                    if (d == 0) continue;
                    const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u;
                    if (b >= p.H) { std::fprintf(stderr, "%s: digit %d of window %d has no bucket\n", name, d, w); return 2; }
                    len[b]++;
                    if (d < 0) negs[b]++;
                }
                top[w] += len[p.H - 1];
                for (uint32_t b = 0; b < p.H; b++) {
                    longest = std::max(longest, len[b]);
                    if (len[b] > dr::TE_HEAVY_BUCKET) heavy++;
                    if (len[b] >= dr::TE_HEAVY_BUCKET) {
                        char buf[96];
                        std::snprintf(buf, sizeof buf, "list %d %u %u %u %u\n", w, g, b, len[b], negs[b]);
                        lists += buf;
                    }
                }
            }
        }
        std::printf("case %s n=%zu c=%d W=%d H=%u groups=%u cmax=%d base=%d rem=%d reconstruct_bad=%zu longest=%u heavy=%zu\n", name, n, p.c, wt.W,
                    p.H, p.groups, dr::wide_cmax(wt), wt.base, wt.rem, bad, longest, heavy);
        std::printf("top");
        for (int w = 0; w < wt.W; w++) std::printf(" %u", top[w]);
        std::printf("\n%s", lists.c_str());
    }
    std::fclose(f);
    return 0;
}

// ---------------------------------------------------------------- the host's window combination
template <class Law>
static int combine_block(FILE* f, size_t n, int bits) {
    constexpr int PW = 2 * Law::WORDS;
    const dr::WideMsmPlan p = dr::plan_wide_msm(n, bits);
    std::vector<typename Law::Point> sums(p.sets);
    std::vector<char> line(4096);
    for (size_t s = 0; s < p.sets; s++) {
        if (std::fscanf(f, " %4095s", line.data()) != 1 || std::strlen(line.data()) != (size_t)PW * 8) return 2;
        uint32_t w[PW] = {};
        for (int b = 0; b < PW * 4; b++) {
            unsigned v;
            if (std::sscanf(line.data() + 2 * b, "%2x", &v) != 1) return 2;
            w[b / 4] |= (uint32_t)v << (8 * (b % 4));
        }
        // through a record of limb images, as the set sums leave the device
        const typename Law::Point pt = Law::from_abi(w);
        uint32_t rec[dr::wide_record_words<Law>()] = {};
        for (int i = 0; i < Law::LIMBS; i++) {
            rec[i] = (uint32_t)pt.x.l[i]; rec[Law::LIMBS + i] = (uint32_t)pt.y.l[i]; rec[2 * Law::LIMBS + i] = (uint32_t)pt.z.l[i];
        }
        sums[s] = dr::wide_record_point<Law>(rec);
    }
    uint32_t out[PW];
    Law::to_abi(dr::wide_combine<Law>(sums.data(), p.wt, p.groups), out);
    for (int b = 0; b < PW * 4; b++) std::printf("%02x", (out[b / 4] >> (8 * (b % 4))) & 0xffu);
    std::printf("\n");
    return 0;
}

static int combines(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    char suite[32];
    size_t n;
    int rc = 0;
    while (rc == 0 && std::fscanf(f, " sums %31s %zu", suite, &n) == 2) {
        const std::string s = suite;
        if (s == "p384") rc = combine_block<dr::P384Law>(f, n, 385);
        else if (s == "p521") rc = combine_block<dr::P521Law>(f, n, 522);
        else if (s == "ed448") rc = combine_block<dr::E448Law>(f, n, 449);
        else if (s == "curve448") rc = combine_block<dr::M448Law>(f, n, 449);
        else rc = 2;
    }
    std::fclose(f);
    if (rc) std::fprintf(stderr, "bad combine input\n");
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "hist") == 0) return histograms(argv[2]);
    if (argc == 3 && std::strcmp(argv[1], "combine") == 0) return combines(argv[2]);
    return plan_checks();
}
