// Host check of the bucket method under dr_te_msm (Ed25519, Baby JubJub, P-256, secp256k1, Curve25519) and dr_blsg1_msm (BLS12-381's
// E(Fq)): the plan (dr::plan_wide_msm over 252 / 254 / 257 tiled bits, from dr::NARROW_PIP_FROM), the digits of scalars reduced as the
// host path reduces them (drh::Mod256::reduce_bytes; E(Fq): as they are), the host laws (narrow_law.hpp) and dr::wide_combine over them
// — all headers as the library compiles them.  Suites: ed25519, bjj, p256, secp256k1, curve25519 (Edwards points in, u || v out), blsg1.
//   narrow_msm_host_check                 plan invariants from the threshold to 4200 and a sweep to 2^20, and the pinned plans of the
//                                         sizes the GPU tests use
//   narrow_msm_host_check hist <file>     blocks "case <name> <suite> <n of the plan> <count>" + count scalars (hex, big-endian, up to
//                                         256 bits; "<hex>*<times>" repeats one).  Per case the plan, the scalars whose digits do not sum
//                                         back to the REDUCED scalar, and the histogram of every (window, index group) set as
//                                         wave_msm_sort walks it: "list <window> <group> <bucket> <length> <negative entries>" for every
//                                         list of TE_HEAVY_BUCKET entries or more.  <file> "-" is the standard input.
//   narrow_msm_host_check law <file>      lines "<suite> <P> <Q>", points in ABI bytes (hex, as in memory).  Per line: add(P, Q), dbl(P)
//                                         and add(add(P, Q), dbl(P)) (projective operands) in ABI bytes.
//   narrow_msm_host_check combine <file>  blocks "sums <suite> <n>" + W x groups set sums in ABI bytes (window-major): the combined point.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "msm_plan.hpp"
#include "narrow_law.hpp"
#include "wide_combine.hpp"

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

static uint32_t group_lo(uint64_t g, uint64_t n, uint64_t G) { return (uint32_t)((g * n + G - 1) / G); }

static void check_invariants(size_t n, int bits) {
    const dr::WideMsmPlan p = dr::plan_wide_msm(n, bits);
    const dr::WideTiling& wt = p.wt;
    const int cmax = dr::wide_cmax(wt);
    CHECK(wt.W >= 1 && cmax <= p.c && cmax >= 6 && wt.bits == bits, "n=%zu bits=%d", n, bits);
    int sum = 0;
    for (int w = 0; w < wt.W; w++) {
        const int width = dr::wide_width(wt, w);
        CHECK(dr::wide_start(wt, w) == sum && (width == cmax || width == cmax - 1), "n=%zu bits=%d window %d", n, bits, w);
        if (w) CHECK(width >= dr::wide_width(wt, w - 1), "n=%zu bits=%d window %d: the wider windows are on top", n, bits, w);
        sum += width;
    }
    CHECK(sum == bits && dr::wide_width(wt, wt.W - 1) == cmax, "n=%zu bits=%d: widths sum to %d", n, bits, sum);
    CHECK(p.H == 1u << (cmax - 1) && p.H <= dr::WIDE_MAX_H && p.L > 0 && p.T * p.L == p.H, "n=%zu bits=%d H=%u L=%u", n, bits, p.H, p.L);
    CHECK(p.groups >= 1 && p.groups <= 64 && (p.groups & (p.groups - 1)) == 0, "n=%zu groups=%u", n, p.groups);
    CHECK(p.sets == (size_t)wt.W * p.groups && p.nbuckets == p.sets * p.H && p.nbuckets < (1ull << 31), "n=%zu", n);
    size_t covered = 0, largest = 0;
    for (uint32_t g = 0; g < p.groups; g++) {
        const uint32_t lo = group_lo(g, n, p.groups), hi = group_lo(g + 1, n, p.groups);
        CHECK(lo == covered && hi >= lo, "n=%zu group %u", n, g);
        covered = hi;
        largest = std::max<size_t>(largest, hi - lo);
    }
    CHECK(covered == n && p.per_set >= largest && (uint64_t)p.sets * p.per_set < (1ull << 31), "n=%zu", n);
}

static void pin(size_t n, int bits, int c, int W, uint32_t H, uint32_t groups) {
    const dr::WideMsmPlan p = dr::plan_wide_msm(n, bits);
    if (!(p.c == c && dr::wide_cmax(p.wt) == c && p.wt.W == W && p.H == H && p.groups == groups) && failures++ < 20)
        std::fprintf(stderr, "FAIL pin n=%zu bits=%d: c=%d cmax=%d W=%d H=%u groups=%u, expected %d %d %u %u\n", n, bits, p.c,
                     dr::wide_cmax(p.wt), p.wt.W, p.H, p.groups, c, W, H, groups);
}

static int plan_checks() {
    static_assert(dr::TE_HEAVY_BUCKET == 64, "a whole wave folds 64 lane sums: the tests' list lengths 64 / 65 are aimed at this");
    static_assert(dr::NARROW_PIP_FROM >= 257, "a dr_te_msm of 256 terms is recorded as two msm_groups launches");
    std::vector<size_t> ns;
    for (size_t n = dr::NARROW_PIP_FROM; n <= 4200; n++) ns.push_back(n);
    for (int e = 13; e <= 20; e++) ns.push_back(((size_t)1 << e) - 1), ns.push_back((size_t)1 << e), ns.push_back(((size_t)1 << e) + 1);
    ns.pop_back();                                           // the sweep ends at 2^20
    for (size_t n = 4201; n < ((size_t)1 << 20); n = n * 3 / 2 + 7) ns.push_back(n);
    for (size_t n : ns)
        for (int bits : {252, 254, 257}) check_invariants(n, bits);
    // the sizes of tests/test_gpu_narrow_msm.py: (c, W at 252 / 254 / 257 bits, H, index groups)
    struct Pin { size_t n; int c, w252, w254, w257; uint32_t H, groups; };
    for (const Pin& u : {Pin{dr::NARROW_PIP_FROM, 7, 36, 37, 37, 64, 1}, Pin{2 * dr::NARROW_PIP_FROM, 7, 36, 37, 37, 64, 1},
                         Pin{1031, 7, 36, 37, 37, 64, 2}, Pin{4103, 8, 32, 32, 33, 128, 4}, Pin{16387, 9, 28, 29, 29, 256, 8},
                         Pin{65539, 10, 26, 26, 26, 512, 16}}) {
        pin(u.n, 252, u.c, u.w252, u.H, u.groups); pin(u.n, 254, u.c, u.w254, u.H, u.groups); pin(u.n, 257, u.c, u.w257, u.H, u.groups);
    }
    for (size_t n : {(size_t)1031, (size_t)4103, (size_t)16387, (size_t)65539})
        CHECK(n % dr::plan_wide_msm(n, 257).groups != 0, "n=%zu: the group bounds are to be ceilings that differ from the floors", n);
    if (failures == 0) std::printf("narrow msm plan ok: %zu sizes from %zu, heavy from %u\n", ns.size(), (size_t)dr::NARROW_PIP_FROM, dr::TE_HEAVY_BUCKET + 1);
    return failures ? 1 : 0;
}

// ---------------------------------------------------------------- suites
struct SuiteInfo { int bits; const drh::Mod256* order; };       // order: what the host path reduces scalars by (null: none)
static bool suite_info(const std::string& s, SuiteInfo& out) {
    if (s == "ed25519" || s == "curve25519") out = {254, &drh::te_curve(3)->n};
    else if (s == "bjj") out = {252, &drh::te_curve(5)->n};
    else if (s == "p256") out = {257, &drh::te_curve(4)->n};
    else if (s == "secp256k1") out = {257, &drh::te_curve(6)->n};
    else if (s == "blsg1") out = {257, nullptr};
    else return false;
    return true;
}
template <class F>
static int with_law(const std::string& s, F&& f) {
    if (s == "ed25519") return f(dr::Ed25519Law{});
    if (s == "curve25519") return f(dr::C25519Law{});
    if (s == "bjj") return f(dr::BjjLaw{});
    if (s == "p256") return f(dr::P256Law{});
    if (s == "secp256k1") return f(dr::Secp256k1Law{});
    if (s == "blsg1") return f(dr::G1hLaw{});
    return 2;
}

// ---------------------------------------------------------------- digits and histograms
// big-endian hex of up to 256 bits -> 32 little-endian bytes
static bool hex_le32(const char* hex, uint8_t out[32]) {
    const size_t len = std::strlen(hex);
    std::memset(out, 0, 32);
    if (len == 0 || len > 64) return false;
    for (size_t i = 0; i < len; i++) {
        const char ch = hex[len - 1 - i];
        const int v = ch >= '0' && ch <= '9' ? ch - '0' : ch >= 'a' && ch <= 'f' ? ch - 'a' + 10 : -1;
        if (v < 0) return false;
        out[i / 2] |= (uint8_t)(v << (4 * (i % 2)));
    }
    return true;
}
// the words the sort kernel reads: reduced as native_msm reduces them
static void scalar_words(const uint8_t le[32], const drh::Mod256* order, uint32_t k[8]) {
    uint8_t b[32];
    std::memcpy(b, le, 32);
    if (order) {
        uint64_t v[4];
        drh::load_le32(le, v);
        if (drh::Mod256::geq(v, order->m)) order->reduce_bytes(le, 32, false, v);
        drh::store_le32(v, b);
    }
    std::memcpy(k, b, 32);
}
// sum_w d_w 2^start_w == k, with nothing left above the scalar's words
static bool reconstructs(const uint32_t k[8], const dr::WideTiling& wt) {
    int64_t acc[10] = {};
    for (int w = 0; w < wt.W; w++) {
        const int start = dr::wide_start(wt, w);
        const int64_t d = dr::wide_digit(k, 8, start, dr::wide_width(wt, w));
        acc[start >> 5] += d * ((int64_t)1 << (start & 31));
    }
    int64_t carry = 0;
    for (int i = 0; i < 10; i++) {
        const int64_t v = acc[i] + carry;
        const int64_t low = v & 0xffffffffll;
        carry = (v - low) / ((int64_t)1 << 32);
        if (low != (i < 8 ? (int64_t)k[i] : 0)) return false;
    }
    return carry == 0;
}

static int histograms(const char* path) {
    FILE* f = std::strcmp(path, "-") == 0 ? stdin : std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    char name[128], suite[32];
    size_t n, count;
    std::vector<char> line(512);
    while (std::fscanf(f, " case %127s %31s %zu %zu", name, suite, &n, &count) == 4) {
        SuiteInfo si;
        if (!suite_info(suite, si) || count > n) { std::fprintf(stderr, "%s: bad case\n", name); return 2; }
        std::vector<uint32_t> ks(count * 8);
        for (size_t i = 0; i < count;) {
            if (std::fscanf(f, " %511s", line.data()) != 1) { std::fprintf(stderr, "%s: scalar %zu is missing\n", name, i); return 2; }
            size_t times = 1;
            if (char* star = std::strchr(line.data(), '*')) {
                *star = 0;
                times = std::strtoull(star + 1, nullptr, 10);
            }
            uint8_t le[32];
            if (times == 0 || times > count - i || !hex_le32(line.data(), le)) { std::fprintf(stderr, "%s: bad scalar %zu\n", name, i); return 2; }
            scalar_words(le, si.order, &ks[i * 8]);
            for (size_t j = 1; j < times; j++) std::memcpy(&ks[(i + j) * 8], &ks[i * 8], 32);
            i += times;
        }
        const dr::WideMsmPlan p = dr::plan_wide_msm(n, si.bits);
        const dr::WideTiling& wt = p.wt;
        size_t bad = 0, heavy = 0;
        for (size_t i = 0; i < count; i++) bad += reconstructs(&ks[i * 8], wt) ? 0 : 1;
        uint32_t longest = 0;
        std::string lists;
        for (int w = 0; w < wt.W; w++) {
            const int start = dr::wide_start(wt, w), width = dr::wide_width(wt, w);
            for (uint32_t g = 0; g < p.groups; g++) {
                std::vector<uint32_t> len(p.H, 0), negs(p.H, 0);
                const uint32_t lo = group_lo(g, n, p.groups), hi = group_lo(g + 1, n, p.groups);
                for (uint32_t i = lo; i < hi && i < count; i++) {
                    const int32_t d = dr::wide_digit(&ks[(size_t)i * 8], 8, start, width);
                    if (d == 0) continue;
                    const uint32_t b = (uint32_t)(d < 0 ? -d : d) - 1u;
                    if (b >= p.H) { std::fprintf(stderr, "%s: digit %d of window %d has no bucket\n", name, d, w); return 2; }
                    len[b]++;
                    if (d < 0) negs[b]++;
                }
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
        std::printf("case %s n=%zu c=%d W=%d H=%u groups=%u cmax=%d reconstruct_bad=%zu longest=%u heavy=%zu\n%s", name, n, p.c, wt.W, p.H,
                    p.groups, dr::wide_cmax(wt), bad, longest, heavy, lists.c_str());
    }
    if (f != stdin) std::fclose(f);
    return 0;
}

// ---------------------------------------------------------------- the laws and the combination
template <int PW>
static bool hex_point(const char* hex, uint32_t (&w)[PW]) {
    if (std::strlen(hex) != (size_t)PW * 8) return false;
    std::memset(w, 0, sizeof w);
    for (int b = 0; b < PW * 4; b++) {
        unsigned v;
        if (std::sscanf(hex + 2 * b, "%2x", &v) != 1) return false;
        w[b / 4] |= (uint32_t)v << (8 * (b % 4));
    }
    return true;
}
template <class Law>
static void print_point(const typename Law::Point& p, char end) {
    uint32_t out[2 * Law::WORDS];
    Law::to_abi(p, out);
    for (int b = 0; b < 8 * Law::WORDS; b++) std::printf("%02x", (out[b / 4] >> (8 * (b % 4))) & 0xffu);
    std::printf("%c", end);
}

static int laws(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    char suite[32];
    std::vector<char> a(512), b(512);
    int rc = 0;
    while (rc == 0 && std::fscanf(f, " %31s %511s %511s", suite, a.data(), b.data()) == 3) {
        rc = with_law(suite, [&](auto law) {
            using Law = decltype(law);
            uint32_t pw[2 * Law::WORDS], qw[2 * Law::WORDS];
            if (!hex_point(a.data(), pw) || !hex_point(b.data(), qw)) return 2;
            const auto P = Law::from_abi(pw), Q = Law::from_abi(qw);
            const auto S = Law::add(P, Q), D = Law::dbl(P);
            print_point<Law>(S, ' ');
            print_point<Law>(D, ' ');
            print_point<Law>(Law::add(S, D), '\n');
            return 0;
        });
    }
    std::fclose(f);
    if (rc) std::fprintf(stderr, "bad law input\n");
    return rc;
}

static int combines(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    char suite[32];
    size_t n;
    int rc = 0;
    std::vector<char> line(512);
    while (rc == 0 && std::fscanf(f, " sums %31s %zu", suite, &n) == 2) {
        SuiteInfo si;
        if (!suite_info(suite, si)) { rc = 2; break; }
        rc = with_law(suite, [&](auto law) {
            using Law = decltype(law);
            const dr::WideMsmPlan p = dr::plan_wide_msm(n, si.bits);
            std::vector<typename Law::Point> sums(p.sets);
            for (size_t s = 0; s < p.sets; s++) {
                uint32_t w[2 * Law::WORDS];
                if (std::fscanf(f, " %511s", line.data()) != 1 || !hex_point(line.data(), w)) return 2;
                sums[s] = Law::from_abi(w);
            }
            print_point<Law>(dr::wide_combine<Law>(sums.data(), p.wt, p.groups), '\n');
            return 0;
        });
    }
    std::fclose(f);
    if (rc) std::fprintf(stderr, "bad combine input\n");
    return rc;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "hist") == 0) return histograms(argv[2]);
    if (argc == 3 && std::strcmp(argv[1], "law") == 0) return laws(argv[2]);
    if (argc == 3 && std::strcmp(argv[1], "combine") == 0) return combines(argv[2]);
    return plan_checks();
}
