// Stand-alone check of hostrecords.hpp (no HIP, no GPU): built by tests/test_io_records_cpu.py with g++ under the address and
// undefined-behaviour sanitizers.  Every vector is sized exactly, so a read or write past a record or a flag word is a sanitizer error.
// Prints one line per checked shape and exits 0, or says what differs and exits 1.
#include <cstdio>
#include <cstdlib>

#include "hostrecords.hpp"

static int failures = 0;
#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::printf("FAILED line %d: %s\n", __LINE__, #cond);           \
            failures++;                                                     \
        }                                                                   \
    } while (0)

static std::vector<uint8_t> pattern(size_t bytes, unsigned seed) {
    std::vector<uint8_t> v(bytes);
    for (size_t i = 0; i < bytes; i++) v[i] = (uint8_t)(1 + (i * 7 + seed) % 250);       // never 0x00, never 0xff
    return v;
}

static void check_pad(size_t n, size_t enc, size_t rec) {
    const std::vector<uint8_t> in = pattern(n * enc, (unsigned)(n + enc));
    const std::vector<uint8_t> out = drh::pad_records(in.data(), n, enc, rec);
    CHECK(out.size() == n * rec);
    for (size_t i = 0; i < n; i++) {
        CHECK(std::memcmp(out.data() + rec * i, in.data() + enc * i, enc) == 0);
        for (size_t j = enc; j < rec; j++) CHECK(out[rec * i + j] == 0);
    }
    std::printf("pad n=%zu %zu->%zu\n", n, enc, rec);
}

// marks: one character per point, '1' the identity; `given`: as the caller's flag bytes (`null_marks`: a null pointer, for no identity),
// otherwise as points of 0xff bytes
static void check_split(const char* marks, bool given, bool null_marks = false) {
    const size_t n = std::strlen(marks), pt = 64;
    std::vector<uint8_t> pts = pattern(n * pt, (unsigned)n), bytes(n);
    bool any = false;
    for (size_t i = 0; i < n; i++) {
        bytes[i] = marks[i] == '1' ? (uint8_t)(1 + i) : 0;                  // (any non-zero byte marks)
        any = any || bytes[i];
        if (!given && bytes[i]) std::memset(pts.data() + pt * i, 0xff, pt);
    }
    if (n) pts[pt - 1] = 0xff;                                               // (one 0xff byte more or less does not make an identity)
    const std::vector<uint8_t> before = pts;
    std::vector<uint8_t> clean;
    std::vector<uint32_t> flags(7, 9);                                       // (stale contents are replaced)
    drh::split_identities(n ? pts.data() : nullptr, n, pt, given, null_marks ? nullptr : bytes.data(), clean, flags);
    CHECK(pts == before);
    CHECK(flags.size() == n);
    CHECK(clean.empty() == !any);
    for (size_t i = 0; i < n; i++) {
        CHECK(flags[i] == (bytes[i] ? 1u : 0u));
        if (!any) continue;
        CHECK(clean.size() == n * pt);
        for (size_t j = 0; j < pt; j++) CHECK(clean[pt * i + j] == (bytes[i] ? 0 : before[pt * i + j]));
    }
    std::printf("split \"%s\" %s\n", marks, null_marks ? "null" : given ? "given" : "ff");
}

int main() {
    for (size_t n : {0, 1, 3}) {
        check_pad(n, 33, 36);
        check_pad(n, 32, 32);
    }
    for (const char* marks : {"", "0", "1", "000", "111", "010", "101"}) {
        check_split(marks, true);
        check_split(marks, false);
    }
    // the caller's flags absent: none is the identity
    for (const char* marks : {"", "0", "000"}) check_split(marks, true, true);
    // ... even a point of 0xff bytes (the coordinate check refuses it later)
    {
        std::vector<uint8_t> pts(3 * 64, 0xff), clean;
        std::vector<uint32_t> flags;
        drh::split_identities(pts.data(), 3, 64, true, nullptr, clean, flags);
        CHECK(clean.empty() && flags == std::vector<uint32_t>(3, 0));
        std::printf("split null marks\n");
    }
    CHECK(drh::all_ff(nullptr, 0));
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
