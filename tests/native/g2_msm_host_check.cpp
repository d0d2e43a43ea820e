// Host check of the bucket method under dr_blsg2_msm (BLS12-381's E(Fq2)): dr::G2hLaw (csrc/g2_law.hpp) — add, dbl, from_abi, to_abi —
// and dr::wide_combine over it with the plan dr::plan_wide_msm makes for 257 tiled bits, from the library's own headers.
// tests/test_g2_msm_cpu.py compiles this with g++ -fsanitize=undefined and compares what it prints with the big-integer restatement.
//   g2_msm_host_check law FILE       lines "P Q" (192-byte points as 384 hex digits) -> "P+Q 2P (P+Q)+2P" through from_abi / to_abi
//   g2_msm_host_check combine FILE   blocks "sums N" followed by the W x G set sums of the plan for N terms -> their combination
//   g2_msm_host_check                the threshold and the plans of the sizes the GPU tests use
#include <cstdio>
#include <cstring>
#include <vector>

#include "g2_law.hpp"
#include "msm_plan.hpp"
#include "wide_combine.hpp"

using Law = dr::G2hLaw;
constexpr int PW = 2 * Law::WORDS, HEX = 8 * PW;
constexpr int BITS = 257;

static bool hex_point(const char* hex, uint32_t (&w)[PW]) {
    if (std::strlen(hex) != (size_t)HEX) return false;
    std::memset(w, 0, sizeof w);
    for (int b = 0; b < PW * 4; b++) {
        unsigned v;
        if (std::sscanf(hex + 2 * b, "%2x", &v) != 1) return false;
        w[b / 4] |= (uint32_t)v << (8 * (b % 4));
    }
    return true;
}
static void print_point(const Law::Point& p, char end) {
    uint32_t out[PW];
    Law::to_abi(p, out);
    for (int b = 0; b < 4 * PW; b++) std::printf("%02x", (out[b / 4] >> (8 * (b % 4))) & 0xffu);
    std::printf("%c", end);
}

static int laws(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    std::vector<char> a(HEX + 2), b(HEX + 2);
    int rc = 0;
    while (rc == 0 && std::fscanf(f, " %385s %385s", a.data(), b.data()) == 2) {
        uint32_t pw[PW], qw[PW];
        if (!hex_point(a.data(), pw) || !hex_point(b.data(), qw)) { rc = 2; break; }
        const Law::Point P = Law::from_abi(pw), Q = Law::from_abi(qw);
        const Law::Point S = Law::add(P, Q), D = Law::dbl(P);
        print_point(S, ' ');
        print_point(D, ' ');
        print_point(Law::add(S, D), '\n');
    }
    std::fclose(f);
    if (rc) std::fprintf(stderr, "bad law input\n");
    return rc;
}

static int combines(const char* path) {
    FILE* f = std::fopen(path, "r");
    if (!f) { std::fprintf(stderr, "cannot open %s\n", path); return 2; }
    size_t n;
    int rc = 0;
    std::vector<char> line(HEX + 2);
    while (rc == 0 && std::fscanf(f, " sums %zu", &n) == 1) {
        const dr::WideMsmPlan p = dr::plan_wide_msm(n, BITS);
        std::vector<Law::Point> sums(p.sets);
        for (size_t s = 0; s < p.sets && rc == 0; s++) {
            uint32_t w[PW];
            if (std::fscanf(f, " %385s", line.data()) != 1 || !hex_point(line.data(), w)) rc = 2;
            else sums[s] = Law::from_abi(w);
        }
        if (rc == 0) print_point(dr::wide_combine<Law>(sums.data(), p.wt, p.groups), '\n');
    }
    std::fclose(f);
    if (rc) std::fprintf(stderr, "bad combine input\n");
    return rc;
}

static int plans() {
    std::printf("from %zu\n", (size_t)dr::BLSG2_PIP_FROM);
    for (size_t n : {(size_t)dr::BLSG2_PIP_FROM, (size_t)1031, (size_t)4103, (size_t)16387}) {
        const dr::WideMsmPlan p = dr::plan_wide_msm(n, BITS);
        std::printf("plan n=%zu c=%d W=%d H=%u groups=%u sets=%zu\n", n, p.c, p.wt.W, p.H, p.groups, (size_t)p.sets);
    }
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 3 && std::strcmp(argv[1], "law") == 0) return laws(argv[2]);
    if (argc == 3 && std::strcmp(argv[1], "combine") == 0) return combines(argv[2]);
    return plans();
}
