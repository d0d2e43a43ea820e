// Host build of dot_ring_amd/csrc/fp384.hip.h, p384_law.hip.h and sswu.hip.h's sswu_map for tests/test_p384_cpu.py.  Input lines,
// values as hexadecimal integers below 2^384, raw limb images as 14 signed decimal integers (an image stands for its value times
// 2^-392 mod p: the field is in Montgomery form):
//   field A B (limb images)     mul(a, b), sqr(a), a + b, a - b, -a, carry(a), 4 a, -(2^28 - 1) a, inv(a), f384_inv_chain(carry(a)),
//                               the root of carry(a), pack(a), sqr(carry(a)), mul2(carry(a), b, a, carry(b)) = 2 a b — fourteen canonical values
//                               — then the flags: a is a square, the canonical a is odd, a is zero, a = b, cneg(a, 1) = -a, select picks
//   mul2 A B C D (limb images)  mul2(a, b, c, d) = a b + c d
//   add x1 y1 x2 y2             p384_add of the two affine points (0 0 is the identity), stored affine
//   sub x1 y1 x2 y2             ... the second point negated by p384_cneg first
//   dbl x y                     p384_dbl
//   map u                       sswu_map<P384Sswu> and sswu_iso_map, stored affine
//   recode k                    the 96 digits of wave_recode<12>, least significant first, then the carry out of the top one
//   words v                     unpack then pack (the canonical value of any 12 words), then below_p
//   lane P Q control            law_lane.hpp: rawadd, rawdbl, both cneg and the chain of six windows on raw limb images, raw limbs out
// Output: canonical values as 96 hexadecimal digits; points as `x y` (the identity as zeros); flags 0 / 1; digits as decimal integers.
// Built with -fsanitize=undefined -fno-sanitize-recover, a signed overflow of a 64-bit column (or of a 32-bit limb) aborts the program:
// that is how the contract of the field and the limb classes annotated in the law are checked without a GPU.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "p384_law.hip.h"
#include "sswu.hip.h"
#include "wave_recode.hip.h"

#include "law_lane.hpp"

struct LaneLaw : dr::P384Law {
    static dr::P384Point cneg(const dr::P384Point& p, bool negate) { return dr::p384_cneg(p, negate); }
};

static bool read_words(std::istringstream& in, uint32_t (&w)[dr::W384]) {
    std::string s;
    if (!(in >> s) || s.empty() || s.size() > 96) return false;
    for (int j = 0; j < dr::W384; j++) w[j] = 0;
    int bit = 0;
    for (size_t i = s.size(); i-- > 0; bit += 4) {
        const char c = s[i];
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (v < 0) return false;
        w[bit >> 5] |= (uint32_t)v << (bit & 31);
    }
    return true;
}
static bool read_hex(std::istringstream& in, dr::F384& a) {
    uint32_t w[dr::W384];
    if (!read_words(in, w)) return false;
    a = dr::unpack(w);
    return true;
}
static bool read_limbs(std::istringstream& in, dr::F384& a) {
    for (int i = 0; i < dr::L384; i++) {
        long long v;
        if (!(in >> v)) return false;
        a.l[i] = (int32_t)v;
    }
    return true;
}
static bool read_point(std::istringstream& in, dr::P384Point& p) {
    dr::F384 x, y;
    if (!read_hex(in, x) || !read_hex(in, y)) return false;
    p = dr::is_zero(x) && dr::is_zero(y) ? dr::p384_identity() : dr::p384_from_affine(x, y);
    return true;
}
static void print_fe(const dr::F384& a) {
    uint32_t w[dr::W384];
    dr::pack(a, w);
    for (int j = dr::W384 - 1; j >= 0; j--) std::printf("%08x", w[j]);
}
static void print_affine(const dr::P384Point& p) {
    const dr::F384 zi = dr::inv(p.z);
    print_fe(dr::mul(p.x, zi));
    std::printf(" ");
    print_fe(dr::mul(p.y, zi));
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string op;
        in >> op;
        dr::P384Point p, q;
        if (op == "field") {
            dr::F384 a, b, root;
            if (!read_limbs(in, a) || !read_limbs(in, b)) return 2;
            const dr::F384 ca = dr::carry(a);
            const bool sq = dr::f384_sqrt(ca, root);
            const dr::F384 vals[14] = {dr::mul(a, b), dr::sqr(a), dr::add(a, b), dr::sub(a, b), dr::neg(a), ca, dr::mul_small(a, 4),
                                       dr::mul_small(a, -dr::M384), dr::inv(a), dr::f384_inv_chain(ca), root, a, dr::sqr(ca),
                                       dr::mul2(ca, b, a, dr::carry(b))};
            for (const dr::F384& v : vals) {
                print_fe(v);
                std::printf(" ");
            }
            const bool sel = dr::equal(dr::select(true, a, b), a) && dr::equal(dr::select(false, a, b), b);
            std::printf("%d %d %d %d %d %d", sq, dr::is_odd(a), dr::is_zero(a), dr::equal(a, b), dr::equal(dr::cneg(a, true), dr::neg(a)), sel);
        } else if (op == "mul2") {
            dr::F384 a, b, c, d;
            if (!read_limbs(in, a) || !read_limbs(in, b) || !read_limbs(in, c) || !read_limbs(in, d)) return 2;
            print_fe(dr::mul2(a, b, c, d));
        } else if (op == "add" || op == "sub") {
            if (!read_point(in, p) || !read_point(in, q)) return 2;
            print_affine(dr::p384_add(p, dr::p384_cneg(q, op == "sub")));
        } else if (op == "dbl") {
            if (!read_point(in, p)) return 2;
            print_affine(dr::p384_dbl(p));
        } else if (op == "map") {
            uint32_t w[dr::W384];
            if (!read_words(in, w)) return 2;
            dr::F384 xn, xd, y;
            dr::sswu_map<dr::P384Sswu>(dr::unpack(w), (w[0] & 1u) != 0, xn, xd, y);
            bool ok;
            print_affine(dr::sswu_iso_map<dr::P384Sswu>(xn, xd, y, ok));
        } else if (op == "recode") {
            uint32_t k[dr::W384], dig[dr::W384];
            if (!read_words(in, k)) return 2;
            const uint32_t top = dr::wave_recode(k, dig);
            for (int w = 0; w < 8 * dr::W384; w++) std::printf("%d ", dr::wave_digit(dig, w));
            std::printf("%u", top);
        } else if (op == "words") {
            uint32_t w[dr::W384];
            if (!read_words(in, w)) return 2;
            print_fe(dr::unpack(w));
            std::printf(" %d", dr::below_p(w) ? 1 : 0);
        } else if (op == "lane") {
            if (!law_lane<LaneLaw>(in)) return 2;
        } else {
            return 3;
        }
        std::printf("\n");
    }
    return 0;
}
