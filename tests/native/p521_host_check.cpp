// Host build of dot_ring_amd/csrc/fp521.hip.h, p521_law.hip.h and sswu.hip.h's sswu_map for tests/test_p521_cpu.py.  Input lines,
// values as hexadecimal integers below 2^544, raw limb images as 19 signed decimal integers:
//   field A B (limb images)     mul(a, b), sqr(a), a + b, a - b, -a, carry(a), 4 a, -(2^28 - 1) a, inv(a), f521_inv_chain(carry(a)),
//                               the root of carry(a), pack(a) — twelve canonical values — then the flags: a is a square, the canonical a
//                               is odd, a is zero, a = b, cneg(a, 1) = -a, select picks
//   add x1 y1 x2 y2             p521_add of the two affine points (0 0 is the identity), stored affine
//   sub x1 y1 x2 y2             ... the second point negated by p521_cneg first
//   dbl x y                     p521_dbl
//   map u                       sswu_map<P521Sswu> and sswu_iso_map, stored affine
//   recode k                    the 131 digits of wave_recode<17>, least significant first, then the nibbles above them (all 0)
//   words v                     unpack then pack (the canonical value of any 17 words below 2^532), then below_p
//   lane P Q control            law_lane.hpp: rawadd, rawdbl, both cneg and the chain of six windows on raw limb images, raw limbs out
// Output: canonical values as 136 hexadecimal digits; points as `x y` (the identity as zeros); flags 0 / 1; digits as decimal integers.
// Built with -fsanitize=undefined -fno-sanitize-recover, a signed overflow of a 64-bit column (or of a 32-bit limb) aborts the program:
// that is how the contract of the field and the limb classes annotated in the law are checked without a GPU.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "p521_law.hip.h"
#include "sswu.hip.h"
#include "wave_recode.hip.h"

#include "law_lane.hpp"

struct LaneLaw : dr::P521Law {
    static dr::P521Point cneg(const dr::P521Point& p, bool negate) { return dr::p521_cneg(p, negate); }
};

static bool read_words(std::istringstream& in, uint32_t (&w)[dr::W521]) {
    std::string s;
    if (!(in >> s) || s.empty() || s.size() > 136) return false;
    for (int j = 0; j < dr::W521; j++) w[j] = 0;
    int bit = 0;
    for (size_t i = s.size(); i-- > 0; bit += 4) {
        const char c = s[i];
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (v < 0) return false;
        w[bit >> 5] |= (uint32_t)v << (bit & 31);
    }
    return true;
}
static bool read_hex(std::istringstream& in, dr::F521& a) {
    uint32_t w[dr::W521];
    if (!read_words(in, w)) return false;
    a = dr::unpack(w);
    return true;
}
static bool read_limbs(std::istringstream& in, dr::F521& a) {
    for (int i = 0; i < dr::L521; i++) {
        long long v;
        if (!(in >> v)) return false;
        a.l[i] = (int32_t)v;
    }
    return true;
}
static bool read_point(std::istringstream& in, dr::P521Point& p) {
    dr::F521 x, y;
    if (!read_hex(in, x) || !read_hex(in, y)) return false;
    p = dr::is_zero(x) && dr::is_zero(y) ? dr::p521_identity() : dr::p521_from_affine(x, y);
    return true;
}
static void print_fe(const dr::F521& a) {
    uint32_t w[dr::W521];
    dr::pack(a, w);
    for (int j = dr::W521 - 1; j >= 0; j--) std::printf("%08x", w[j]);
}
static void print_affine(const dr::P521Point& p) {
    const dr::F521 zi = dr::inv(p.z);
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
        dr::P521Point p, q;
        if (op == "field") {
            dr::F521 a, b, root;
            if (!read_limbs(in, a) || !read_limbs(in, b)) return 2;
            const dr::F521 ca = dr::carry(a);
            const bool sq = dr::f521_sqrt(ca, root);
            const dr::F521 vals[12] = {dr::mul(a, b), dr::sqr(a), dr::add(a, b), dr::sub(a, b), dr::neg(a), ca, dr::mul_small(a, 4),
                                       dr::mul_small(a, -dr::M521), dr::inv(a), dr::f521_inv_chain(ca), root, a};
            for (const dr::F521& v : vals) {
                print_fe(v);
                std::printf(" ");
            }
            const bool sel = dr::equal(dr::select(true, a, b), a) && dr::equal(dr::select(false, a, b), b);
            std::printf("%d %d %d %d %d %d", sq, dr::is_odd(a), dr::is_zero(a), dr::equal(a, b), dr::equal(dr::cneg(a, true), dr::neg(a)), sel);
        } else if (op == "add" || op == "sub") {
            if (!read_point(in, p) || !read_point(in, q)) return 2;
            print_affine(dr::p521_add(p, dr::p521_cneg(q, op == "sub")));
        } else if (op == "dbl") {
            if (!read_point(in, p)) return 2;
            print_affine(dr::p521_dbl(p));
        } else if (op == "map") {
            uint32_t w[dr::W521];
            if (!read_words(in, w)) return 2;
            dr::F521 xn, xd, y;
            dr::sswu_map<dr::P521Sswu>(dr::unpack(w), (w[0] & 1u) != 0, xn, xd, y);
            bool ok;
            print_affine(dr::sswu_iso_map<dr::P521Sswu>(xn, xd, y, ok));
        } else if (op == "recode") {
            uint32_t k[dr::W521], dig[dr::W521];
            if (!read_words(in, k)) return 2;
            dr::wave_recode(k, dig);
            for (int w = 0; w < 8 * dr::W521; w++) std::printf("%d ", dr::wave_digit(dig, w));
        } else if (op == "words") {
            uint32_t w[dr::W521];
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
