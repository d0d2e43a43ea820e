// Host build of a signed 28-bit field, dot_ring_amd/csrc/sw3_law.hip.h over it and sswu.hip.h's sswu_map, once for
// p384_host_check.cpp (tests/test_p384_cpu.py) and p521_host_check.cpp (tests/test_p521_cpu.py); each includes its curve's law header,
// then this, and gives a description T of what differs:
//   D, Sswu                     the curve's descriptions for sw3_law.hip.h and sswu.hip.h
//   WINDOWS, M                  the windows of the fixed schedule and the largest normal limb
//   sqrt(a, r), inv_chain(a)    the field's root and its inversion by the addition chain
// Input lines, values as hexadecimal integers of up to 8 digits a word, raw limb images as LIMBS signed decimal integers:
//   field A B (limb images)     mul(a, b), sqr(a), a + b, a - b, -a, carry(a), 4 a, -(2^28 - 1) a, inv(a), inv_chain(carry(a)),
//                               the root of carry(a), pack(a) — twelve canonical values — and where the field has mul2 (D::FUSED)
//                               sqr(carry(a)) and mul2(carry(a), b, a, carry(b)) = 2 a b as well; then the flags: a is a square, the
//                               canonical a is odd, a is zero, a = b, cneg(a, 1) = -a, select picks
//   mul2 A B C D (limb images)  mul2(a, b, c, d) = a b + c d (D::FUSED only)
//   add x1 y1 x2 y2             the sum of the two affine points (0 0 is the identity), stored affine
//   sub x1 y1 x2 y2             ... the second point negated by the law's cneg first
//   dbl x y                     the double
//   map u                       sswu_map<Sswu> and sswu_iso_map, stored affine
//   recode k                    the 8 WORDS digits of wave_recode, least significant first; then, where the schedule has a window for
//                               it (WINDOWS > 8 WORDS), the carry out of the top one
//   words v                     unpack then pack (the canonical value of any WORDS words the field unpacks), then below_p
//   lane P Q control            law_lane.hpp: rawadd, rawdbl, both cneg and the chain of six windows on raw limb images, raw limbs out
// Output: canonical values as 8 WORDS hexadecimal digits; points as `x y` (the identity as zeros); flags 0 / 1; digits as decimal
// integers.  Built with -fsanitize=undefined -fno-sanitize-recover, a signed overflow of a 64-bit column (or of a 32-bit limb) aborts
// the program: that is how the contract of the field and the limb classes annotated in the law are checked without a GPU.
#pragma once
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "sswu.hip.h"
#include "wave_recode.hip.h"

#include "law_lane.hpp"

template <class T>
struct Sw3HostCheck {
    using Law = dr::Sw3Law<typename T::D>;
    using Fe = typename Law::Fe;
    using Point = typename Law::Point;
    static constexpr int W = Law::WORDS, L = Law::LIMBS;

    static bool read_words(std::istringstream& in, uint32_t (&w)[W]) {
        std::string s;
        if (!(in >> s) || s.empty() || s.size() > (size_t)(8 * W)) return false;
        for (int j = 0; j < W; j++) w[j] = 0;
        int bit = 0;
        for (size_t i = s.size(); i-- > 0; bit += 4) {
            const char c = s[i];
            const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
            if (v < 0) return false;
            w[bit >> 5] |= (uint32_t)v << (bit & 31);
        }
        return true;
    }
    static bool read_hex(std::istringstream& in, Fe& a) {
        uint32_t w[W];
        if (!read_words(in, w)) return false;
        a = dr::unpack(w);
        return true;
    }
    static bool read_limbs(std::istringstream& in, Fe& a) {
        for (int i = 0; i < L; i++) {
            long long v;
            if (!(in >> v)) return false;
            a.l[i] = (int32_t)v;
        }
        return true;
    }
    static bool read_point(std::istringstream& in, Point& p) {
        Fe x, y;
        if (!read_hex(in, x) || !read_hex(in, y)) return false;
        p = dr::is_zero(x) && dr::is_zero(y) ? Law::identity() : Law::from_affine(x, y);
        return true;
    }
    static void print_fe(const Fe& a) {
        uint32_t w[W];
        dr::pack(a, w);
        for (int j = W - 1; j >= 0; j--) std::printf("%08x", w[j]);
    }
    static void print_affine(const Point& p) {
        const Fe zi = dr::inv(p.z);
        print_fe(dr::mul(p.x, zi));
        std::printf(" ");
        print_fe(dr::mul(p.y, zi));
    }

    static int main() {
        std::string line;
        while (std::getline(std::cin, line)) {
            if (line.empty()) continue;
            std::istringstream in(line);
            std::string op;
            in >> op;
            Point p, q;
            if (op == "field") {
                Fe a, b, root;
                if (!read_limbs(in, a) || !read_limbs(in, b)) return 2;
                const Fe ca = dr::carry(a);
                const bool sq = T::sqrt(ca, root);
                std::vector<Fe> vals = {dr::mul(a, b), dr::sqr(a), dr::add(a, b), dr::sub(a, b), dr::neg(a), ca, dr::mul_small(a, 4),
                                        dr::mul_small(a, -T::M), dr::inv(a), T::inv_chain(ca), root, a};
                if constexpr (T::D::FUSED) {
                    vals.push_back(dr::sqr(ca));
                    vals.push_back(dr::mul2(ca, b, a, dr::carry(b)));
                }
                for (const Fe& v : vals) {
                    print_fe(v);
                    std::printf(" ");
                }
                const bool sel = dr::equal(dr::select(true, a, b), a) && dr::equal(dr::select(false, a, b), b);
                std::printf("%d %d %d %d %d %d", sq, dr::is_odd(a), dr::is_zero(a), dr::equal(a, b), dr::equal(dr::cneg(a, true), dr::neg(a)), sel);
            } else if (T::D::FUSED && op == "mul2") {
                if constexpr (T::D::FUSED) {
                    Fe a, b, c, d;
                    if (!read_limbs(in, a) || !read_limbs(in, b) || !read_limbs(in, c) || !read_limbs(in, d)) return 2;
                    print_fe(dr::mul2(a, b, c, d));
                }
            } else if (op == "add" || op == "sub") {
                if (!read_point(in, p) || !read_point(in, q)) return 2;
                print_affine(Law::add(p, Law::cneg(q, op == "sub")));
            } else if (op == "dbl") {
                if (!read_point(in, p)) return 2;
                print_affine(Law::dbl(p));
            } else if (op == "map") {
                uint32_t w[W];
                if (!read_words(in, w)) return 2;
                Fe xn, xd, y;
                dr::sswu_map<typename T::Sswu>(dr::unpack(w), (w[0] & 1u) != 0, xn, xd, y);
                bool ok;
                print_affine(dr::sswu_iso_map<typename T::Sswu>(xn, xd, y, ok));
            } else if (op == "recode") {
                uint32_t k[W], dig[W];
                if (!read_words(in, k)) return 2;
                const uint32_t top = dr::wave_recode(k, dig);
                for (int w = 0; w < 8 * W; w++) std::printf("%d ", dr::wave_digit(dig, w));
                if (T::WINDOWS > 8 * W) std::printf("%u", top);
            } else if (op == "words") {
                uint32_t w[W];
                if (!read_words(in, w)) return 2;
                print_fe(dr::unpack(w));
                std::printf(" %d", dr::below_p(w) ? 1 : 0);
            } else if (op == "lane") {
                if (!law_lane<Law>(in)) return 2;
            } else {
                return 3;
            }
            std::printf("\n");
        }
        return 0;
    }
};
