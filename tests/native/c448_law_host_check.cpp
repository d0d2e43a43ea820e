// Host build of dot_ring_amd/csrc/c448_law.hip.h for tests/test_curve448_cpu.py.  Input lines, values as hexadecimal integers below
// 2^448, flags 0 / 1, raw limb images as 16 signed decimal integers:
//   add f1 u1 v1 f2 u2 v2   m448_load both, m448_add, m448_store
//   sub f1 u1 v1 f2 u2 v2   ... the second point negated by m448_cneg first
//   dbl f u v               m448_load, m448_dbl, m448_store
//   ell2 u                  m448_ell2, m448_load_fraction, m448_store
//   oncurve u v             m448_on_curve
//   rawadd x1 y1 z1 x2 y2 z2 (limb images)   m448_add on them as they are
//   rawdbl x y z (limb images)               m448_dbl
//   lane P Q control                         law_lane.hpp: the same and the chain of six windows, raw limbs out
// Output: `flag u v` (flag 1 = the identity; u, v 112 hexadecimal digits) for add / sub / dbl; `has_value flag u v` for ell2; `0` / `1`
// for oncurve; `X Y Z` (canonical, 112 digits each) for the raw forms.  Built with -fsanitize=undefined -fno-sanitize-recover, a signed
// overflow of a 64-bit column (or of a 32-bit limb) aborts the program: that is how the limb classes annotated in the header are
// checked without a GPU.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "c448_law.hip.h"
#include "law_lane.hpp"

struct LaneLaw : dr::M448Law {
    static dr::M448Point cneg(const dr::M448Point& p, bool negate) { return dr::m448_cneg(p, negate); }
};

static bool read_hex(std::istringstream& in, dr::F448& a) {
    std::string s;
    if (!(in >> s) || s.empty() || s.size() > 112) return false;
    uint32_t w[dr::W448] = {0};
    int bit = 0;
    for (size_t i = s.size(); i-- > 0; bit += 4) {
        const char c = s[i];
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (v < 0) return false;
        w[bit >> 5] |= (uint32_t)v << (bit & 31);
    }
    a = dr::unpack(w);
    return true;
}
static bool read_limbs(std::istringstream& in, dr::F448& a) {
    for (int i = 0; i < dr::L448; i++) {
        long long v;
        if (!(in >> v)) return false;
        a.l[i] = (int32_t)v;
    }
    return true;
}
static bool read_point(std::istringstream& in, dr::M448Point& p) {
    int flag;
    dr::F448 u, v;
    if (!(in >> flag) || !read_hex(in, u) || !read_hex(in, v)) return false;
    p = dr::m448_load(u, v, flag != 0);
    return true;
}
static void print_fe(const dr::F448& a) {
    uint32_t w[dr::W448];
    dr::pack(a, w);
    for (int j = dr::W448 - 1; j >= 0; j--) std::printf("%08x", w[j]);
}
static void print_stored(const dr::M448Point& p) {
    dr::F448 u, v;
    const bool ident = dr::m448_store(p, u, v);
    std::printf("%d ", ident ? 1 : 0);
    print_fe(u);
    std::printf(" ");
    print_fe(v);
}
static void print_projective(const dr::M448Point& p) {
    print_fe(p.x);
    std::printf(" ");
    print_fe(p.y);
    std::printf(" ");
    print_fe(p.z);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string op;
        in >> op;
        dr::M448Point p, q;
        if (op == "add" || op == "sub") {
            if (!read_point(in, p) || !read_point(in, q)) return 2;
            print_stored(dr::m448_add(p, dr::m448_cneg(q, op == "sub")));
        } else if (op == "dbl") {
            if (!read_point(in, p)) return 2;
            print_stored(dr::m448_dbl(p));
        } else if (op == "ell2") {
            dr::F448 u, N, D, v;
            bool has_value;
            if (!read_hex(in, u)) return 2;
            dr::m448_ell2(u, N, D, v, has_value);
            std::printf("%d ", has_value ? 1 : 0);
            print_stored(dr::m448_load_fraction(N, D, v));
        } else if (op == "oncurve") {
            dr::F448 u, v;
            if (!read_hex(in, u) || !read_hex(in, v)) return 2;
            std::printf("%d", dr::m448_on_curve(u, v) ? 1 : 0);
        } else if (op == "rawadd") {
            if (!read_limbs(in, p.x) || !read_limbs(in, p.y) || !read_limbs(in, p.z) || !read_limbs(in, q.x) || !read_limbs(in, q.y) ||
                !read_limbs(in, q.z))
                return 2;
            print_projective(dr::m448_add(p, q));
        } else if (op == "rawdbl") {
            if (!read_limbs(in, p.x) || !read_limbs(in, p.y) || !read_limbs(in, p.z)) return 2;
            print_projective(dr::m448_dbl(p));
        } else if (op == "lane") {
            if (!law_lane<LaneLaw>(in)) return 2;
        } else {
            return 3;
        }
        std::printf("\n");
    }
    return 0;
}
