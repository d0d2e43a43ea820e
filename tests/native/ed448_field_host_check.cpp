// Host build of dot_ring_amd/csrc/fe448.hip.h for tests/test_ed448_cpu.py.  Each input line is an operation name followed by the raw
// limb images of its operands (16 signed decimal integers each):
//   mul a b | sqr a | carry a | pack a | small39081 a | small156326 a | inv a | sqrt a | p34 a
// and each output line is the canonical value of the result as 112 hexadecimal digits (big-endian), followed for `sqrt` by 1 or 0
// (whether the operand is a square) and for `carry` by the sixteen limbs carry() left.  Built with -fsanitize=undefined
// -fno-sanitize-recover, a signed overflow of a 64-bit column (or of a 32-bit limb) aborts the program: that is how the accumulator
// budget at the head of fe448.hip.h is checked without a GPU.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "fe448.hip.h"

static bool read_fe(std::istringstream& in, dr::F448& a) {
    for (int i = 0; i < dr::L448; i++) {
        long long v;
        if (!(in >> v)) return false;
        a.l[i] = (int32_t)v;
    }
    return true;
}
static void print_fe(const dr::F448& a) {
    uint32_t w[dr::W448];
    dr::pack(a, w);
    for (int j = dr::W448 - 1; j >= 0; j--) std::printf("%08x", w[j]);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string op;
        in >> op;
        dr::F448 a, b;
        if (!read_fe(in, a)) return 2;
        if (op == "mul") {
            if (!read_fe(in, b)) return 2;
            print_fe(dr::mul(a, b));
        } else if (op == "sqr") {
            print_fe(dr::sqr(a));
        } else if (op == "carry") {
            const dr::F448 c = dr::carry(a);
            print_fe(c);
            for (int i = 0; i < dr::L448; i++) std::printf(" %d", c.l[i]);
        } else if (op == "pack") {
            print_fe(a);
        } else if (op == "small39081") {
            print_fe(dr::mul_small(a, 39081));
        } else if (op == "small156326") {
            print_fe(dr::mul_small(a, 156326));
        } else if (op == "inv") {
            print_fe(dr::inv(a));
        } else if (op == "p34") {
            print_fe(dr::f448_pow_p34(a));
        } else if (op == "sqrt") {
            dr::F448 r;
            const bool sq = dr::f448_sqrt(a, r);
            print_fe(r);
            std::printf(" %d", sq ? 1 : 0);
        } else {
            return 3;
        }
        std::printf("\n");
    }
    return 0;
}
