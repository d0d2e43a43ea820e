// Host build of dot_ring_amd/csrc/wave_recode.hip.h for tests/test_wave_recode_cpu.py.  Input lines: `KW k`, KW in {8, 14, 17} and k a
// hexadecimal integer below 2^(32 KW).  Output per line: the 8 KW digits of wave_recode<KW>, least significant first, as decimal
// integers, then the carry out of the top nibble.  Built with -fsanitize=undefined -fno-sanitize-recover: a shift or an index out of
// range aborts the program.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "wave_recode.hip.h"

template <int KW>
static bool recode_line(const std::string& s) {
    if (s.empty() || s.size() > 8 * KW) return false;
    uint32_t k[KW] = {}, dig[KW];
    int bit = 0;
    for (size_t i = s.size(); i-- > 0; bit += 4) {
        const char c = s[i];
        const int v = c >= '0' && c <= '9' ? c - '0' : c >= 'a' && c <= 'f' ? c - 'a' + 10 : -1;
        if (v < 0) return false;
        k[bit >> 5] |= (uint32_t)v << (bit & 31);
    }
    const uint32_t carry = dr::wave_recode(k, dig);
    for (int w = 0; w < 8 * KW; w++) std::printf("%d ", dr::wave_digit(dig, w));
    std::printf("%u\n", carry);
    return true;
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        int kw;
        std::string s;
        if (!(in >> kw >> s)) return 2;
        const bool ok = kw == 8 ? recode_line<8>(s) : kw == 14 ? recode_line<14>(s) : kw == 17 ? recode_line<17>(s) : false;
        if (!ok) return 2;
    }
    return 0;
}
