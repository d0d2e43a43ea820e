// Host check of dot_ring_amd/csrc/verify_tree.hpp: the descent with a stub predicate.  One case per input line: `B k b_1 ... b_k` (B leaves,
// the k bad ones).  A node passes iff no bad leaf lies under it.  Prints per case: the number of nodes tested, how many of them had
// only padding under them, how many were asked although no bad leaf lies under their parent (a parent that holds), the
// largest request handed to the predicate at once, and the verdicts as a string of 0 / 1.
// Built with -fsanitize=undefined -fno-sanitize-recover: a shift or an index out of range ends the program.
#include <algorithm>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "verify_tree.hpp"

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        size_t B = 0, k = 0;
        if (!(in >> B >> k)) continue;
        std::vector<uint8_t> bad(B, 0);
        for (size_t j = 0; j < k; j++) { size_t b; in >> b; if (b < B) bad[b] = 1; }
        const drh::VerifyTreeShape sh(B);
        size_t padding_tested = 0, orphan = 0, widest = 0;
        auto test = [&](const std::vector<size_t>& ask, std::vector<uint8_t>& pass) {
            widest = std::max(widest, ask.size());
            for (size_t j = 0; j < ask.size(); j++) {
                size_t lo, count;
                sh.span(ask[j], lo, count);
                if (lo >= B) padding_tested++;
                bool ok = true;
                for (size_t i = lo; i < lo + count && i < B; i++) if (bad[i]) ok = false;
                pass[j] = ok ? 1 : 0;
                if (ask[j] != 0) {
                    size_t parent = (ask[j] - 1) / 2;
                    bool parent_failed = false;
                    size_t plo, pcount;
                    sh.span(parent, plo, pcount);
                    for (size_t i = plo; i < plo + pcount && i < B; i++) if (bad[i]) parent_failed = true;
                    if (!parent_failed) orphan++;
                }
            }
        };
        std::vector<uint8_t> verdicts(B ? B : 1, 2);
        const size_t tested = drh::verify_tree_descend(sh, test, verdicts.data());
        std::string bits;
        for (size_t i = 0; i < B; i++) bits += verdicts[i] == 1 ? '1' : verdicts[i] == 0 ? '0' : '?';
        std::printf("%zu %zu %zu %zu %zu %zu %s\n", tested, padding_tested, orphan, widest, sh.padded, sh.depth, bits.c_str());
    }
    return 0;
}
