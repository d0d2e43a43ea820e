// Host build of dot_ring_amd/csrc/e448_law.hip.h for tests/test_law_images_cpu.py.  Input lines:
//   lane P Q control     law_lane.hpp: e448_add, e448_dbl, e448_cneg and the chain of six windows on RAW limb images (x, y, z of 16
//                        signed decimal integers each), raw limbs out
// Built with -fsanitize=undefined -fno-sanitize-recover, a signed overflow of a 64-bit column (or of a 32-bit limb) aborts the program:
// that is how the limb classes annotated in the header are checked without a GPU.
#include <iostream>
#include <sstream>
#include <string>

#include "e448_law.hip.h"
#include "law_lane.hpp"

struct LaneLaw : dr::E448Law {
    static dr::E448Point cneg(const dr::E448Point& p, bool negate) { return dr::e448_cneg(p, negate); }
};

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string op;
        in >> op;
        if (op != "lane") return 3;
        if (!law_lane<LaneLaw>(in)) return 2;
        std::printf("\n");
    }
    return 0;
}
