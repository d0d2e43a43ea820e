// Host build of dot_ring_amd/csrc/fp521.hip.h, sw3_law.hip.h over it (p521_law.hip.h) and sswu.hip.h's sswu_map for
// tests/test_p521_cpu.py: sw3_host_check.hpp's program, which lists the input lines.  Values are hexadecimal integers below 2^544
// (`words`: below 2^532) and print as 136 digits; a raw limb image is 19 signed decimal integers.  The field has no mul2, so the `field`
// line answers twelve values and there is no `mul2` line; `recode` answers the 131 digits of the schedule and the nibbles above them
// (all 0), and no carry.
#include "p521_law.hip.h"

#include "sw3_host_check.hpp"

struct P521Check {
    using D = dr::P521Sw3;
    using Sswu = dr::P521Sswu;
    static constexpr int WINDOWS = dr::P521_WINDOWS;
    static constexpr int32_t M = dr::M521;
    static bool sqrt(const dr::F521& a, dr::F521& r) { return dr::f521_sqrt(a, r); }
    static dr::F521 inv_chain(const dr::F521& a) { return dr::f521_inv_chain(a); }
};

int main() { return Sw3HostCheck<P521Check>::main(); }
