// Host build of dot_ring_amd/csrc/fp384.hip.h, sw3_law.hip.h over it (p384_law.hip.h) and sswu.hip.h's sswu_map for
// tests/test_p384_cpu.py: sw3_host_check.hpp's program, which lists the input lines.  Values are hexadecimal integers below 2^384 and
// print as 96 digits; a raw limb image is 14 signed decimal integers and stands for its value times 2^-392 mod p (the field is in
// Montgomery form).  The field has mul2, so the `field` line answers fourteen values and there is a `mul2` line; `recode` answers 96
// digits and the carry out of the top one (window 96).
#include "p384_law.hip.h"

#include "sw3_host_check.hpp"

struct P384Check {
    using D = dr::P384Sw3;
    using Sswu = dr::P384Sswu;
    static constexpr int WINDOWS = dr::P384_WINDOWS;
    static constexpr int32_t M = dr::M384;
    static bool sqrt(const dr::F384& a, dr::F384& r) { return dr::f384_sqrt(a, r); }
    static dr::F384 inv_chain(const dr::F384& a) { return dr::f384_inv_chain(a); }
};

int main() { return Sw3HostCheck<P384Check>::main(); }
