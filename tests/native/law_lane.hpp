// The `lane` line of the host builds of the group laws (p384_host_check.cpp, p521_host_check.cpp, c448_law_host_check.cpp,
// e448_law_host_check.cpp): what dot_ring_amd/csrc/wave_curve.hip.h's wave_law_selftest runs on the device, without the LDS table, on
// RAW limb images in and out, for tests/law_images.py's lanes and checker.
//   lane P Q control     P and Q as x, y, z of LIMBS signed decimal integers each, the control word as a decimal integer
// answers the raw limbs (x, y, z) of eleven points on one line:  add(P, Q)  (rawadd),  add(P, cneg(Q, true)),  dbl(P)  (rawdbl),
// cneg(P, true),  cneg(P, false),  and the accumulator after each of the six windows of the fixed schedule started at acc = P (the
// chain): four doublings, then the table term add(P, Q) added, negated when bit w of the control word is set and replaced by the
// identity when bit 8 + w is.  Under -fsanitize=undefined -fno-sanitize-recover a signed column overflow anywhere in a law at the edge of
// its contract aborts there.
// LAW gives Point (members x, y, z with limbs l[]), LIMBS, identity(), add, dbl and cneg.
#pragma once
#include <cstdio>
#include <sstream>

template <class LAW>
bool law_lane_read_point(std::istringstream& in, typename LAW::Point& p) {
    auto read = [&](auto& fe) {
        for (int i = 0; i < LAW::LIMBS; i++) {
            long long v;
            if (!(in >> v)) return false;
            fe.l[i] = (int32_t)v;
        }
        return true;
    };
    return read(p.x) && read(p.y) && read(p.z);
}
template <class LAW>
void law_lane_print(const typename LAW::Point& p, bool last = false) {
    for (int i = 0; i < LAW::LIMBS; i++) std::printf("%d ", p.x.l[i]);
    for (int i = 0; i < LAW::LIMBS; i++) std::printf("%d ", p.y.l[i]);
    for (int i = 0; i < LAW::LIMBS; i++) std::printf(i + 1 == LAW::LIMBS && last ? "%d" : "%d ", p.z.l[i]);
}
// false if the line does not parse
template <class LAW>
bool law_lane(std::istringstream& in) {
    typename LAW::Point P, Q;
    unsigned long control;
    if (!law_lane_read_point<LAW>(in, P) || !law_lane_read_point<LAW>(in, Q) || !(in >> control)) return false;
    const typename LAW::Point table = LAW::add(P, Q);
    law_lane_print<LAW>(table);
    law_lane_print<LAW>(LAW::add(P, LAW::cneg(Q, true)));
    law_lane_print<LAW>(LAW::dbl(P));
    law_lane_print<LAW>(LAW::cneg(P, true));
    law_lane_print<LAW>(LAW::cneg(P, false));
    typename LAW::Point acc = P;
    for (int w = 0; w < 6; w++) {
        for (int j = 0; j < 4; j++) acc = LAW::dbl(acc);
        typename LAW::Point T = LAW::cneg(table, ((control >> w) & 1u) != 0);
        if (((control >> (8 + w)) & 1u) != 0) T = LAW::identity();
        acc = LAW::add(acc, T);
        law_lane_print<LAW>(acc, w == 5);
    }
    return true;
}
