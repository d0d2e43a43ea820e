// The host's end of the wide suites' bucket method (dr_wide_msm; wave_msm.hip.h): the W x G set sums that leave the device as records of
// limb images become points of the suite's own law (P384Law, P521Law, E448Law, M448Law: p384_law.hip.h, p521_law.hip.h, e448_law.hip.h,
// c448_law.hip.h, which compile for the host), and index groups and windows are combined from the top window down — doublings by the
// width of each window, then the additions of its groups.  A chain of ~bits doublings: one CPU core, not one GPU lane.
// The suites whose set sums leave as affine ABI points (the 256-bit curves and E(Fq): narrow_law.hpp) use wide_combine alone, over laws
// of the same shape.
// Plain host C++ over those headers: g++ builds it for tests/native/wide_msm_plan_check.cpp and tests/native/narrow_msm_host_check.cpp.
#pragma once
#include <cstddef>
#include <cstdint>

#include "wide_recode.hip.h"

namespace dr {

// words of a record: x, y, z limb images, padded to whole uint4 (wave_msm_record_words)
template <class Law>
constexpr int wide_record_words() { return (3 * Law::LIMBS + 3) & ~3; }

template <class Law>
typename Law::Point wide_record_point(const uint32_t* rec) {
    typename Law::Point p;
    for (int i = 0; i < Law::LIMBS; i++) {
        p.x.l[i] = (int32_t)rec[i];
        p.y.l[i] = (int32_t)rec[Law::LIMBS + i];
        p.z.l[i] = (int32_t)rec[2 * Law::LIMBS + i];
    }
    return p;
}

// sums[w * groups + g]: the value of bucket set (window w, index group g)
template <class Law>
typename Law::Point wide_combine(const typename Law::Point* sums, const WideTiling& wt, uint32_t groups) {
    typename Law::Point acc = Law::identity();
    for (int w = wt.W - 1; w >= 0; w--) {
        if (w != wt.W - 1)
            for (int j = 0; j < wide_width(wt, w); j++) acc = Law::dbl(acc);
        for (uint32_t g = 0; g < groups; g++) acc = Law::add(acc, sums[(size_t)w * groups + g]);
    }
    return acc;
}

}  // namespace dr
