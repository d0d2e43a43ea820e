// The host's law of the bucket method on BLS12-381's E(Fq2): y^2 = x^3 + 4 (1 + i) (dr_blsg2_msm): what wide_combine.hpp asks of a Law —
// Point, identity / add / dbl, from_abi / to_abi over the ABI's canonical words — for the set sums that wave_msm_fold_affine stores as
// affine points, the sibling of narrow_law.hpp's laws over hostpairing.hpp's drh::Fq2.  The addition is the complete projective one of
// Renes, Costello and Batina (2016, algorithm 7) for a = 0 with b3 = 3 b = 12 (1 + i), the law kernels_g2_h2c.hip.h runs on the device:
// equal points, inverse pairs and the identity (0 : 1 : 0) are operands like any other, and nothing in it depends on the point lying in
// G2.  There is no doubling of its own: a combine is ~256 doublings and a few hundred additions.  192 zero bytes are the identity, in and
// out (Z = 0 gives x = y = 0 through 0^-1 = 0).  Plain host C++: g++ builds it for tests/native/g2_msm_host_check.cpp.
#pragma once
#include <cstdint>
#include <cstring>

#include "hostpairing.hpp"

namespace dr {

struct G2hLaw {
    static constexpr int WORDS = 24;
    using E = drh::Fq2;
    struct Point { E x, y, z; };
    static E mul_b3(const E& a) {                                      // 12 (1 + i) a
        const E x = a.mul_xi(), x2 = x + x, x4 = x2 + x2;
        return x4 + x4 + x4;
    }
    static Point identity() { return Point{E::zero(), E::one(), E::zero()}; }
    static Point add(const Point& p, const Point& q) {
        const E t0 = p.x * q.x, t1 = p.y * q.y, t2 = p.z * q.z;
        const E xy = (p.x + p.y) * (q.x + q.y) - (t0 + t1);            // X1 Y2 + X2 Y1
        const E yz = (p.y + p.z) * (q.y + q.z) - (t1 + t2);            // Y1 Z2 + Y2 Z1
        const E xz = (p.x + p.z) * (q.x + q.z) - (t0 + t2);            // X1 Z2 + X2 Z1
        const E y3 = mul_b3(xz), x3 = t0 + t0 + t0, bz = mul_b3(t2);
        const E zp = t1 + bz, xm = t1 - bz;
        return Point{xy * xm - yz * y3, xm * zp + y3 * x3, zp * yz + x3 * xy};
    }
    static Point dbl(const Point& p) { return add(p, p); }
    // (the callers have checked that coordinates are canonical)
    static Point from_abi(const uint32_t* w) {
        uint8_t b[192];
        std::memcpy(b, w, 192);
        bool zero = true;
        for (int i = 0; i < 192; i++) zero = zero && b[i] == 0;
        if (zero) return identity();
        Point r;
        (void)drh::Fq::load_le(r.x.c0, b);
        (void)drh::Fq::load_le(r.x.c1, b + 48);
        (void)drh::Fq::load_le(r.y.c0, b + 96);
        (void)drh::Fq::load_le(r.y.c1, b + 144);
        r.z = E::one();
        return r;
    }
    static void to_abi(const Point& p, uint32_t* w) {
        const E zi = p.z.inv(), x = p.x * zi, y = p.y * zi;
        uint8_t b[192];
        x.c0.store_le(b);
        x.c1.store_le(b + 48);
        y.c0.store_le(b + 96);
        y.c1.store_le(b + 144);
        std::memcpy(w, b, 192);
    }
};

}  // namespace dr
