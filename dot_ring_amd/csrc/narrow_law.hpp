// The host's laws of the bucket method on the 256-bit suites and BLS12-381's E(Fq) (dr_te_msm from NARROW_PIP_FROM terms on,
// dr_blsg1_msm): what wide_combine.hpp asks of a Law — Point, identity / add / dbl, from_abi / to_abi over the ABI's canonical words —
// for the set sums that wave_msm_fold_affine stores as affine points.  The 29-bit field headers of these curves do not compile for the
// host, so two small laws run over drh::Mod256 (a runtime 256-bit field, standard form in and out):
//   TeLaw256<K>   the unified extended twisted Edwards addition (add-2008-hwcd) with (a, d): Ed25519 (a = -1) and Baby JubJub (a = 1).
//                 a is a square and d is not on both, so the addition is complete: small-order points are terms like any other.
//   SwLaw256<K>   the complete projective short Weierstrass addition of Renes, Costello and Batina (2016, algorithm 1) with (a, 3 b):
//                 P-256 and secp256k1 (prime order).
// Neither has a doubling of its own: a combine is ~256 doublings and a few hundred additions, microseconds on one core.
// C25519Law is Ed25519's law whose to_abi gives Montgomery u || v by c25519_store's rules (kernels_curve25519.hip.h).  G1hLaw is
// hostmath.hpp's XYZZ law of E(Fq): its branches take equal points, inverse pairs and the identity, and nothing in it depends on the
// point lying in G1.  Plain host C++: g++ builds it for tests/native/narrow_msm_host_check.cpp.
#pragma once
#include <cstdint>
#include <cstring>

#include "hostmath.hpp"
#include "hostproto.hpp"

namespace dr {

// an element of the field K::field(), standard form
template <class K>
struct El256 {
    uint64_t v[4];
    static El256 of(const uint64_t* w) { El256 r; std::memcpy(r.v, w, 32); return r; }
    static El256 small(uint64_t s) { El256 r{{s, 0, 0, 0}}; return r; }
    friend El256 operator+(const El256& a, const El256& b) { El256 r; K::field().add(a.v, b.v, r.v); return r; }
    friend El256 operator-(const El256& a, const El256& b) { El256 r; K::field().sub(a.v, b.v, r.v); return r; }
    friend El256 operator*(const El256& a, const El256& b) { El256 r; K::field().mul(a.v, b.v, r.v); return r; }
    El256 inv() const { El256 r; K::field().inv(v, r.v); return r; }                 // 0 -> 0
    bool is_zero() const { return (v[0] | v[1] | v[2] | v[3]) == 0; }
};

// the fields and constants: a and d of a x^2 + y^2 = 1 + d x^2 y^2; a and 3 b of y^2 = x^3 + a x + b
struct Ed25519K {
    static const drh::Mod256& field() { return drh::mod_p25519(); }
    static El256<Ed25519K> a() { return El256<Ed25519K>::small(0) - El256<Ed25519K>::small(1); }
    static El256<Ed25519K> d() { return El256<Ed25519K>::of(drh::te_curve(3)->d); }
};
struct BjjK {
    static const drh::Mod256& field() { return drh::mod_pbn254(); }
    static El256<BjjK> a() { return El256<BjjK>::small(1); }
    static El256<BjjK> d() { return El256<BjjK>::of(drh::te_curve(5)->d); }
};
struct P256K {
    static const drh::Mod256& field() { return drh::mod_p256(); }
    static El256<P256K> a() { return El256<P256K>::small(0) - El256<P256K>::small(3); }
    static El256<P256K> b3() {     // 3 x 0x5ac635d8aa3a93e7b3ebbd55769886bc651d06b0cc53b0f63bce3c3e27d2604b mod p
        static const uint64_t w[4] = {0xb36ab4ba777720e2ULL, 0x2f57141164fb12e2ULL, 0x1bc3380063c99435ULL, 0x1052a18afeafbbb6ULL};
        return El256<P256K>::of(w);
    }
};
struct Secp256k1K {
    static const drh::Mod256& field() { return drh::mod_psecp256k1(); }
    static El256<Secp256k1K> a() { return El256<Secp256k1K>::small(0); }
    static El256<Secp256k1K> b3() { return El256<Secp256k1K>::small(21); }
};

template <class K>
struct TeLaw256 {
    using E = El256<K>;
    static constexpr int WORDS = 8;
    struct Point { E x, y, z, t; };
    static Point identity() { return Point{E::small(0), E::small(1), E::small(1), E::small(0)}; }
    static Point add(const Point& p, const Point& q) {
        const E A = p.x * q.x, B = p.y * q.y, C = p.t * K::d() * q.t, D = p.z * q.z;
        const E Ee = (p.x + p.y) * (q.x + q.y) - A - B, F = D - C, G = D + C, H = B - K::a() * A;
        return Point{Ee * F, G * H, F * G, Ee * H};
    }
    static Point dbl(const Point& p) { return add(p, p); }
    static Point from_abi(const uint32_t* w) {
        uint64_t v[8];
        std::memcpy(v, w, 64);
        const E x = E::of(v), y = E::of(v + 4);
        return Point{x, y, E::small(1), x * y};
    }
    static void to_abi(const Point& p, uint32_t* w) {
        const E zi = p.z.inv(), x = p.x * zi, y = p.y * zi;
        std::memcpy(w, x.v, 32);
        std::memcpy(w + 8, y.v, 32);
    }
};

template <class K>
struct SwLaw256 {
    using E = El256<K>;
    static constexpr int WORDS = 8;
    struct Point { E x, y, z; };
    static Point identity() { return Point{E::small(0), E::small(1), E::small(0)}; }
    static Point add(const Point& p, const Point& q) {
        const E a = K::a(), b3 = K::b3();
        const E t0 = p.x * q.x, t1 = p.y * q.y, t2 = p.z * q.z;
        const E xy = (p.x + p.y) * (q.x + q.y) - (t0 + t1);            // X1 Y2 + X2 Y1
        const E xz = (p.x + p.z) * (q.x + q.z) - (t0 + t2);            // X1 Z2 + X2 Z1
        const E yz = (p.y + p.z) * (q.y + q.z) - (t1 + t2);            // Y1 Z2 + Y2 Z1
        const E s = b3 * t2 + a * xz;
        const E xm = t1 - s, zp = t1 + s;
        const E at2 = a * t2;
        const E u = t0 + t0 + t0 + at2;                                // 3 X1 X2 + a Z1 Z2
        const E v = b3 * xz + a * (t0 - at2);
        return Point{xy * xm - yz * v, xm * zp + u * v, yz * zp + xy * u};
    }
    static Point dbl(const Point& p) { return add(p, p); }
    // 64 zero bytes are the identity, in and out (z = 0 gives x = y = 0 through 0^-1 = 0)
    static Point from_abi(const uint32_t* w) {
        uint64_t v[8];
        std::memcpy(v, w, 64);
        const E x = E::of(v), y = E::of(v + 4);
        return x.is_zero() && y.is_zero() ? identity() : Point{x, y, E::small(1)};
    }
    static void to_abi(const Point& p, uint32_t* w) {
        const E zi = p.z.inv(), x = p.x * zi, y = p.y * zi;
        std::memcpy(w, x.v, 32);
        std::memcpy(w + 8, y.v, 32);
    }
};

using Ed25519Law = TeLaw256<Ed25519K>;
using BjjLaw = TeLaw256<BjjK>;
using P256Law = SwLaw256<P256K>;
using Secp256k1Law = SwLaw256<Secp256k1K>;

// Ed25519's law for Curve25519's set sums (Edwards x || y in); the one result leaves as u || v = ((Z + Y) / (Z - Y), c (Z + Y) Z / (X (Z - Y)))
// with c = sqrt(-486664), kernels_ed25519.hip.h's Ed25519Ell2::SQRT_NEG_A_MINUS_2 as one integer: (0, -1) gives (0, 0) through 0^-1 = 0
// and the identity 64 bytes of 0xff, as c25519_store's flag becomes at the ABI
struct C25519Law : Ed25519Law {
    static void to_abi(const Point& p, uint32_t* w) {
        static const uint64_t C[4] = {0xcc6e04aaff457e06ULL, 0xc5a1d3d14b7d1a82ULL, 0xd27b08dc03fc4f7eULL, 0x0f26edf460a006bbULL};
        const E zmy = p.z - p.y, zpy = p.z + p.y;
        if (p.x.is_zero() && zmy.is_zero()) {
            std::memset(w, 0xff, 64);
            return;
        }
        const E zi = zpy * (p.x * zmy).inv(), u = zi * p.x, v = E::of(C) * zi * p.z;
        std::memcpy(w, u.v, 32);
        std::memcpy(w + 8, v.v, 32);
    }
};

// E(Fq): y^2 = x^3 + 4 over BLS12-381's base field; 96 zero bytes are the identity
struct G1hLaw {
    static constexpr int WORDS = 12;
    using Point = drh::G1;
    static Point identity() { return drh::G1::inf(); }
    static Point add(const Point& p, const Point& q) { return drh::g1_add(p, q); }
    static Point dbl(const Point& p) { return drh::g1_dbl(p); }
    static Point from_abi(const uint32_t* w) {
        uint8_t b[96];
        std::memcpy(b, w, 96);
        Point r = identity();
        bool zero = true;
        for (int i = 0; i < 96; i++) zero = zero && b[i] == 0;
        if (zero) return r;
        (void)drh::Fq::load_le(r.x, b);                    // (the callers have checked that coordinates are canonical)
        (void)drh::Fq::load_le(r.y, b + 48);
        r.zz = r.zzz = drh::Fq::one();
        return r;
    }
    static void to_abi(const Point& p, uint32_t* w) {
        uint8_t b[96] = {};
        drh::Fq x, y;
        if (drh::g1_to_affine(p, x, y)) {
            x.store_le(b);
            y.store_le(b + 48);
        }
        std::memcpy(w, b, 96);
    }
};

}  // namespace dr
