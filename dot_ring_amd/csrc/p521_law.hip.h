// P-521 (DR_CURVE_P521_RO / DR_CURVE_P521_NU; the reference's specs/p521.py) as the curve's own file: y^2 = x^3 - 3 x + b over
// p = 2^521 - 1 (fp521.hip.h, standard form), prime order, cofactor 1.  The law is sw3_law.hip.h's complete a = -3 law over this field,
// with the unfused endings (mul needs ka kb <= 6 and there is no mul2).  Here are b, that header's description of the curve, the point
// and law names the rest of the project uses, the map's description for sswu.hip.h, so that the host can check it, and the window
// count of the fixed schedule.
// Plain integer C++ like fp521.hip.h: compiles for the device and, with g++, for the host (tests/native/p521_host_check.cpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "fp521.hip.h"
#include "sw3_law.hip.h"

namespace dr {

struct P521Consts {
    // b = 0x0051953eb9618e1c9a1f929a21a0b68540eea2da725b99b315f3b8b489918ef109e156193951ec7e937b1652c0bd3bb1bf073573df883d2c34f1ef451fd46b503f00
    static constexpr int32_t B[L521] = {0xb503f00, 0x451fd46, 0xc34f1ef, 0xdf883d2, 0xf073573, 0xbd3bb1b, 0xb1652c0, 0xec7e937, 0x6193951, 0xf109e15,
                                        0x489918e, 0x15f3b8b, 0x25b99b3, 0xeea2da7, 0x0b68540, 0x929a21a, 0xe1c9a1f, 0x3eb9618, 0x0005195};
};

// sw3_law.hip.h's description of P-521: b is a full-width constant in standard form, and the field has no room for the fused endings
struct P521Sw3 {
    using Fe = F521;
    static constexpr bool FUSED = false;
    DR_L28_MEMBER static F521 b() {     // (not F521::constant<>: through it the compiler loads b from memory and the law's kernels change)
        F521 r;
#pragma unroll
        for (int i = 0; i < L521; i++) r.l[i] = P521Consts::B[i];
        return r;
    }
};
using P521Point = Sw3Point<F521>;
using P521Law = Sw3Law<P521Sw3>;
// the curve's own names of the law, as the kernels and the host programs over this header call it
DR_L28_FN P521Point p521_identity() { return P521Law::identity(); }
DR_L28_FN P521Point p521_from_affine(const F521& x, const F521& y) { return P521Law::from_affine(x, y); }
DR_L28_FN bool p521_is_identity(const P521Point& p) { return P521Law::is_identity(p); }
DR_L28_FN P521Point p521_cneg(const P521Point& p, bool negate) { return P521Law::cneg(p, negate); }
DR_L28_FN P521Point p521_dbl(const P521Point& p) { return sw3_dbl<P521Sw3>(p); }
DR_L28_FN P521Point p521_add(const P521Point& p, const P521Point& q) { return sw3_add<P521Sw3>(p, q); }

// sswu.hip.h's description of P-521: the simplified SWU map straight onto the curve (A = -3, B = b, Z = -4, no isogeny).  The field is
// in standard form, so A, Z and sqrt(-Z) = 2 are one-limb elements, -Z x is a small multiple and only B x is a full product.
struct P521Sswu : Sw3Sswu<P521Sw3> {
    DR_L28_MEMBER static F521 z() { return F521::small(-4); }
    DR_L28_MEMBER static F521 sqrt_neg_z() { return F521::small(2); }
    DR_L28_MEMBER static F521 mul_neg_z(const F521& x) { return mul_small(x, 4); }              // n
    DR_L28_MEMBER static F521 pow_p34(const F521& x) { return f521_pow_p34(x); }
};

// ---------------------------------------------------------------- the windows of the fixed schedule
// Signed 4-bit digits (wave_recode.hip.h) of a scalar k < 2^521 given as 17 words: k = sum d_w 16^w, d_w in [-8, 7], w = 0..130.  131
// nibbles cover 524 bits; nibble 130 holds bit 520 alone, so with the carry into it d_130 <= 2 and nothing leaves it: 131 windows, and
// no window for a carry out as the 448-bit schedules need.  The nibbles from 131 up come out as 8 (zero).
constexpr int P521_WINDOWS = 131;

}  // namespace dr
