// P-384 (DR_CURVE_P384_RO / DR_CURVE_P384_NU; the reference's specs/p384.py) as the curve's own file: y^2 = x^3 - 3 x + b over
// p = 2^384 - 2^128 - 2^96 + 2^32 - 1 (fp384.hip.h, Montgomery form), prime order, cofactor 1.  The law is sw3_law.hip.h's complete
// a = -3 law over this field, with the fused endings: where the last step of a coordinate is a sum of two products it is ONE
// reduction (fp384.hip.h's mul2, ka kb + kc kd <= 8), which p521_law.hip.h's field has no room for.  Here are that header's
// description of the curve, the point and law names the rest of the project uses, the map's description for sswu.hip.h, so that the
// host can check it, and the window count of the fixed schedule.
// Plain integer C++ like fp384.hip.h: compiles for the device and, with g++, for the host (tests/native/p384_host_check.cpp, where
// -fsanitize=undefined turns a signed 64-bit column overflow into an abort).
#pragma once
#include "fp384.hip.h"
#include "sw3_law.hip.h"

namespace dr {

// sw3_law.hip.h's description of P-384: b is a full-width constant in Montgomery form, and the field has room for the fused endings
struct P384Sw3 {
    using Fe = F384;
    static constexpr bool FUSED = true;
    DR_L28_MEMBER static F384 b() { return F384::constant<Fp384Consts::B>(); }
};
using P384Point = Sw3Point<F384>;
using P384Law = Sw3Law<P384Sw3>;
// the curve's own names of the law, as the kernels and the host programs over this header call it
DR_L28_FN P384Point p384_identity() { return P384Law::identity(); }
DR_L28_FN P384Point p384_from_affine(const F384& x, const F384& y) { return P384Law::from_affine(x, y); }
DR_L28_FN bool p384_is_identity(const P384Point& p) { return P384Law::is_identity(p); }
DR_L28_FN P384Point p384_cneg(const P384Point& p, bool negate) { return P384Law::cneg(p, negate); }
DR_L28_FN P384Point p384_dbl(const P384Point& p) { return sw3_dbl<P384Sw3>(p); }
DR_L28_FN P384Point p384_add(const P384Point& p, const P384Point& q) { return sw3_add<P384Sw3>(p, q); }

// sswu.hip.h's description of P-384: the simplified SWU map straight onto the curve (A = -3, B = b, Z = -12, no isogeny).  A and Z are
// the small elements -3 R and -12 R (five signed limbs each, 1 n), -Z x is the small multiple 12 x, and only B x and the product with
// sqrt(-Z) = sqrt(12) meet a full-width constant.
struct P384Sswu : Sw3Sswu<P384Sw3> {
    DR_L28_MEMBER static F384 z() { return F384::small(-12); }
    DR_L28_MEMBER static F384 sqrt_neg_z() { return F384::constant<Fp384Consts::SQRT12>(); }
    DR_L28_MEMBER static F384 mul_neg_z(const F384& x) { return mul_small(x, 12); }             // n
    DR_L28_MEMBER static F384 pow_p34(const F384& x) { return f384_pow_p34(x); }
};

// ---------------------------------------------------------------- the windows of the fixed schedule
// Signed 4-bit digits (wave_recode.hip.h) of a scalar of 12 words: 96 digits and the carry out of the top one as window 96, so every
// 384-bit value has its windows and the host refuses no scalar.
constexpr int P384_WINDOWS = 97;

}  // namespace dr
