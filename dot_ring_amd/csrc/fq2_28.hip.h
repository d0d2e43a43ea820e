// Fq2 = Fq[i] / (i^2 + 1) for BLS12-381 on the device: two Fq28 components (fq28.hip.h: 14 signed limbs of 28 bits, Montgomery form with
// R = 2^392, lazy reduction), c0 + c1 i.  Nothing of fq28.hip.h changes; every product here is one of its mul / sqr / mul2.
//
// Operand classes, per COMPONENT, against fq28.hip.h's contract (mul / sqr: 14 max|a_i| max|b_j| + 2^60 < 2^63 and |a|, |b| < 32 p;
// mul2(a, b, c, d): at most one operand with limbs up to 2^29, the others below 2^28, and |a b| + |c d| < 1024 p^2, which keeps the
// result in (-p / 2, 1.5 p) because p / R < 2^-11.2):
//   n   a product: limbs 0..12 in [0, 2^28), a small signed top limb, value in (-0.02 p, 1.02 p) when |a b| + |c d| < 50 p^2 (every
//       product below is), and in (-0.41 p, 1.41 p) at the 1024 p^2 limit
//   cK  carried: limbs 0..12 in [0, 2^28), a small signed top limb, |value| < K p.  K < 32 everywhere, so a cK is a valid operand of mul
//       on either side and of mul2 in any place (its limbs are below 2^28; a negated cK has limbs in (-2^28, 0], the same magnitude)
//   lazy  a sum or difference of two carried values before its carry: |limb| < 2^29
// A function's comment gives what it takes and returns; "K1 K2" bounds below are in units of p^2.
#pragma once
#include "kernels_g1_h2c.hip.h"

namespace dr {

struct G2hFieldConsts {
    static constexpr uint32_t INV2[14] = {0x1a3fe5cu, 0xec00000u, 0x001588cu, 0x066f369u, 0x6390970u, 0xc1d1048u, 0x01bb34fu, 0x6d07b9fu, 0x4d84da1u, 0x894bdd8u, 0x28aecc7u, 0x009653eu, 0x32cfe7du, 0x0002bbdu};      // 1 / 2, Montgomery form
};

struct Fq2 {
    Fq28 c0, c1;
    DR_DEV static Fq2 zero() { return {Fq28::zero(), Fq28::zero()}; }
    DR_DEV static Fq2 one() { return {Fq28::one(), Fq28::zero()}; }
    template <const uint32_t (&C)[2][14]>
    DR_DEV static Fq2 constant() {
        Fq2 r;
#pragma unroll
        for (int i = 0; i < L28; i++) { r.c0.l[i] = (int32_t)C[0][i]; r.c1.l[i] = (int32_t)C[1][i]; }
        return r;
    }
};

// ---------------------------------------------------------------- the cheap operations: limb-wise, no carry unless the name says so
// add / sub / dbl: carried in, lazy out (|limb| < 2^29): carry before a product.  neg / conj / cneg: cK in, limbs in (-2^28, 2^28) out,
// the same |value|; they may feed a product as they are.
DR_DEV Fq2 add(const Fq2& a, const Fq2& b) { return {add(a.c0, b.c0), add(a.c1, b.c1)}; }
DR_DEV Fq2 sub(const Fq2& a, const Fq2& b) { return {sub(a.c0, b.c0), sub(a.c1, b.c1)}; }
DR_DEV Fq2 dbl(const Fq2& a) { return {dbl(a.c0), dbl(a.c1)}; }
DR_DEV Fq2 neg(const Fq2& a) { return {neg(a.c0), neg(a.c1)}; }
DR_DEV Fq2 conj(const Fq2& a) { return {a.c0, neg(a.c1)}; }
DR_DEV Fq2 cneg(const Fq2& a, bool negate) { return {cneg(a.c0, negate), cneg(a.c1, negate)}; }
DR_DEV Fq2 carry(const Fq2& a) { return {carry(a.c0), carry(a.c1)}; }                  // |limb| < 2^30 in, carried out, value unchanged
DR_DEV Fq2 select(bool c, const Fq2& a, const Fq2& b) { return {select(c, a.c0, b.c0), select(c, a.c1, b.c1)}; }

// a carried value in (-K p, L p) -> carried in (-(K - 1) p, L p) for K >= 1 (and unchanged range for a non-negative one): adds p where
// the value is negative.  Exact sign: limbs 0..12 are non-negative and sum below 2^364, so the value is negative iff the top limb is.
// The sum's limbs stay below 2^29 and are carried again.
DR_DEV Fq28 fq_fold(const Fq28& a) {
    const bool negative = a.l[L28 - 1] < 0;
    Fq28 r;
#pragma unroll
    for (int i = 0; i < L28; i++) r.l[i] = a.l[i] + (negative ? (int32_t)Fq28Params::P[i] : 0);
    return carry(r);
}

// ---------------------------------------------------------------- products
// a b: components cKa, cKb (or negations of such) with 2 Ka Kb < 1024; n out.  Two fused pairs, one reduction each:
// a0 b0 + (-a1) b1 and a0 b1 + a1 b0.
DR_DEV Fq2 mul(const Fq2& a, const Fq2& b) { return {mul2(a.c0, b.c0, neg(a.c1), b.c1), mul2(a.c0, b.c1, a.c1, b.c0)}; }
// a^2 = (a0 + a1)(a0 - a1) + 2 a0 a1 i: components cK with 4 K^2 < 1024 (K < 16) for the first product (both factors carried, below
// 2 K p) and limbs of 2 a0 below 2^29 for the second (sqr-style bound 2^29 x 2^28); n out
DR_DEV Fq2 sqr(const Fq2& a) { return {mul(carry(add(a.c0, a.c1)), carry(sub(a.c0, a.c1))), mul(dbl(a.c0), a.c1)}; }
// a s for s in Fq: cKa x cKs with Ka Ks < 1024; n out
DR_DEV Fq2 mul_fq(const Fq2& a, const Fq28& s) { return {mul(a.c0, s), mul(a.c1, s)}; }
// a0^2 + a1^2 in Fq: components cK with 2 K^2 < 1024; n out
DR_DEV Fq28 norm(const Fq2& a) { return mul2(a.c0, a.c0, a.c1, a.c1); }
// a b + c d with FOUR reductions instead of the six of two products and a sum, paired so that each fused pair holds one term of either
// product:  c0 = (a0 b0 + c0 d0) + ((-a1) b1 + (-c1) d1),  c1 = (a0 b1 + a1 b0) + (c0 d1 + c1 d0).  Components cKa .. cKd with
// Ka Kb + Kc Kd < 1024 (first row) and 2 Ka Kb < 1024, 2 Kc Kd < 1024 (second row).  Out: the carried sum of two n, c2.1 (c2.9 at the
// 1024 limit).
DR_DEV Fq2 mul_add(const Fq2& a, const Fq2& b, const Fq2& c, const Fq2& d) {
    Fq2 r;
    r.c0 = carry(add(mul2(a.c0, b.c0, c.c0, d.c0), mul2(neg(a.c1), b.c1, neg(c.c1), d.c1)));
    r.c1 = carry(add(mul2(a.c0, b.c1, a.c1, b.c0), mul2(c.c0, d.c1, c.c1, d.c0)));
    return r;
}
// a^-1 = conj(a) / norm(a) (0 -> 0, as fq28.hip.h's inv): components cK, 2 K^2 < 1024; n out.  One division-step inversion in Fq (its
// canon28 takes the norm, an n).
DR_DEV Fq2 inv(const Fq2& a) {
    const Fq28 ni = inv(norm(a));
    return {mul(a.c0, ni), mul(neg(a.c1), ni)};
}

// 12 (1 + i) a = 12 (a0 - a1) + 12 (a0 + a1) i by additions and carries, as g1h_mul12.  a: components in (-0.1 p, 1.1 p) (an n, or a
// carried value folded into that range).  a0 - a1 and a0 + a1 - p both lie in (-1.2 p, 1.2 p); one fold brings them into (-0.2 p, 1.2 p),
// and g1h_mul12 (carried limbs x 4, then x 3: below 2^30) gives components in (-2.4 p, 14.4 p): c14.4 — for n components (-0.5 p,
// 12.5 p).  Without the fold the components would span 12 p either way, and the doubling's Y^2 - 3 b3 Z^2 38 p: past mul's 32 p.
DR_DEV Fq2 mul_b3(const Fq2& a) {
    const Fq28 d0 = fq_fold(carry(sub(a.c0, a.c1)));
    const Fq28 d1 = fq_fold(carry(sub(add(a.c0, a.c1), Fq28::constant<Fq28Params::P>())));
    return {g1h_mul12(d0), g1h_mul12(d1)};
}

// ---------------------------------------------------------------- predicates on the canonical value (components cK, K < 32: from_mont28)
DR_DEV bool is_zero(const Fq2& a) { return g1h_is_zero(a.c0) && g1h_is_zero(a.c1); }
DR_DEV bool equal(const Fq2& a, const Fq2& b) { return is_zero(carry(sub(a, b))); }      // a, b: cK with K < 16
// sgn0 of RFC 9380 4.1 for m = 2 (the reference's Fp2.sgn0): the parity of c0, or of c1 where c0 = 0
DR_DEV bool sgn0(const Fq2& a) {
    uint32_t w0[12], w1[12], any0 = 0;
    from_mont28(a.c0, w0);
    from_mont28(a.c1, w1);
#pragma unroll
    for (int j = 0; j < 12; j++) any0 |= w0[j];
    return ((w0[0] & 1u) | ((any0 == 0 ? 1u : 0u) & (w1[0] & 1u))) != 0;
}

// ---------------------------------------------------------------- square roots from Fq operations (p = 3 mod 4, i^2 = -1)
// a is a square in Fq2 iff norm(a) is one in Fq (a^((p^2 - 1) / 2) = norm(a)^((p - 1) / 2)).  root_norm: s = v v^((p - 3) / 4) for v =
// norm(a), and whether s^2 = v; ONE exponentiation.  a: components cK, 2 K^2 < 1024.
DR_DEV bool fq2_norm_root(const Fq2& a, Fq28& s) {
    const Fq28 v = norm(a);
    s = mul(g1h_pow_p34(v), v);
    return g1h_is_zero(sub(sqr(s), v));
}
// a root of a SQUARE a (components n) given s with s^2 = norm(a): ONE exponentiation and ONE inversion in Fq.
//   a1 != 0:  d = (a0 + s) / 2 and (a0 - s) / 2 multiply to -a1^2 / 4, a non-square, so exactly one of them is a square.  With r = d^((p +
//             1) / 4) and t = a1 / (2 r): either r^2 = d, then r^2 - t^2 = d - (s - a0) / 2 = a0 and the root is (r, t); or r^2 = -d,
//             then t^2 - r^2 = (a0 - s) / 2 + d = a0 and the root is (t, r).  2 r t = a1 both times.
//   a1 == 0:  s = +-a0 would make d = 0 for one sign, so d = a0 itself: r^2 = a0 gives (r, 0), r^2 = -a0 gives (0, r) — Fp2.sqrt's case.
// Which of the two roots comes out is left to the caller's sgn0.  a = 0 gives (0, 0) (inv(0) = 0).  One select, no branch.
DR_DEV Fq2 fq2_sqrt_with(const Fq2& a, const Fq28& s) {
    const bool real = g1h_is_zero(a.c1);
    const Fq28 half = mul(carry(add(a.c0, s)), Fq28::constant<G2hFieldConsts::INV2>());          // c2.1 x n
    const Fq28 d = select(real, a.c0, half);
    const Fq28 r = mul(g1h_pow_p34(d), d);
    const bool direct = g1h_is_zero(sub(sqr(r), d));
    const Fq28 t = mul(a.c1, inv(carry(dbl(r))));                                                // a1 / (2 r); 0 when a1 = 0
    return {select(direct, r, t), select(direct, t, r)};
}
// the general form: whether a is a square, and then a root of it (else unspecified); two exponentiations and one inversion
DR_DEV bool fq2_sqrt(const Fq2& a, Fq2& root) {
    Fq28 s;
    const bool ok = fq2_norm_root(a, s);
    root = fq2_sqrt_with(a, s);
    return ok;
}

}  // namespace dr
