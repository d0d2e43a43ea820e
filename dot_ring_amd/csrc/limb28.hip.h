// What the signed 28-bit fields share (fe448.hip.h: 16 limbs, fp521.hip.h: 19, fp384.hip.h: 14): the element type, the limb-wise
// operations, the words <-> limbs bit layout, the predicates on the canonical limbs, the "add p, take p off twice" canonicaliser of the
// two standard-form fields, the plain column products of the Montgomery one, the field selftests' store of a record, and the two bases
// their laws and curve descriptions derive from.  Plain integer C++: compiles for the device (hipcc) and for the host (g++, tests/native/*_host_check.cpp).
//
// An element is Limb28<F>: F::LIMBS SIGNED limbs, value sum l[i] 2^(28 i).  F is the field's description, a struct of constants that is
// also the tag keeping the fields distinct types (F448, F521 and F384 are aliases, overloads resolve by them).  The header assumes of
// F only what the function used needs:
//   F::LIMBS, F::WORDS                      the limbs of an element and the 32-bit words of a canonical one; every limb starts inside the
//                                           words and every word holds bits of a limb (asserted by the layout routines)
//   F::small(v) -> Limb28<F>                the element v for a small v (P-384: v R spread over four limbs)
//   canon_limbs(a, u)                       the limbs of the representative in [0, p), limbs 0..LIMBS - 2 in [0, 2^28) (pack, is_zero,
//                                           is_odd, equal): the one below, or the field's own overload (fp384.hip.h)
//   F::p_limb(i), F::TOP_BITS, carry(a)     limb i of p, the bits of limb LIMBS - 1 of a canonical value, and the field's ripple
//                                           (the canon_limbs below)
//   F::unpack(w) -> Limb28<F>               the element of WORDS canonical words (Limb28Law, Limb28Curve)
//   F::reduce(int64_t (&c)[2 LIMBS - 1])    columns of a product -> an element; may clobber c (mul, mul2, sqr)
// It guarantees: limb-wise operations (add, sub, dbl, neg, cneg, select) do not carry and do not look at the field; mul, mul2 and sqr
// sum exactly the LIMBS^2 (mul2: twice that; sqr: LIMBS (LIMBS + 1) / 2) partial products into 2 LIMBS - 1 int64 columns and hand them
// to F::reduce — every |column| must stay below 2^63, and which operand limbs achieve that (with the reduction's own additions) is the
// bookkeeping of the field's header, as is every bound on values ("n", "k n", the contracts); the layout routines move bits and
// nothing else; the predicates see the canonical value alone.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define DR_L28_FN __host__ __device__ __forceinline__
#define DR_L28_MEMBER __host__ __device__ __forceinline__
#else
#define DR_L28_FN static inline
#define DR_L28_MEMBER inline
#endif

namespace dr {

constexpr int32_t MASK28 = 0x0fffffff;

template <class F>
struct Limb28 {
    using Field = F;
    int32_t l[F::LIMBS];
    DR_L28_MEMBER static Limb28 zero() {
        Limb28 r;
#pragma unroll
        for (int i = 0; i < F::LIMBS; i++) r.l[i] = 0;
        return r;
    }
    DR_L28_MEMBER static Limb28 small(int32_t v) { return F::small(v); }
    template <const int32_t (&C)[F::LIMBS]>
    DR_L28_MEMBER static Limb28 constant() {
        Limb28 r;
#pragma unroll
        for (int i = 0; i < F::LIMBS; i++) r.l[i] = C[i];
        return r;
    }
};

// ---------------------------------------------------------------- limb-wise, no carry
template <class F>
DR_L28_FN Limb28<F> add(const Limb28<F>& a, const Limb28<F>& b) {
    Limb28<F> r;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}
template <class F>
DR_L28_FN Limb28<F> sub(const Limb28<F>& a, const Limb28<F>& b) {
    Limb28<F> r;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) r.l[i] = a.l[i] - b.l[i];
    return r;
}
template <class F>
DR_L28_FN Limb28<F> dbl(const Limb28<F>& a) { return add(a, a); }
template <class F>
DR_L28_FN Limb28<F> neg(const Limb28<F>& a) {
    Limb28<F> r;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) r.l[i] = -a.l[i];
    return r;
}
template <class F>
DR_L28_FN Limb28<F> cneg(const Limb28<F>& a, bool negate) {      // negate ? -a : a
    const int32_t s = negate ? -1 : 0;
    Limb28<F> r;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) r.l[i] = (a.l[i] ^ s) - s;
    return r;
}
template <class F>
DR_L28_FN Limb28<F> select(bool c, const Limb28<F>& a, const Limb28<F>& b) {   // c ? a : b
    Limb28<F> r;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}

// ---------------------------------------------------------------- column products over F::reduce (the fields whose reduction is not
// folded into the column loop: fp384.hip.h)
template <class F>
DR_L28_FN Limb28<F> mul(const Limb28<F>& a, const Limb28<F>& b) {
    int64_t c[2 * F::LIMBS - 1];
#pragma unroll
    for (int j = 0; j < 2 * F::LIMBS - 1; j++) {
        int64_t s = 0;
#pragma unroll
        for (int i = 0; i < F::LIMBS; i++)
            if (j - i >= 0 && j - i < F::LIMBS) s += (int64_t)a.l[i] * b.l[j - i];
        c[j] = s;
    }
    return F::reduce(c);
}
template <class F>
DR_L28_FN Limb28<F> mul2(const Limb28<F>& a, const Limb28<F>& b, const Limb28<F>& c, const Limb28<F>& d) {   // a b + c d, one reduction
    int64_t col[2 * F::LIMBS - 1];
#pragma unroll
    for (int j = 0; j < 2 * F::LIMBS - 1; j++) {
        int64_t s = 0;
#pragma unroll
        for (int i = 0; i < F::LIMBS; i++)
            if (j - i >= 0 && j - i < F::LIMBS) s += (int64_t)a.l[i] * b.l[j - i] + (int64_t)c.l[i] * d.l[j - i];
        col[j] = s;
    }
    return F::reduce(col);
}
// the off-diagonal products once, against the doubled operand
template <class F>
DR_L28_FN Limb28<F> sqr(const Limb28<F>& a) {
    int32_t a2[F::LIMBS];
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) a2[i] = 2 * a.l[i];
    int64_t c[2 * F::LIMBS - 1];
#pragma unroll
    for (int j = 0; j < 2 * F::LIMBS - 1; j++) {
        int64_t s = 0;
#pragma unroll
        for (int i = 0; i < F::LIMBS; i++) {
            const int m = j - i;
            if (m >= i && m < F::LIMBS) s += i == m ? (int64_t)a.l[i] * a.l[i] : (int64_t)a2[i] * a.l[m];
        }
        c[j] = s;
    }
    return F::reduce(c);
}
template <class F>
DR_L28_FN Limb28<F> sqr_n(Limb28<F> a, int n) {         // a^(2^n), by the field's own sqr
#pragma unroll 1
    for (int i = 0; i < n; i++) a = sqr(a);
    return a;
}

// ---------------------------------------------------------------- WORDS x u32 words <-> limbs: bit 28 i of the words is bit 0 of limb i
template <class F>
constexpr bool limb28_layout_fits() { return 28 * (F::LIMBS - 1) < 32 * F::WORDS && 28 * F::LIMBS > 32 * (F::WORDS - 1); }
// any words -> limbs in [0, 2^28) (no arithmetic: the value is reinterpreted in radix 2^28); bits of the words from 28 LIMBS up are
// not read
template <class F>
DR_L28_FN Limb28<F> limbs_of_words(const uint32_t (&w)[F::WORDS]) {
    static_assert(limb28_layout_fits<F>(), "every limb starts inside the words and every word holds bits of a limb");
    Limb28<F> r;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) {
        const int bit = 28 * i, j = bit >> 5, sh = bit & 31;
        uint32_t v = w[j] >> sh;
        if (sh > 4 && j + 1 < F::WORDS) v |= w[j + 1] << (32 - sh);
        r.l[i] = (int32_t)(v & (uint32_t)MASK28);
    }
    return r;
}
// canonical limbs (limbs 0..LIMBS - 2 in [0, 2^28), the value below 2^(32 WORDS)) -> words
template <class F>
DR_L28_FN void words_of_limbs(const int32_t (&u)[F::LIMBS], uint32_t (&w)[F::WORDS]) {
    static_assert(limb28_layout_fits<F>(), "every limb starts inside the words and every word holds bits of a limb");
#pragma unroll
    for (int j = 0; j < F::WORDS; j++) w[j] = 0;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) {
        const int bit = 28 * i, j = bit >> 5, sh = bit & 31;
        const uint32_t v = (uint32_t)u[i];
        w[j] |= v << sh;
        if (sh > 4 && j + 1 < F::WORDS) w[j + 1] |= v >> (32 - sh);
    }
}
// ---------------------------------------------------------------- canonical limbs of a standard-form field
// The limbs of the representative in [0, p): limbs 0..LIMBS - 2 in [0, 2^28), limb LIMBS - 1 in [0, 2^TOP_BITS).  The field's carry
// leaves a value within p of [0, 2^(28 (LIMBS - 1) + TOP_BITS)); + p is positive and below 3 p, so p is taken off twice where it fits.
template <class F>
DR_L28_FN void canon_limbs(const Limb28<F>& a, int32_t (&u)[F::LIMBS]) {
    const Limb28<F> x = carry(a);
    int32_t c = 0;
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) {
        const int bits = i == F::LIMBS - 1 ? F::TOP_BITS : 28;
        const int32_t t = x.l[i] + F::p_limb(i) + c;
        u[i] = t & ((1 << bits) - 1);
        c = t >> bits;
    }
    int32_t top = c;                                    // 0, 1 or 2
#pragma unroll
    for (int pass = 0; pass < 2; pass++) {
        int32_t d[F::LIMBS];
        c = 0;
#pragma unroll
        for (int i = 0; i < F::LIMBS; i++) {
            const int bits = i == F::LIMBS - 1 ? F::TOP_BITS : 28;
            const int32_t t = u[i] - F::p_limb(i) + c;
            d[i] = t & ((1 << bits) - 1);
            c = t >> bits;
        }
        const int32_t dt = top + c;
        const bool take = dt >= 0;
#pragma unroll
        for (int i = 0; i < F::LIMBS; i++) u[i] = take ? d[i] : u[i];
        top = take ? dt : top;
    }
}

// the canonical representative in [0, p) as little-endian words: the field's canonicaliser, then the layout
template <class F>
DR_L28_FN void pack(const Limb28<F>& a, uint32_t (&w)[F::WORDS]) {
    int32_t u[F::LIMBS];
    canon_limbs(a, u);
    words_of_limbs<F>(u, w);
}

// ---------------------------------------------------------------- predicates on the canonical value
template <class F>
DR_L28_FN bool is_zero(const Limb28<F>& a) {
    int32_t u[F::LIMBS], acc = 0;
    canon_limbs(a, u);
#pragma unroll
    for (int i = 0; i < F::LIMBS; i++) acc |= u[i];
    return acc == 0;
}
// the canonical value is odd: sgn0 of RFC 9380 and the prefix bit of the SEC1 codec
template <class F>
DR_L28_FN bool is_odd(const Limb28<F>& a) {
    int32_t u[F::LIMBS];
    canon_limbs(a, u);
    return (u[0] & 1) != 0;
}
template <class F>
DR_L28_FN bool equal(const Limb28<F>& a, const Limb28<F>& b) { return is_zero(sub(a, b)); }

// Record r of a lane's output as canonical words, for the field selftests (k_ed448_, k_p521_, k_p384_field_selftest; the record lists
// are theirs, and so is the loop that loads the two raw limb images: behind a shared routine the compiler orders all three kernels
// differently)
template <class F>
DR_L28_FN void field_selftest_put(uint32_t* o, int r, const Limb28<F>& v) {
    uint32_t w[F::WORDS];
    pack(v, w);
#pragma unroll
    for (int j = 0; j < F::WORDS; j++) o[r * F::WORDS + j] = w[j];
}

// ---------------------------------------------------------------- what the laws and the curve descriptions over these fields share
// The ABI's affine x || y words <-> a projective point (X : Y : Z), x = X / Z, y = Y / Z, as the host side of dr_wide_msm takes a law
// (wide_combine.hpp).  Law gives identity(), from_affine(x, y) and ZERO_IS_IDENTITY: whether zero words are the identity, which then
// has Z = 0 and stores them by 0^-1 = 0.  (M448Law's points cross the ABI as Montgomery (u, v): it keeps its own pair.)
template <class Law, class P>
struct Limb28Law {
    using Point = P;
    using Fe = decltype(P::x);
    static constexpr int WORDS = Fe::Field::WORDS, LIMBS = Fe::Field::LIMBS;
    DR_L28_MEMBER static P from_abi(const uint32_t (&w)[2 * WORDS]) {
        uint32_t x[WORDS], y[WORDS], o = 0;
        for (int j = 0; j < WORDS; j++) { x[j] = w[j]; y[j] = w[WORDS + j]; o |= x[j] | y[j]; }
        if (Law::ZERO_IS_IDENTITY && o == 0) return Law::identity();
        return Law::from_affine(Fe::Field::unpack(x), Fe::Field::unpack(y));
    }
    DR_L28_MEMBER static void to_abi(const P& p, uint32_t (&w)[2 * WORDS]) {
        const Fe zi = inv(p.z);
        uint32_t x[WORDS], y[WORDS];
        pack(mul(p.x, zi), x);
        pack(mul(p.y, zi), y);
        for (int j = 0; j < WORDS; j++) { w[j] = x[j]; w[WORDS + j] = y[j]; }
    }
};
// The part of wave_curve.hip.h's description of a curve that its field decides: canonical words at the ABI and the limb images, as
// they are, in the LDS table.  (It supplies no inv: that stays a one-line forwarder in each description, because from here
// k_ed448_field_selftest changes, DESIGN.md section 8x.  to_lds / from_lds spell out the loops of wave_curve.hip.h's
// wave_limbs_to_words / wave_words_to_limbs: this header compiles for the host and so does not include field.hip.h or what builds on it.)
template <class F>
struct Limb28Curve {
    using Fe = Limb28<F>;
    static constexpr int WORDS = F::WORDS, LDS_WORDS = F::LIMBS;
    DR_L28_MEMBER static Fe unpack(const uint32_t (&w)[WORDS]) { return F::unpack(w); }
    DR_L28_MEMBER static void pack(const Fe& a, uint32_t (&w)[WORDS]) { dr::pack(a, w); }
    DR_L28_MEMBER static void to_lds(const Fe& a, uint32_t (&w)[LDS_WORDS]) {
#pragma unroll
        for (int i = 0; i < LDS_WORDS; i++) w[i] = (uint32_t)a.l[i];
    }
    DR_L28_MEMBER static Fe from_lds(const uint32_t (&w)[LDS_WORDS]) {
        Fe a;
#pragma unroll
        for (int i = 0; i < LDS_WORDS; i++) a.l[i] = (int32_t)w[i];
        return a;
    }
};

}  // namespace dr
