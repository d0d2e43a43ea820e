// What the 9 x 29-bit fields share (fe25519.hip.h, fp256.hip.h, fbn254.hip.h, fsecp256k1.hip.h): the element type, the limb-wise
// operations, the column products, the 8-word <-> 9-limb bit layout and the predicates on the canonical words.
//
// An element is Limb29<F>: nine SIGNED limbs, value sum l[i] 2^(29 i).  F is the field's description, a struct of constants that is
// also the tag keeping the fields distinct types (F25, F256, Fbn and FK are aliases, overloads resolve by them).  The header assumes
// of F only what the function used needs:
//   F::reduce(int64_t (&c)[17]) -> Limb29<F>   columns c_0..c_16 of a product -> an element (mul, sqr, mul2, sqr_n); may clobber c
//   F::pack(a, w)                              the canonical representative in [0, p) as 8 little-endian words (is_zero, equal,
//                                              is_odd, is_larger)
//   F::HALF_P[8], F::PW[8]                     (p - 1) / 2 and p as words (is_larger; sub_p_if_ge)
// It guarantees: limb-wise operations (add, sub, dbl, neg, cneg, select) do not carry and do not look at the field; a product sums
// exactly the 81 (sqr: 45, mul2: 162) partial products into 17 int64 columns and hands them to F::reduce — every |column| must stay
// below 2^63, and which operand limbs achieve that (with the reduction's own additions) is the bookkeeping of the field's header, as
// is every bound on values; the layout routines move bits and nothing else.
#pragma once
#include "field.hip.h"

namespace dr {

constexpr int LIMBS29 = 9;
constexpr uint32_t MASK29 = 0x1fffffffu;

template <class F>
struct Limb29 {
    int32_t l[LIMBS29];
    DR_DEV static Limb29 zero() {
        Limb29 r;
#pragma unroll
        for (int i = 0; i < LIMBS29; i++) r.l[i] = 0;
        return r;
    }
    DR_DEV static Limb29 small(int32_t v) {          // the value v, |v| < 2^29 (in a Montgomery field: v R^-1)
        Limb29 r = zero();
        r.l[0] = v;
        return r;
    }
    template <const uint32_t (&C)[9]>
    DR_DEV static Limb29 constant() {
        Limb29 r;
#pragma unroll
        for (int i = 0; i < LIMBS29; i++) r.l[i] = (int32_t)C[i];
        return r;
    }
};

// ---------------------------------------------------------------- limb-wise, no carry
template <class F>
DR_DEV Limb29<F> add(const Limb29<F>& a, const Limb29<F>& b) {
    Limb29<F> r;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) r.l[i] = a.l[i] + b.l[i];
    return r;
}
template <class F>
DR_DEV Limb29<F> sub(const Limb29<F>& a, const Limb29<F>& b) {
    Limb29<F> r;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) r.l[i] = a.l[i] - b.l[i];
    return r;
}
template <class F>
DR_DEV Limb29<F> dbl(const Limb29<F>& a) { return add(a, a); }
template <class F>
DR_DEV Limb29<F> neg(const Limb29<F>& a) {
    Limb29<F> r;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) r.l[i] = -a.l[i];
    return r;
}
template <class F>
DR_DEV Limb29<F> cneg(const Limb29<F>& a, bool negate) {
    const int32_t s = negate ? -1 : 0;
    Limb29<F> r;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) r.l[i] = (a.l[i] ^ s) - s;
    return r;
}
template <class F>
DR_DEV Limb29<F> select(bool c, const Limb29<F>& a, const Limb29<F>& b) {
    Limb29<F> r;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) r.l[i] = c ? a.l[i] : b.l[i];
    return r;
}

// ---------------------------------------------------------------- column products over F::reduce
template <class F>
DR_DEV Limb29<F> mul(const Limb29<F>& a, const Limb29<F>& b) {
    int64_t c[17];
#pragma unroll
    for (int k = 0; k < 17; k++) c[k] = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++)
#pragma unroll
        for (int j = 0; j < LIMBS29; j++) c[i + j] += (int64_t)a.l[i] * (int64_t)b.l[j];
    return F::reduce(c);
}
template <class F>
DR_DEV Limb29<F> sqr(const Limb29<F>& a) {
    int32_t d[LIMBS29];
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) d[i] = 2 * a.l[i];
    int64_t c[17];
#pragma unroll
    for (int k = 0; k < 17; k++) c[k] = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        c[2 * i] += (int64_t)a.l[i] * (int64_t)a.l[i];
#pragma unroll
        for (int j = i + 1; j < LIMBS29; j++) c[i + j] += (int64_t)d[i] * (int64_t)a.l[j];
    }
    return F::reduce(c);
}
template <class F>
DR_DEV Limb29<F> mul2(const Limb29<F>& a, const Limb29<F>& b, const Limb29<F>& x, const Limb29<F>& y) {   // a b + x y, one reduction
    int64_t c[17];
#pragma unroll
    for (int k = 0; k < 17; k++) c[k] = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++)
#pragma unroll
        for (int j = 0; j < LIMBS29; j++) {
            c[i + j] += (int64_t)a.l[i] * (int64_t)b.l[j];
            c[i + j] += (int64_t)x.l[i] * (int64_t)y.l[j];
        }
    return F::reduce(c);
}
template <class F>
DR_DEV Limb29<F> sqr_n(Limb29<F> a, int n) {         // a^(2^n)
#pragma unroll 1
    for (int i = 0; i < n; i++) a = sqr(a);
    return a;
}

// ---------------------------------------------------------------- 8 x u32 words <-> limbs: bit 29 i of the words is bit 0 of limb i
// any 8 words -> limbs 0..7 in [0, 2^29), limb 8 = bits 232..255 (below 2^24)
template <class F>
DR_DEV Limb29<F> limbs_of_words(const uint32_t (&w)[8]) {
    Limb29<F> r;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        const int bit = 29 * i, j = bit >> 5, sh = bit & 31;
        uint32_t v = w[j] >> sh;
        if (sh > 3 && j + 1 < 8) v |= w[j + 1] << (32 - sh);
        r.l[i] = (int32_t)(v & MASK29);
    }
    return r;
}
// limbs 0..7 in [0, 2^29) and limb 8 (its bits from 24 up drop out) -> 8 words.  The packs of fe25519 and fsecp256k1 end in it; those
// of fp256 and fbn254 and bn_to_words keep the same loop in place, because through this routine the compiler orders the Montgomery
// step before it differently
DR_DEV void words_of_limbs(const uint32_t (&l)[LIMBS29], uint32_t (&w)[8]) {
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = 0;
#pragma unroll
    for (int i = 0; i < LIMBS29; i++) {
        const int bit = 29 * i, j = bit >> 5, sh = bit & 31;
        w[j] |= l[i] << sh;
        if (sh > 3 && j + 1 < 8) w[j + 1] |= l[i] >> (32 - sh);
    }
}
// w < 2 p -> w mod p: the last step of a pack
template <class F>
DR_DEV void sub_p_if_ge(uint32_t (&w)[8]) {
    uint32_t d[8], borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) d[j] = subb(w[j], F::PW[j], borrow);
    const bool ge = borrow == 0;                       // w >= p
#pragma unroll
    for (int j = 0; j < 8; j++) w[j] = ge ? d[j] : w[j];
}

// ---------------------------------------------------------------- predicates on the canonical value
template <class F>
DR_DEV bool is_zero(const Limb29<F>& a) {
    uint32_t w[8];
    F::pack(a, w);
    uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) o |= w[j];
    return o == 0;
}
template <class F>
DR_DEV bool equal(const Limb29<F>& a, const Limb29<F>& b) { return is_zero(sub(a, b)); }
// the canonical value is odd: sgn0 of RFC 9380 and the prefix bit of the SEC1 codec
template <class F>
DR_DEV bool is_odd(const Limb29<F>& a) {
    uint32_t w[8];
    F::pack(a, w);
    return (w[0] & 1u) != 0;
}
// x > p - x for the canonical x (its words w): the reference's sign rule (x > -x % p), not the parity of x
template <class F>
DR_DEV bool is_larger_words(const uint32_t (&w)[8]) {
    uint32_t borrow = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) (void)subb(F::HALF_P[j], w[j], borrow);
    return borrow != 0;                              // (p - 1) / 2 - x < 0
}
template <class F>
DR_DEV bool is_larger(const Limb29<F>& a) {
    uint32_t w[8];
    F::pack(a, w);
    return is_larger_words<F>(w);
}

}  // namespace dr
