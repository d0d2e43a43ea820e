// The wave-per-workgroup scalar-multiplication family of every curve with kernels of its own — the four native 256-bit curves (Ed25519,
// Baby JubJub, P-256, secp256k1), BLS12-381's E(Fq) (48-byte coordinates), Ed448, Curve448 (56-byte coordinates and scalars), P-521
// (68-byte) and P-384 (48-byte coordinates and scalars) — as one set of templates over a description C of the curve: the memory forms, the fixed-schedule scalar multiplication the
// provers' secret scalars go through, the two kernel bodies built on it, a diagnostic of the law on raw limb images, and the SEC1-compressed decoder.  kernels_ed25519.hip.h
// (Ed25519Curve), kernels_bjj.hip.h (BjjCurve), kernels_p256.hip.h (P256Curve), kernels_secp256k1.hip.h (Secp256k1Curve),
// kernels_g1_h2c.hip.h (G1hCurve), kernels_ed448.hip.h (Ed448Curve), kernels_curve448.hip.h (Curve448Curve), kernels_p521.hip.h
// (P521Curve) and kernels_p384.hip.h (P384Curve) each give a field, a group law, one description and one thin named __global__ per kernel; the schedule below exists once.
// C provides
//   Fe, Point                      the field element (int32_t limbs l[]) and the point: members x, y, z and, when EXTENDED, t
//   WORDS                          the 32-bit words of a coordinate at the ABI: 8, 12, 14 or 17 (any count).  A point is 2 WORDS words
//                                  (x || y) and moves as the widest of uint4 / uint2 / words that divides its byte length
//   SCALAR_WORDS                   the 32-bit words of a scalar at the ABI: 8, 12, 14 or 17; it moves the same way
//   BLOCK, WINDOWS                 the workgroup size (64: one wave) and the number of signed 4-bit windows of a scalar: 8 SCALAR_WORDS + 1
//                                  where a carry can leave the top digit (65: an order of 256 bits; 97: any k < 2^384; 113: any k < 2^448), otherwise the
//                                  digits that can be non-zero (64: an order below 2^255; 131: k < 2^521, p521_law.hip.h)
//   EXTENDED, LDS_WORDS            whether the point has a fourth coordinate t; the words of one coordinate in the LDS table
//   ZERO_IS_IDENTITY               whether zero bytes stand for the identity at the ABI (the Weierstrass curves: (0, 0) is no point)
//   unpack(w), pack(a, w), inv(a)  the ABI's canonical WORDS words <-> an element (in the field's own form); a^-1 with 0^-1 = 0
//   to_lds(a, w), from_lds(w)      a normal coordinate <-> its LDS_WORDS table words (canonical or Montgomery words, or the limb image)
//   identity(), from_affine(x, y)  the neutral element; the point of affine coordinates
//   add(P, Q), dbl(P)              the unified / complete addition and the doubling (all coordinates)
//   dbl_no_t(P)                    when EXTENDED: the doubling without t (three of a window's four doublings are only doubled again)
//   cneg(P, b)                     -P if b
//   load_scalar(p, k)              SCALAR_WORDS words at p reduced mod the group order, or (G1hCurve, Ed448Curve, P521Curve) as they
//                                  are: E(Fq) and E448 are not of prime order, and the windows take every scalar of the width (P-521:
//                                  every k < 2^521; the host refuses others)
// and, for sec1_decode:  below_p(w), y_of_x(x, y) (a root of the curve equation, false if none), is_odd(y) (of the canonical value),
// and with CHECK in_subgroup(x, y).  Curve448Curve, whose points cross the ABI as Montgomery (u, v) with a flag word, gives the law and
// the table forms only: its kernels (and kernels_curve25519.hip.h's over Ed25519Curve) call the core from bodies of their own.
// The four descriptions over the signed 28-bit fields derive Fe, WORDS, LDS_WORDS, unpack, pack, to_lds and from_lds from limb28.hip.h's
// Limb28Curve<F>.
#pragma once
#include "field.hip.h"
#include "wave_recode.hip.h"

namespace dr {

constexpr int WAVE_TABLE = 8;         // entries 1P..8P: what a signed 4-bit digit can select

DR_DEV void wave_load8(const uint32_t* p, uint32_t (&w)[8]) {
    const uint4* q = reinterpret_cast<const uint4*>(p);
    const uint4 a = q[0], b = q[1];
    w[0] = a.x; w[1] = a.y; w[2] = a.z; w[3] = a.w;
    w[4] = b.x; w[5] = b.y; w[6] = b.z; w[7] = b.w;
}
DR_DEV void wave_store8(uint32_t* p, const uint32_t (&w)[8]) {
    uint4* q = reinterpret_cast<uint4*>(p);
    q[0] = make_uint4(w[0], w[1], w[2], w[3]);
    q[1] = make_uint4(w[4], w[5], w[6], w[7]);
}
DR_DEV void wave_store_zero8(uint32_t* p) {
    const uint32_t z[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    wave_store8(p, z);
}
// the same for N words of any count: they move as the widest of uint4 / uint2 / words that divides their byte length (N = 8: the three
// above; seven uint4 for a point of 2 x 14 words, seven uint2 for a scalar of 14, seventeen uint2 for a point of 2 x 17)
template <int N>
DR_DEV void wave_load_words(const uint32_t* p, uint32_t (&w)[N]) {
    if constexpr (N == 8) {
        wave_load8(p, w);
    } else if constexpr (N % 4 == 0) {
        const uint4* q = reinterpret_cast<const uint4*>(p);
#pragma unroll
        for (int j = 0; j < N / 4; j++) {
            const uint4 a = q[j];
            w[4 * j] = a.x; w[4 * j + 1] = a.y; w[4 * j + 2] = a.z; w[4 * j + 3] = a.w;
        }
    } else if constexpr (N % 2 == 0) {
        const uint2* q = reinterpret_cast<const uint2*>(p);
#pragma unroll
        for (int j = 0; j < N / 2; j++) {
            const uint2 a = q[j];
            w[2 * j] = a.x; w[2 * j + 1] = a.y;
        }
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) w[j] = p[j];
    }
}
template <int N>
DR_DEV void wave_store_words(uint32_t* p, const uint32_t (&w)[N]) {
    if constexpr (N == 8) {
        wave_store8(p, w);
    } else if constexpr (N % 4 == 0) {
        uint4* q = reinterpret_cast<uint4*>(p);
#pragma unroll
        for (int j = 0; j < N / 4; j++) q[j] = make_uint4(w[4 * j], w[4 * j + 1], w[4 * j + 2], w[4 * j + 3]);
    } else if constexpr (N % 2 == 0) {
        uint2* q = reinterpret_cast<uint2*>(p);
#pragma unroll
        for (int j = 0; j < N / 2; j++) q[j] = make_uint2(w[2 * j], w[2 * j + 1]);
    } else {
#pragma unroll
        for (int j = 0; j < N; j++) p[j] = w[j];
    }
}
template <int N>
DR_DEV void wave_store_zero_words(uint32_t* p) {
    const uint32_t z[N] = {};
    wave_store_words(p, z);
}
// a point, x || y of W words each: coordinate by coordinate where a coordinate is a whole number of uint4 (W = 8, 12), otherwise as one
// run of 2 W words (a coordinate of 14 or 17 words alone is not aligned to the vector its point moves as)
template <int W>
DR_DEV void wave_load_point_words(const uint32_t* p, uint32_t (&x)[W], uint32_t (&y)[W]) {
    if constexpr (W % 4 == 0) {
        wave_load_words(p, x);
        wave_load_words(p + W, y);
    } else {
        uint32_t w[2 * W];
        wave_load_words(p, w);
#pragma unroll
        for (int j = 0; j < W; j++) { x[j] = w[j]; y[j] = w[W + j]; }
    }
}
template <int W>
DR_DEV void wave_store_point_words(uint32_t* p, const uint32_t (&x)[W], const uint32_t (&y)[W]) {
    if constexpr (W % 4 == 0) {
        wave_store_words(p, x);
        wave_store_words(p + W, y);
    } else {
        uint32_t w[2 * W];
#pragma unroll
        for (int j = 0; j < W; j++) { w[j] = x[j]; w[W + j] = y[j]; }
        wave_store_words(p, w);
    }
}

// ---------------------------------------------------------------- memory
template <class C>
DR_DEV typename C::Fe wave_load_fe(const uint32_t* p) {
    uint32_t w[C::WORDS];
    wave_load_words(p, w);
    return C::unpack(w);
}
template <class C>
DR_DEV void wave_store_fe(uint32_t* p, const typename C::Fe& a) {
    uint32_t w[C::WORDS];
    C::pack(a, w);
    wave_store_words(p, w);
}
// x || y of the point; where the identity has Z = 0, x = y = 0 after the multiplication by 0^-1 = 0: it stores zero bytes
template <class C>
DR_DEV void wave_store_affine(uint32_t* out, const typename C::Point& acc) {
    const typename C::Fe zi = C::inv(acc.z);
    if constexpr (C::WORDS % 4 == 0) {
        wave_store_fe<C>(out, mul(acc.x, zi));
        wave_store_fe<C>(out + C::WORDS, mul(acc.y, zi));
    } else {
        uint32_t x[C::WORDS], y[C::WORDS];
        C::pack(mul(acc.x, zi), x);
        C::pack(mul(acc.y, zi), y);
        wave_store_point_words(out, x, y);
    }
}
// One term of a batch: the point of affine x || y (2 WORDS words, canonical) at pt and the scalar at kp, reduced into k.  The scalar is
// reduced before the point is built from its coordinates (an extended point costs a product that nothing needs across that loop).
template <class C>
DR_DEV typename C::Point wave_load_term(const uint32_t* pt, const uint32_t* kp, uint32_t (&k)[C::SCALAR_WORDS]) {
    uint32_t x[C::WORDS], y[C::WORDS];
    wave_load_point_words(pt, x, y);
    [[maybe_unused]] uint32_t o = 0;
#pragma unroll
    for (int j = 0; j < C::WORDS; j++) o |= x[j] | y[j];
    const typename C::Fe px = C::unpack(x), py = C::unpack(y);
    C::load_scalar(kp, k);
    typename C::Point r = C::from_affine(px, py);
    if constexpr (C::ZERO_IS_IDENTITY) {
        if (o == 0) r = C::identity();
    }
    return r;
}
// the limb image of a coordinate as table words: what to_lds / from_lds are where the table keeps limbs (no packing)
template <class Fe, int N>
DR_DEV void wave_limbs_to_words(const Fe& a, uint32_t (&w)[N]) {
    static_assert(N == sizeof(a.l) / sizeof(a.l[0]), "LDS_WORDS of a limb-image table is the field's limb count");
#pragma unroll
    for (int i = 0; i < N; i++) w[i] = (uint32_t)a.l[i];
}
template <class Fe, int N>
DR_DEV Fe wave_words_to_limbs(const uint32_t (&w)[N]) {
    Fe a;
    static_assert(N == sizeof(a.l) / sizeof(a.l[0]), "LDS_WORDS of a limb-image table is the field's limb count");
#pragma unroll
    for (int i = 0; i < N; i++) a.l[i] = (int32_t)w[i];
    return a;
}
// LDS table [entry][word][lane] (bank = lane whatever the entry)
template <class C>
constexpr int wave_table_words() { return WAVE_TABLE * (C::EXTENDED ? 4 : 3) * C::LDS_WORDS * C::BLOCK; }
template <class C>
DR_DEV void wave_lds_store(uint32_t* tab, int entry, int lane, const typename C::Point& p) {
    constexpr int W = C::LDS_WORDS, B = C::BLOCK;
    uint32_t* base = tab + (size_t)entry * (wave_table_words<C>() / WAVE_TABLE) + lane;
    [[maybe_unused]] uint32_t x[W], y[W], z[W], t[W];
    C::to_lds(p.x, x); C::to_lds(p.y, y); C::to_lds(p.z, z);
    if constexpr (C::EXTENDED) C::to_lds(p.t, t);
#pragma unroll
    for (int i = 0; i < W; i++) {
        base[(0 + i) * B] = x[i];
        base[(W + i) * B] = y[i];
        base[(2 * W + i) * B] = z[i];
        if constexpr (C::EXTENDED) base[(3 * W + i) * B] = t[i];
    }
}
template <class C>
DR_DEV typename C::Point wave_lds_load(const uint32_t* tab, int entry, int lane) {
    constexpr int W = C::LDS_WORDS, B = C::BLOCK;
    const uint32_t* base = tab + (size_t)entry * (wave_table_words<C>() / WAVE_TABLE) + lane;
    [[maybe_unused]] uint32_t x[W], y[W], z[W], t[W];
#pragma unroll
    for (int i = 0; i < W; i++) {
        x[i] = base[(0 + i) * B];
        y[i] = base[(W + i) * B];
        z[i] = base[(2 * W + i) * B];
        if constexpr (C::EXTENDED) t[i] = base[(3 * W + i) * B];
    }
    typename C::Point p;
    p.x = C::from_lds(x); p.y = C::from_lds(y); p.z = C::from_lds(z);
    if constexpr (C::EXTENDED) p.t = C::from_lds(t);
    return p;
}
template <class C>
DR_DEV typename C::Point wave_shfl_down(const typename C::Point& p, unsigned delta) {
    typename C::Point o;
#pragma unroll
    for (int t = 0; t < (int)(sizeof(p.x.l) / sizeof(p.x.l[0])); t++) {
        o.x.l[t] = __shfl_down(p.x.l[t], delta, 64);
        o.y.l[t] = __shfl_down(p.y.l[t], delta, 64);
        o.z.l[t] = __shfl_down(p.z.l[t], delta, 64);
        if constexpr (C::EXTENDED) o.t.l[t] = __shfl_down(p.t.l[t], delta, 64);
    }
    return o;
}

// ---------------------------------------------------------------- scalar multiplication
// k P on a fixed schedule: table 1P..8P in LDS, WINDOWS signed 4-bit windows (wave_recode.hip.h) of a scalar of SCALAR_WORDS words —
// its 8 SCALAR_WORDS digits and, where WINDOWS is one more (an order of 256 bits; any k < 2^448), the carry out of the top digit as the
// last window; where it is fewer (64 for an order below 2^255, 131 for k < 2^521) the digits above are zero and no carry leaves —
// four doublings and one table addition each whatever the digits (the table index, always in range, is the only thing a digit decides:
// no branch and no loop bound depends on one) — the secret scalars of the provers go through here.  The fixed schedule is this window
// loop ALONE: the affine store that follows inverts Z by division steps, whose batch loop ends when g reaches 0 (divstep28.hip.h), so
// its batch count depends on Z, a value derived from the scalar.  The kernels are not fixed-time as a whole.
template <class C>
DR_DEV typename C::Point wave_scalar_mul_core(uint32_t* tab, int lane, const typename C::Point& P, const uint32_t (&k)[C::SCALAR_WORDS]) {
    using Point = typename C::Point;
    constexpr int DIGITS = 8 * C::SCALAR_WORDS;
    static_assert(C::WINDOWS <= DIGITS + 1, "a window is a digit of the recoding or the carry out of its top digit");
    wave_lds_store<C>(tab, 0, lane, P);
    Point Q = C::dbl(P);
    wave_lds_store<C>(tab, 1, lane, Q);
#pragma unroll 1
    for (int e = 2; e < WAVE_TABLE; e++) {
        Q = C::add(Q, P);
        wave_lds_store<C>(tab, e, lane, Q);
    }
    // wave_recode(k, dig), its loop over the words spelled here, and below wave_digit(dig, w) with its 8 taken off here: with either
    // behind a call of its own the compiler orders the kernels of the 256-bit curves another way
    uint32_t dig[C::SCALAR_WORDS];
    uint32_t carry = 0;
#pragma unroll
    for (int w = 0; w < C::SCALAR_WORDS; w++) dig[w] = wave_recode_word(k[w], carry);
    [[maybe_unused]] const uint32_t top_carry = carry;
    Point acc = C::identity();
#pragma unroll 1
    for (int w = C::WINDOWS - 1; w >= 0; w--) {
        if constexpr (C::EXTENDED) {             // three doublings whose T nothing reads, then one with T
#pragma unroll 1
            for (int j = 0; j < 3; j++) acc = C::dbl_no_t(acc);
            acc = C::dbl(acc);
        } else {
#pragma unroll 1
            for (int j = 0; j < 4; j++) acc = C::dbl(acc);
        }
        int dg;
        if constexpr (C::WINDOWS == DIGITS + 1) dg = w == DIGITS ? (int)top_carry : (int)wave_nibble(dig, w) - 8;
        else dg = (int)wave_nibble(dig, w) - 8;
        const int mag = dg < 0 ? -dg : dg;
        Point T = wave_lds_load<C>(tab, mag == 0 ? 0 : mag - 1, lane);
        T = C::cneg(T, dg < 0);
        if (mag == 0) T = C::identity();
        acc = C::add(acc, T);
    }
    return acc;
}

// out[i] = k[i] P[i].  pts: n x 2 WORDS words (x || y), ks: n x SCALAR_WORDS, out: n x 2 WORDS.  One lane per multiplication.
template <class C>
DR_DEV void wave_scalar_mul(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks, uint32_t* __restrict__ out, uint32_t n) {
    __shared__ uint32_t tab[wave_table_words<C>()];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * C::BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;            // keep the wave converged; the duplicate result is not stored
    uint32_t k[C::SCALAR_WORDS];
    const typename C::Point P = wave_load_term<C>(pts + (size_t)i * (2 * C::WORDS), ks + (size_t)i * C::SCALAR_WORDS, k);
    const typename C::Point acc = wave_scalar_mul_core<C>(tab, lane, P, k);
    if (live) wave_store_affine<C>(out + (size_t)i * (2 * C::WORDS), acc);
}

// out[g] = sum_{j<m} k[g m + j] P[g m + j]: one lane per term (m padded to mpad, a power of two <= 64), folded with shuffles by the
// unified / complete addition (terms that coincide or cancel need nothing special)
template <class C>
DR_DEV void wave_msm_groups(const uint32_t* __restrict__ pts, const uint32_t* __restrict__ ks, uint32_t* __restrict__ out,
                            uint32_t groups, uint32_t m, uint32_t mpad) {
    using Point = typename C::Point;
    __shared__ uint32_t tab[wave_table_words<C>()];
    const int lane = threadIdx.x;
    const uint32_t per_block = C::BLOCK / mpad;
    const uint32_t g = blockIdx.x * per_block + lane / mpad;
    const uint32_t j = lane % mpad;
    const bool live = g < groups && j < m;
    const size_t idx = live ? (size_t)g * m + j : 0;          // dead lanes recompute term 0 and are masked out
    uint32_t k[C::SCALAR_WORDS];
    const Point P = wave_load_term<C>(pts + idx * (2 * C::WORDS), ks + idx * C::SCALAR_WORDS, k);
    const Point r = wave_scalar_mul_core<C>(tab, lane, P, k);
    Point acc = live ? r : C::identity();
#pragma unroll 1
    for (uint32_t s = mpad >> 1; s > 0; s >>= 1) acc = C::add(acc, wave_shfl_down<C>(acc, s));
    if (g < groups && j == 0) wave_store_affine<C>(out + (size_t)g * (2 * C::WORDS), acc);
}

// ---------------------------------------------------------------- diagnostic of the law (dr_*_law_selftest)
// The description's law on RAW limb images, one lane per record: no packing, no inversion and no ABI conversion on either side, so a test
// sees the congruence AND the register form of everything the law returns, and can put every coordinate at the edge of the class the
// law documents.  pts: n records of P then Q, each x, y, z (and t when EXTENDED) of sizeof(Fe::l) / 4 int32 limbs; ctl: n control words;
// out: n x WAVE_LAW_SLOTS points in the same form.  The slots:
//   0  add(P, Q)                1  add(P, cneg(Q, true))       2  dbl(P)          3  dbl_no_t(P) (EXTENDED only; otherwise not written)
//   4  cneg(P, true)            5  slot 0 after wave_lds_store to entry WAVE_LAW_ENTRY and wave_lds_load back     6  cneg(P, false)
//   7 + w, w = 0..5             acc after window w of a chain run exactly as wave_scalar_mul_core runs one: four doublings (the first
//                               three dbl_no_t when EXTENDED), then add of the table term loaded from LDS entry WAVE_LAW_ENTRY (slot 0's
//                               point, stored once), negated when bit w of the control word is set and replaced by identity() when bit
//                               8 + w is; the chain starts at acc = P
// The table is the scalar multiplication's own (wave_table_words<C>()).  A lane past n recomputes record n - 1 and stores nothing.
constexpr int WAVE_LAW_SLOTS = 13, WAVE_LAW_WINDOWS = 6, WAVE_LAW_ENTRY = 3;
template <class C>
DR_DEV void wave_law_selftest(const int32_t* __restrict__ pts, const uint32_t* __restrict__ ctl, uint32_t n, int32_t* __restrict__ out) {
    using Point = typename C::Point;
    using Fe = typename C::Fe;
    constexpr int L = (int)(sizeof(Fe::l) / sizeof(int32_t)), NC = C::EXTENDED ? 4 : 3;
    __shared__ uint32_t tab[wave_table_words<C>()];
    const int lane = threadIdx.x;
    uint32_t i = blockIdx.x * C::BLOCK + lane;
    const bool live = i < n;
    if (!live) i = n - 1;            // keep the wave converged; the duplicate results are not stored
    auto load = [&](const int32_t* p) {
        Point r;
#pragma unroll
        for (int t = 0; t < L; t++) {
            r.x.l[t] = p[t]; r.y.l[t] = p[L + t]; r.z.l[t] = p[2 * L + t];
            if constexpr (C::EXTENDED) r.t.l[t] = p[3 * L + t];
        }
        return r;
    };
    int32_t* const o = out + (size_t)i * (WAVE_LAW_SLOTS * NC * L);
    auto put = [&](int slot, const Point& r) {
        if (!live) return;
        int32_t* q = o + slot * (NC * L);
#pragma unroll
        for (int t = 0; t < L; t++) {
            q[t] = r.x.l[t]; q[L + t] = r.y.l[t]; q[2 * L + t] = r.z.l[t];
            if constexpr (C::EXTENDED) q[3 * L + t] = r.t.l[t];
        }
    };
    const Point P = load(pts + (size_t)i * (2 * NC * L)), Q = load(pts + (size_t)i * (2 * NC * L) + NC * L);
    const uint32_t cw = ctl[i];
#pragma unroll 1
    for (int s = 0; s < 2; s++) {
        const Point R = C::add(P, C::cneg(Q, s != 0));
        put(s, R);
        if (s == 0) wave_lds_store<C>(tab, WAVE_LAW_ENTRY, lane, R);
    }
    put(2, C::dbl(P));
    if constexpr (C::EXTENDED) put(3, C::dbl_no_t(P));
#pragma unroll 1
    for (int s = 0; s < 2; s++) put(s == 0 ? 4 : 6, C::cneg(P, s == 0));
    put(5, wave_lds_load<C>(tab, WAVE_LAW_ENTRY, lane));
    Point acc = P;
#pragma unroll 1
    for (int w = 0; w < WAVE_LAW_WINDOWS; w++) {
        if constexpr (C::EXTENDED) {
#pragma unroll 1
            for (int j = 0; j < 3; j++) acc = C::dbl_no_t(acc);
            acc = C::dbl(acc);
        } else {
#pragma unroll 1
            for (int j = 0; j < 4; j++) acc = C::dbl(acc);
        }
        Point T = wave_lds_load<C>(tab, WAVE_LAW_ENTRY, lane);
        T = C::cneg(T, ((cw >> w) & 1u) != 0);
        if (((cw >> (8 + w)) & 1u) != 0) T = C::identity();
        acc = C::add(acc, T);
        put(7 + w, acc);
    }
}

// ---------------------------------------------------------------- SEC1 compressed points
// x = bytes 1..4 W of a (4 W + 1)-byte string (W + 1 words, the last three bytes zero; W = 8: 33 bytes, W = 12: 49) read BIG-endian:
// little-endian word q is the byte swap of the (unaligned) word at byte 4 W - 3 - 4 q
template <int W>
DR_DEV void sec1_x_words(const uint32_t (&w)[W + 1], uint32_t (&xb)[W]) {
#pragma unroll
    for (int q = 0; q < W; q++) {
        const int k = W - 1 - q;
        xb[q] = __builtin_bswap32((w[k] >> 8) | (w[k + 1] << 24));
    }
}
// One lane per SEC1 compressed encoding (33 or 49 bytes) padded to WORDS + 1 words: byte 0 is 0x02 or 0x03, x < p, the curve equation
// has a root, y the root of byte 0's parity (y = 0 cannot happen: the group orders are odd).  With CHECK the point must also pass the
// description's in_subgroup (curves with a cofactor; the point is computed either way, so the wave stays converged).  out = x || y and
// ok = 1, or zero bytes and ok = 0.
template <class C, bool CHECK = false>
DR_DEV void sec1_decode(const uint32_t* __restrict__ enc /* n*(WORDS+1) */, uint32_t* __restrict__ out_xy /* n*2*WORDS */,
                        uint32_t* __restrict__ ok, uint32_t n) {
    constexpr int W = C::WORDS;
    uint32_t i = blockIdx.x * C::BLOCK + threadIdx.x;
    const bool live = i < n;
    if (!live) i = n - 1;
    uint32_t w[W + 1];
#pragma unroll
    for (int j = 0; j < W + 1; j++) w[j] = enc[(size_t)i * (W + 1) + j];
    const uint32_t first = w[0] & 0xffu;
    uint32_t xb[W];
    sec1_x_words<W>(w, xb);
    const typename C::Fe x = C::unpack(xb);
    typename C::Fe y;
    const bool root = C::y_of_x(x, y);
    bool valid = (first == 0x02u || first == 0x03u) && C::below_p(xb) && root;
    if (C::is_odd(y) != ((first & 1u) != 0)) y = neg(y);
    if constexpr (CHECK) valid = C::in_subgroup(x, y) && valid;
    if (live) {
        if (valid) {
            wave_store_words(out_xy + (size_t)i * (2 * W), xb);
            wave_store_fe<C>(out_xy + (size_t)i * (2 * W) + W, y);
        } else {
            wave_store_zero_words<W>(out_xy + (size_t)i * (2 * W));
            wave_store_zero_words<W>(out_xy + (size_t)i * (2 * W) + W);
        }
        ok[i] = valid ? 1u : 0u;
    }
}

}  // namespace dr
