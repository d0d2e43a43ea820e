// RFC 9380 section 5 on the host, once for every suite: expand_message_xmd, expand_message_xof, and the reductions of the wide fields
// (BLS12-381's Fq from 64 bytes, Ed448's field from 84, P-521's from 98, P-384's from 72).  Plain C++: tests/native/h2c_hash_check.cpp builds it without the HIP toolchain.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

#include "hosthash.hpp"
#include "hostmath.hpp"

namespace drh {

// expand_message_xmd (section 5.3.1) over the hash H with digests of DIGEST bytes and a Z_pad of BLOCK bytes: L bytes (L <= 255 DIGEST)
// to `out` from prefix || msg under the tag `dst` (DST_prime = dst || len(dst) is formed here).  The prefix is a salt in front of the
// message; empty parts have no buffer to read.
template <class H, size_t BLOCK, size_t DIGEST>
inline void expand_message_xmd(const void* dst, size_t dst_len, const uint8_t* prefix, size_t prefix_len, const uint8_t* msg, size_t len, size_t L,
                               uint8_t* out) {
    const uint8_t zpad[BLOCK] = {0}, dl = (uint8_t)dst_len, lb[3] = {(uint8_t)(L >> 8), (uint8_t)L, 0};
    uint8_t b0[DIGEST], prev[DIGEST];
    H h;
    h.update(zpad, BLOCK);
    if (prefix_len) h.update(prefix, prefix_len);
    if (len) h.update(msg, len);
    h.update(lb, 3);
    h.update(dst, dst_len);
    h.update(&dl, 1);
    h.final(b0);
    for (size_t i = 1; DIGEST * (i - 1) < L; i++) {
        H g;
        uint8_t x[DIGEST];
        for (size_t j = 0; j < DIGEST; j++) x[j] = i == 1 ? b0[j] : (uint8_t)(b0[j] ^ prev[j]);
        g.update(x, DIGEST);
        const uint8_t ib = (uint8_t)i;
        g.update(&ib, 1);
        g.update(dst, dst_len);
        g.update(&dl, 1);
        g.final(prev);
        const size_t at = DIGEST * (i - 1);
        std::memcpy(out + at, prev, L - at < DIGEST ? L - at : DIGEST);
    }
}
// expand_message_xof (section 5.3.3) over SHAKE256: L bytes to `out`
inline void expand_message_xof(const void* dst, size_t dst_len, const uint8_t* prefix, size_t prefix_len, const uint8_t* msg, size_t len, size_t L,
                               uint8_t* out) {
    const uint8_t lb[2] = {(uint8_t)(L >> 8), (uint8_t)L}, dl = (uint8_t)dst_len;
    Shake256 h;
    if (prefix_len) h.update(prefix, prefix_len);
    if (len) h.update(msg, len);
    h.update(lb, 2);
    h.update(dst, dst_len);
    h.update(&dl, 1);
    h.digest(out, L);
}

// 64 big-endian bytes mod BLS12-381's p -> 48 bytes little-endian: hi 2^384 + lo with both halves taken as raw 384-bit values (a
// Montgomery product with R^2 accepts any operand below 2^384), 2^384 mod p being R^2's own Montgomery image
inline void fq_reduce_be64(const uint8_t* in, uint8_t* out) {
    Fq lo = Fq::zero(), hi = Fq::zero(), r;
    for (int i = 0; i < 48; i++) lo.l[i / 8] |= (uint64_t)in[63 - i] << (8 * (i % 8));
    for (int i = 0; i < 16; i++) hi.l[i / 8] |= (uint64_t)in[15 - i] << (8 * (i % 8));
    std::memcpy(r.l, FieldParams<6>::R2, sizeof r.l);
    (lo.to_mont() + hi.to_mont() * r).store_le(out);
}

// Ed448's p = 2^448 - 2^224 - 1 as seven 64-bit words: all ones but bit 224 (word 3, bit 32)
constexpr uint64_t P448[7] = {~0ull, ~0ull, ~0ull, 0xfffffffeffffffffull, ~0ull, ~0ull, ~0ull};
// 84 big-endian bytes (672 bits) mod p -> 56 bytes little-endian: hi 2^448 + lo = lo + hi + hi 2^224 (hi of 224 bits), a value below
// 2^449 + 2^225, less p while it is not below p (at most three times)
inline void fe_reduce_be84(const uint8_t* in, uint8_t* out) {
    uint8_t le[88] = {0};
    for (size_t i = 0; i < 84; i++) le[i] = in[83 - i];
    uint64_t lo[8] = {0}, hi[8] = {0}, hs[8] = {0}, v[8];
    std::memcpy(lo, le, 56);
    std::memcpy(hi, le + 56, 28);
    std::memcpy(reinterpret_cast<uint8_t*>(hs) + 28, le + 56, 28);      // hi << 224
    unsigned __int128 c = 0;
    for (int i = 0; i < 8; i++) {
        c += (unsigned __int128)lo[i] + hi[i] + hs[i];
        v[i] = (uint64_t)c;
        c >>= 64;
    }
    for (int pass = 0; pass < 3; pass++) {
        uint64_t d[8], borrow = 0;
        for (int i = 0; i < 8; i++) {
            const unsigned __int128 t = (unsigned __int128)v[i] - (i < 7 ? P448[i] : 0) - borrow;
            d[i] = (uint64_t)t;
            borrow = (uint64_t)(t >> 64) & 1;
        }
        if (!borrow) std::memcpy(v, d, sizeof d);
    }
    std::memcpy(out, v, 56);
}

// 98 big-endian bytes (784 bits) mod P-521's p = 2^521 - 1 -> 68 bytes little-endian.  2^521 = 1: the value is lo + hi with lo its low
// 521 bits and hi the 263 above; the sum is below 2^521 + 2^263, so folding its bit 521 once more leaves a value <= p, and p itself is 0
inline void fp521_reduce_be98(const uint8_t* in, uint8_t* out) {
    uint8_t le[112] = {0};
    for (size_t i = 0; i < 98; i++) le[i] = in[97 - i];
    uint64_t v[14], s[9];
    std::memcpy(v, le, sizeof v);
    unsigned __int128 c = 0;
    for (int i = 0; i < 9; i++) {
        const uint64_t lo = i < 8 ? v[i] : v[8] & 0x1ffull;
        const uint64_t hi = i + 9 < 14 ? (v[i + 8] >> 9) | (v[i + 9] << 55) : 0;      // (v >> 521), words 0..4 non-zero
        c += (unsigned __int128)lo + hi;
        s[i] = (uint64_t)c;
        c >>= 64;
    }
    uint64_t carry = s[8] >> 9;                          // bit 521
    s[8] &= 0x1ffull;
    for (int i = 0; i < 9 && carry; i++) {
        s[i] += carry;
        carry = s[i] == 0 ? 1 : 0;
    }
    bool is_p = s[8] == 0x1ffull;
    for (int i = 0; i < 8; i++) is_p = is_p && s[i] == ~0ull;
    if (is_p) std::memset(s, 0, sizeof s);
    std::memcpy(out, s, 68);
}

// 72 big-endian bytes (576 bits) mod P-384's p = 2^384 - 2^128 - 2^96 + 2^32 - 1 -> 48 bytes little-endian.  2^384 = 2^128 + 2^96 - 2^32 + 1:
// with hi the 192 bits above lo's 384, the value is lo + hi + (hi << 96) + (hi << 128) - (hi << 32), every shift a whole number of 32-bit
// words; the sum is not negative and below 2^384 + 2^321 < 2 p, so p comes off at most once (the loop allows twice)
inline void fp384_reduce_be72(const uint8_t* in, uint8_t* out) {
    static const uint32_t PW[12] = {0xffffffffu, 0, 0, 0xffffffffu, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu, 0xffffffffu,
                                    0xffffffffu, 0xffffffffu};
    uint32_t w[18];
    for (int j = 0; j < 18; j++) {
        const uint8_t* q = in + 68 - 4 * j;
        w[j] = (uint32_t)q[3] | (uint32_t)q[2] << 8 | (uint32_t)q[1] << 16 | (uint32_t)q[0] << 24;
    }
    const uint32_t* hi = w + 12;
    uint32_t v[13];
    int64_t c = 0;
    for (int j = 0; j < 13; j++) {
        int64_t t = c + (j < 12 ? w[j] : 0);
        if (j < 6) t += hi[j];
        if (j >= 3 && j < 9) t += hi[j - 3];
        if (j >= 4 && j < 10) t += hi[j - 4];
        if (j >= 1 && j < 7) t -= hi[j - 1];
        v[j] = (uint32_t)t;
        c = t >> 32;
    }
    for (int pass = 0; pass < 2; pass++) {
        uint32_t d[13];
        int64_t borrow = 0;
        for (int j = 0; j < 13; j++) {
            const int64_t t = (int64_t)v[j] - (j < 12 ? PW[j] : 0) + borrow;
            d[j] = (uint32_t)t;
            borrow = t >> 32;
        }
        if (borrow == 0) std::memcpy(v, d, sizeof d);
    }
    std::memcpy(out, v, 48);
}

// hash_to_field of the BLS12-381 suites: expand_message_xmd over SHA-256 to `chunks` x 64 bytes (at most 4), each big-endian mod p;
// out = chunks x 48 bytes little-endian.  G1 asks for one chunk per element, G2 for two (c0 || c1).
inline void hash_to_field_fq(const void* dst, size_t dst_len, unsigned chunks, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len,
                             uint8_t* out) {
    uint8_t raw[256];
    expand_message_xmd<Sha256, 64, 32>(dst, dst_len, salt, salt_len, msg, len, 64 * (size_t)chunks, raw);
    for (unsigned k = 0; k < chunks; k++) fq_reduce_be64(raw + 64 * k, out + 48 * k);
}
// hash_to_field of the Ed448 suites: expand_message_xof to count x 84 bytes (at most 2); out = count x 56 bytes little-endian
inline void hash_to_field_fe448(const void* dst, size_t dst_len, unsigned count, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len,
                                uint8_t* out) {
    uint8_t raw[168];
    expand_message_xof(dst, dst_len, salt, salt_len, msg, len, 84 * (size_t)count, raw);
    for (unsigned k = 0; k < count; k++) fe_reduce_be84(raw + 84 * k, out + 56 * k);
}
// hash_to_field of the P-521 suites: expand_message_xmd over SHA-512 to count x 98 bytes (at most 2); out = count x 68 bytes little-endian
inline void hash_to_field_fp521(const void* dst, size_t dst_len, unsigned count, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len,
                                uint8_t* out) {
    uint8_t raw[196];
    expand_message_xmd<Sha512, 128, 64>(dst, dst_len, salt, salt_len, msg, len, 98 * (size_t)count, raw);
    for (unsigned k = 0; k < count; k++) fp521_reduce_be98(raw + 98 * k, out + 68 * k);
}

// hash_to_field of the P-384 suites: expand_message_xmd over SHA-384 to count x 72 bytes (at most 2); out = count x 48 bytes little-endian
inline void hash_to_field_fp384(const void* dst, size_t dst_len, unsigned count, const uint8_t* salt, size_t salt_len, const uint8_t* msg, size_t len,
                                uint8_t* out) {
    uint8_t raw[144];
    expand_message_xmd<Sha384, 128, 48>(dst, dst_len, salt, salt_len, msg, len, 72 * (size_t)count, raw);
    for (unsigned k = 0; k < count; k++) fp384_reduce_be72(raw + 72 * k, out + 48 * k);
}

}  // namespace drh
