/*
 * dotring_hip.h — C ABI of libdotring_hip.so: the MI355X (gfx950) replacement for the native arithmetic on
 * dot-ring's Ring-VRF prove/verify hot path.  Plain pointers and sizes only; no torch types.
 *
 * Conventions
 *   - every function returns 0 on success or a negative dr_status; dr_last_error() gives the text
 *     (thread-local).  The Python shim maps DR_ERR_INVALID -> ValueError, DR_ERR_NOMEM -> MemoryError,
 *     the same exception types the reference raises at these seams.
 *   - the caller owns every buffer; the library keeps no caller pointer after return.  Handles made by
 *     *_create / *_load are freed by *_destroy.  A dr_ctx is bound to one GPU and one HIP stream; calls on
 *     one ctx are synchronous (results are on the host when the call returns) and must not be issued
 *     concurrently from several threads; different ctx objects are independent.
 *   - Bandersnatch field elements / scalars: 32 bytes little-endian, standard form (as the reference's
 *     bls_scalar_from_bytes, dot_ring/curve/native_field/bls12_381_scalar.c:266).  A TE affine point is
 *     x(32) || y(32).
 *   - BLS12-381 G1 affine points: 96 bytes, big-endian x(48) || y(48) — the SRS file record
 *     (dot_ring/ring_proof/pcs/srs.py:61-70) and blst's serialize() format; all-zero coordinates or the
 *     0x40 flag in byte 0 denote infinity.  KZG scalars: 32 bytes little-endian, any value < 2^256.
 *   - *_dev variants take pointers into GPU memory obtained from dr_dev_alloc (same layouts) so that a
 *     pipeline — or a benchmark — can keep its operands resident in HBM.
 */
#ifndef DOTRING_HIP_H
#define DOTRING_HIP_H

#include <stddef.h>
#include <stdint.h>

#if defined(__GNUC__)
#define DR_API __attribute__((visibility("default")))
#else
#define DR_API
#endif

#ifdef __cplusplus
extern "C" {
#endif

typedef struct dr_ctx dr_ctx;
typedef struct dr_srs dr_srs;

enum dr_status {
    DR_OK = 0,
    DR_ERR_INVALID = -1,   /* bad length / encoding / argument  (reference: ValueError) */
    DR_ERR_NOMEM = -2,     /* host or device allocation failed  (reference: MemoryError) */
    DR_ERR_DEVICE = -3,    /* HIP runtime failure, no usable gfx950 device */
    DR_ERR_NOTSQUARE = -4  /* dr_fr_sqrt: input is a quadratic non-residue (reference: ValueError) */
};

/* ---- library / context ------------------------------------------------------------------------- */
DR_API const char *dr_version(void);
DR_API const char *dr_last_error(void);
DR_API int dr_device_count(void);
DR_API int dr_ctx_create(int device_id, dr_ctx **out);
DR_API void dr_ctx_destroy(dr_ctx *ctx);
DR_API int dr_ctx_sync(dr_ctx *ctx);

/* HBM buffers for the *_dev entry points */
DR_API int dr_dev_alloc(dr_ctx *ctx, size_t bytes, void **dptr);
DR_API int dr_dev_free(dr_ctx *ctx, void *dptr);
DR_API int dr_dev_upload(dr_ctx *ctx, void *dptr, const void *host, size_t bytes);
DR_API int dr_dev_download(dr_ctx *ctx, void *host, const void *dptr, size_t bytes);

/* Per-kernel timing with HIP events on the ctx stream (used by bench.py for the roofline line).
 * dr_prof_get: accumulated milliseconds and launch count of the kernel called `name` since the last reset. */
DR_API int dr_prof_enable(dr_ctx *ctx, int on);
DR_API int dr_prof_reset(dr_ctx *ctx);
DR_API int dr_prof_get(dr_ctx *ctx, const char *name, double *total_ms, int *launches);

/* ---- seam A: Bandersnatch kernels ---------------------------------------------------------------
 * Replaces dot_ring/curve/native_field/bandersnatch_te.pyx:
 *   scalar_mult_windowed_native_w2_cy :480 (+ GLV callers dot_ring/curve/glv.py:191, specs/bandersnatch.py:177)
 *   scalar_mult_4_native_w2_cy :557, scalar_mult_6_native_w2_cy :669, msm_pippenger_signed_native_cy :257
 *   sqrt_mod_bls_scalar_cy :421, projective_to_affine_cy :244
 * Outputs are canonical affine coordinates (the reference normalises its projective tuples immediately,
 * glv.py:243-248), so any internal windowing gives identical bytes.
 */

/* out[i] = scalars[i] * pts[i]  for i < n.  Scalars are taken mod the group order. */
DR_API int dr_bsn_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_xy /* n*64 */, const uint8_t *scalars /* n*32 */,
                            size_t n, uint8_t *out_xy /* n*64 */);
DR_API int dr_bsn_scalar_mul_batch_dev(dr_ctx *ctx, const void *d_pts_xy, const void *d_scalars, size_t n, void *d_out_xy);

/* out = sum_i scalars[i] * pts[i]   (n may be 0: identity (0,1)) */
DR_API int dr_bsn_msm(dr_ctx *ctx, const uint8_t *pts_xy, const uint8_t *scalars, size_t n, uint8_t out_xy[64]);

/* groups[g] = sum of `m` consecutive terms: out[g] = sum_{j<m} scalars[g*m+j] * pts[g*m+j], g < groups.
 * One launch for the many small fixed-arity MSMs of the sigma protocols (m = 2, 3, 4). */
DR_API int dr_bsn_msm_groups(dr_ctx *ctx, const uint8_t *pts_xy, const uint8_t *scalars, size_t groups, size_t m,
                      uint8_t *out_xy /* groups*64 */);

/* Elligator 2 hash-to-curve field work for n inputs: out[i] = clear_cofactor(map(u[2i]) + map(u[2i+1])), i.e.
 * TEAffinePoint._e2c_ell2_ro (dot_ring/curve/twisted_edwards/te_affine_point.py:212-295, te_curve.py:48-95) after
 * hash_to_field, which stays on the host.  u_pairs: n*2 canonical field elements (32-byte LE). */
DR_API int dr_bsn_encode_to_curve_batch(dr_ctx *ctx, const uint8_t *u_pairs, size_t n, uint8_t *out_xy);

/* dec_point for n compressed points (dot_ring/vrf/codec.py:39-45, curve/point.py:150-214, curve/curve.py:56-67):
 * decompression (y < p, x^2 = (1-y^2)/(a-d y^2), the sign bit picks the larger root) and validation (not the
 * identity, prime-order subgroup) on the GPU.  ok[i] = 1 for valid points; out_xy[i] is meaningful only then. */
DR_API int dr_bsn_decode_points(dr_ctx *ctx, const uint8_t *enc /* n*32 */, size_t n, uint8_t *out_xy /* n*64 */, uint8_t *ok /* n */);

/* The same four operations on any twisted Edwards curve over this base field the library knows:
 * DR_CURVE_BANDERSNATCH (a = -5, cofactor 4; identical to the dr_bsn_* calls) or DR_CURVE_JUBJUB (a = -1, cofactor 8,
 * dot_ring/curve/specs/jubjub.py:17-29 — no endomorphism, so the plain 64-window kernels).  The sigma-protocol and
 * ring entry points below take the curve from dr_vrf_suite.curve. */
enum { DR_CURVE_BANDERSNATCH = 0, DR_CURVE_JUBJUB = 1, DR_CURVE_BANDERSNATCH_SW = 2 };
/* DR_CURVE_BANDERSNATCH_SW: Bandersnatch in short Weierstrass form (dot_ring/curve/specs/bandersnatch_sw.py), the same prime-order group;
 * the kernels compute on its twisted Edwards image (Montgomery-model maps of dot_ring/ring_proof/ring_curve.py:10-23, on the device).
 * For this curve a raw point is SW affine x(32) || y(32) little-endian, the identity 64 zero bytes; an encoded point is 33 bytes,
 * x(32) LE then a flag byte (0x80: y is the larger of +-y; dec rejects 0x40 = infinity, any of the low six bits, x >= p, no y, y = 0,
 * points outside the prime-order subgroup), so dr_te_decode_points reads n*33 bytes.  Accepted by the four calls above and below,
 * dr_te_fixed_base_msm_groups (curve 2 outside these calls' size limits is refused, never read as TE), dr_encode_to_curve_batch
 * (try-and-increment, bandersnatch_sw.py + point.py:252-296), dr_ietf_prove_batch, dr_pedersen_prove_batch and dr_pedersen_verify_batch
 * (proofs 81 / 98 / 196 bytes; inside them points stay TE and are mapped to SW only to be encoded).  The ring prover, the Ring-VRF
 * calls and dr_ietf_verify_batch refuse it (DR_ERR_INVALID). */
/* DR_CURVE_ED25519: Ed25519 (dot_ring/curve/specs/ed25519.py, the Ed25519_TAI variant: a = -1, cofactor 8, n = l, try-and-increment with
 * SHA-512), over GF(2^255 - 19) — its own kernels (csrc/kernels_ed25519.hip.h, field csrc/fe25519.hip.h).  Raw points are x || y
 * little-endian, coordinates below 2^255 - 19; encodings are 32 bytes, y with bit 255 = (x > p - x), the reference's sign rule (not
 * RFC 8032's parity).  Scalars are reduced mod l on the device (sound for points of the prime-order subgroup).  Accepted by
 * dr_te_scalar_mul_batch, dr_te_msm, dr_te_msm_groups, dr_te_decode_points (canonical y, a root, not the identity, no torsion
 * component), dr_te_fixed_base_msm_groups (through the variable-base grouped kernel: no window table), dr_encode_to_curve_batch,
 * dr_ietf_prove_batch, dr_pedersen_prove_batch and dr_pedersen_verify_batch (proofs 80 / 96 / 192 bytes).  Every call runs on the
 * kernels (no host route).  The ring prover, the Ring-VRF calls, dr_ietf_verify_batch and the dr_bsn_* calls refuse it. */
enum { DR_CURVE_ED25519 = 3 };
/* DR_CURVE_P256: P-256 (dot_ring/curve/specs/p256.py, the P256_TAI variant: y^2 = x^3 - 3 x + b, cofactor 1, n of 256 bits,
 * try-and-increment with SHA-256) over its own field — its own kernels (csrc/kernels_p256.hip.h, field csrc/fp256.hip.h).  Raw points
 * are affine x || y little-endian, coordinates below p; 64 zero bytes are the identity ((0, 0) is not on the curve).  Encodings are 33
 * bytes: x little-endian, then a flag byte (bit 7: y > p - y, bit 6: infinity); a string that starts with 0x02 / 0x03 and does not
 * decode so is decoded as SEC1 compressed (x = its bytes 1..32 big-endian), as the reference does.  Scalars are reduced mod n on the
 * device.  Accepted by dr_te_scalar_mul_batch, dr_te_msm, dr_te_msm_groups, dr_te_decode_points (decoded and not the identity),
 * dr_te_fixed_base_msm_groups (through the variable-base grouped kernel), dr_encode_to_curve_batch, dr_ietf_prove_batch,
 * dr_pedersen_prove_batch and dr_pedersen_verify_batch (proofs 81 / 98 / 196 bytes; the suite's xof is 2).  Every call runs on the
 * kernels.  The ring prover, the Ring-VRF calls, dr_ietf_verify_batch, dr_hash_to_field_batch and the dr_bsn_* calls refuse it. */
enum { DR_CURVE_P256 = 4 };
/* DR_CURVE_BABYJUBJUB: Baby JubJub (dot_ring/curve/specs/baby_jubjub.py: a = 1, cofactor 8, n = l of 251 bits, try-and-increment with
 * SHA-512), over the BN254 scalar field (254 bits) — its own kernels (csrc/kernels_bjj.hip.h, field csrc/fbn254.hip.h).  Raw points are
 * x || y little-endian, coordinates below p; encodings are 32 bytes, y with bit 255 = (x > p - x); y >= p (so any encoding with bit 254
 * set) is rejected.  Try-and-increment candidates have bit 254 cleared and the sign bit kept, as the reference masks them.  Scalars are
 * reduced mod l on the device.  Accepted by dr_te_scalar_mul_batch, dr_te_msm, dr_te_msm_groups, dr_te_decode_points (canonical y, a
 * root, not the identity, no torsion component), dr_te_fixed_base_msm_groups (through the variable-base grouped kernel),
 * dr_encode_to_curve_batch, dr_ietf_prove_batch, dr_pedersen_prove_batch and dr_pedersen_verify_batch (proofs 80 / 96 / 192 bytes).
 * Every call runs on the kernels (no host route).  The ring prover, the Ring-VRF calls, dr_ietf_verify_batch and the dr_bsn_* calls
 * refuse it. */
enum { DR_CURVE_BABYJUBJUB = 5 };
/* DR_CURVE_SECP256K1 (the reference's Secp256k1 = Secp256k1_RO) and DR_CURVE_SECP256K1_NU (Secp256k1_NU): secp256k1
 * (dot_ring/curve/specs/secp256k1.py: y^2 = x^3 + 7, cofactor 1, n of 256 bits) over its own field 2^256 - 2^32 - 977 — its own kernels
 * (csrc/kernels_secp256k1.hip.h, field csrc/fsecp256k1.hip.h).  The two ids differ only in how they hash to the curve (RFC 9380,
 * secp256k1_XMD:SHA-256_SSWU_RO_: two field elements and the sum of their images; ..._NU_: one), and they share one suite id, which is
 * why the variant is part of the curve id.  Raw points are affine x || y little-endian, coordinates below p, 64 zero bytes for the
 * identity; encodings are 33 bytes, plain SEC1 compressed: 0x02 / 0x03 by the parity of y, then x BIG-endian (no string encodes the
 * identity).  Scalars are reduced mod n on the device.  Accepted by the same entry points as DR_CURVE_P256 (dr_te_decode_points: prefix,
 * x below p, a root); dr_vrf_suite.xof must be 2.  The ring prover, the Ring-VRF calls, dr_ietf_verify_batch, the GLV and dr_bsn_*
 * entry points refuse them. */
enum { DR_CURVE_SECP256K1 = 6, DR_CURVE_SECP256K1_NU = 7 };
/* The RFC 9380 variants of P-256 and Ed25519 (the reference's P256_RO / P256_NU and Ed25519_RO / Ed25519_NU): the groups, kernels,
 * raw point form and scalar handling of DR_CURVE_P256 and DR_CURVE_ED25519, hashing to the curve by a map kernel in place of
 * try-and-increment (RO: two field elements and the sum of their images; NU: one).  Each shares its suite id with the
 * try-and-increment variant, which is why the variant is part of the curve id.
 *   DR_CURVE_P256_RO / _NU     P256_XMD:SHA-256_SSWU_RO_ / _NU_: the simplified SWU map straight onto the curve (csrc/sswu.hip.h, the
 *                              template k_secp256k1_map_to_curve is the other instance of); dr_vrf_suite.xof must be 2.  Encodings are
 *                              33 bytes, plain SEC1 compressed as DR_CURVE_SECP256K1's — NOT DR_CURVE_P256's little-endian x and flag
 *                              byte: dr_te_decode_points reads 0x02 / 0x03, x big-endian below p, a root, and nothing else.
 *   DR_CURVE_ED25519_RO / _NU  edwards25519_XMD:SHA-512_ELL2_RO_ / _NU_: Elligator 2 onto curve25519, the reference's mont_to_ed25519,
 *                              the cofactor cleared; dr_vrf_suite.xof must be 0.  Encodings are DR_CURVE_ED25519's.
 * The ring prover, the Ring-VRF calls, dr_ietf_verify_batch, the GLV and dr_bsn_* entry points refuse them, as they refuse ids 3, 4, 6, 7. */
enum { DR_CURVE_P256_RO = 8, DR_CURVE_P256_NU = 9, DR_CURVE_ED25519_RO = 10, DR_CURVE_ED25519_NU = 11 };
/* Curve25519_RO / Curve25519_NU (the reference's specs/curve25519.py): v^2 = u^3 + 486662 u^2 + u over GF(2^255 - 19), the group of
 * DR_CURVE_ED25519 in Montgomery form.  Raw points are u || v, 32 little-endian bytes each, and the ENCODING of a point is those same 64
 * bytes (dr_vrf_suite: point length 64, challenge length 16, xof 0; suite id curve25519_XMD:SHA-512_ELL2_RO_ for both variants, the DST
 * of the maps QUUX-V01-CS02-with- || suite id with _RO_ replaced by _NU_ for the nonuniform one).  The kernels (csrc/kernels_curve25519.hip.h)
 * compute on the Ed25519 group law through x = c u / v, y = (u - 1) / (u + 1), c = sqrt(-486664), converting at both ends of each launch.
 *
 * THE IDENTITY.  (0, 0) is a point of this curve (the one of order 2), so 64 zero bytes do NOT stand for the identity here, as they do
 * on the Weierstrass curves.  The identity is carried beside the point:
 *   - the dr_curve25519_* entry points below take and give one FLAG BYTE per point: 0 = the 64 bytes are the point, 1 = the point is the
 *     identity (its 64 bytes are ignored on input and zero on output).  The kernels' form of the same flag is one 32-bit word per point.
 *   - the generic dr_te_* entry points and the dr_*_prove_batch / verify calls, whose points are 64 bytes and nothing else, write the
 *     identity of these two curve ids as 64 bytes of 0xff: u = v = 2^256 - 1 is no field element, so it is no point.
 * A proof whose point would be the identity has no encoding (the reference's point_to_string raises): the provers return DR_ERR_INVALID.
 * The ring prover, the Ring-VRF calls, dr_ietf_verify_batch, the GLV and dr_bsn_* entry points refuse these ids, as they refuse 3 - 11.
 * Id 12 is not assigned (every entry point answers DR_ERR_INVALID to it).
 *
 * dr_te_msm on ids 3 - 11, 13 and 14 (the curves with kernels of their own): up to 256 terms it is dr_te_msm_groups' kernel over chunks of
 * 64 and once more over the partial sums, a fixed schedule per term; from 257 terms on the bucket method (csrc/wave_msm.hip.h), which is
 * NOT a fixed schedule — bucket choice and list lengths depend on the scalars, as on Bandersnatch from 256 terms.  The result is the same
 * sum of (k_i mod n) P_i.  Secret scalars belong in dr_te_scalar_mul_batch and dr_te_msm_groups. */
enum { DR_CURVE_CURVE25519_RO = 13, DR_CURVE_CURVE25519_NU = 14 };
DR_API int dr_te_scalar_mul_batch(dr_ctx *ctx, int curve, const uint8_t *pts_xy, const uint8_t *scalars, size_t n, uint8_t *out_xy);
DR_API int dr_te_msm(dr_ctx *ctx, int curve, const uint8_t *pts_xy, const uint8_t *scalars, size_t n, uint8_t out_xy[64]);
DR_API int dr_te_msm_groups(dr_ctx *ctx, int curve, const uint8_t *pts_xy, const uint8_t *scalars, size_t groups, size_t m, uint8_t *out_xy);
DR_API int dr_te_decode_points(dr_ctx *ctx, int curve, const uint8_t *enc, size_t n, uint8_t *out_xy, uint8_t *ok);

/* Fixed-base multiplication for CONSTANT points — the generator G and the Pedersen blinding base B of the sigma protocols
 * (dot_ring/vrf/pedersen/vrf.py:94,104,111: x*G + b*B, k*G + k_b*B; curve.py:384 pk = sk*G):
 * out[g] = sum_{j<m} scalars[g*m+j] * bases[j], m <= 4.  The first call with a base builds its window table in HBM
 * (every multiple (e+1)*16^w*P, 48 KB, cached in the context); a multiplication is then 64 table additions and no doubling,
 * spread over four lanes.  Results are the canonical affine points, as dr_bsn_msm_groups gives them. */
DR_API int dr_te_fixed_base_msm_groups(dr_ctx *ctx, int curve, const uint8_t *bases_xy /* m*64 */, size_t m,
                                       const uint8_t *scalars /* groups*m*32 */, size_t groups, uint8_t *out_xy /* groups*64 */);

/* Diagnostic: the device's field arithmetic on the base field of the twisted Edwards curves (the 9 x 29-bit representation of
 * csrc/fr29.hip.h that every kernel of this seam computes in), one lane per pair of canonical little-endian elements.
 * out: n x 12 x 32 bytes — a b, a^2, a + b, a - b, a^-1 (0 for 0), (a + b)(a - b), -5 a, 2 a b (fused product), sqrt(a) or 0;
 * then, each times 2^261 (the form the kernels compute in): a b + a, a + 27 b, a - 28 b through the lazy-sum helpers of the NTT /
 * polynomial kernels (canon29_small, reduce_small).  is_square[i] = 1 iff a[i] is a square.  The reference has no counterpart: its field is Python / C big integers
 * (dot_ring/curve/native_field/scalar.pyx); the tests check this entry point against the same integers. */
DR_API int dr_fr_ops_selftest(dr_ctx *ctx, const uint8_t *a /* n*32 */, const uint8_t *b /* n*32 */, size_t n, uint8_t *out /* n*384 */,
                              uint8_t *is_square /* n */);

/* Diagnostic: csrc/fr29.hip.h and the addition chains of csrc/curve.hip.h on RAW limb images: no packing and no conversion on the way
 * in, so a test can put every operand at the bound its header documents and read the limbs of what comes back.  images[i] = four
 * images a, b, c, d of nine signed 32-bit limbs each; every operation runs on every record.  out[i] = 150 words:
 *   13 x 9 limbs   mul(a, b), sqr(a), mul2(a, b, c, d), carry(a), carry_u(a), sub_3p(carry_u(a)), reduce_small(a), unpack(pack(a)),
 *                  inv(a), te_aA(a) and te_b_minus_aA(a, b) for Bandersnatch, the same two for JubJub
 *   4 x 8 words    canon29(a), canon29_small(a), fs_to_std(a), to_mont256(a)
 *   1 word         bit 0 is_zero(a), bit 1 equal(a, b)
 * n = 0 returns at once; a null buffer and n >= 2^24 are refused.  The call launches under no profiled name. */
DR_API int dr_fr_raw_selftest(dr_ctx *ctx, const int32_t *images /* n*4*9 */, size_t n, uint32_t *out /* n*150 */);

/* Diagnostic: the twisted Edwards law of csrc/curve.hip.h (te_add, te_dbl, te_cneg) and te_madd on RAW limb images, for
 * DR_CURVE_BANDERSNATCH and DR_CURVE_JUBJUB (any other id is refused), in the manner of the dr_*_law_selftest calls below.
 * records[i] = P then Q (x, y, z, t of nine signed 32-bit limbs each), then one table row (x2, y2, d x2 y2) as the bucket walk hands it
 * to te_madd: 11 x 9 limbs; controls[i] = one word; out[i] = 17 points (x, y, z, t):
 *   0 te_add(P, Q)   1 te_add(P, -Q)   2 te_dbl<true>(P)   3 te_dbl<false>(P) (T = 0)   4 te_cneg(P, true)   6 te_cneg(P, false)
 *   5 slot 0 through the LDS table of the scalar multiplication (lds_store_point, lds_load_point) and back
 *   7 + w, w < 6: the accumulator after window w of the fixed schedule started at P: three te_dbl<false>, one te_dbl<true>, then the
 *   table term (slot 0's point, from LDS) added, negated if bit w of the control word is set, the identity if bit 8 + w is
 *   13 te_madd(P, row)   14 te_madd four times from the identity with the same row; bit 16 of the control word negates the row's x and
 *   d x2 y2 limb-wise first   15 te_add(slot 0, slot 2)   16 the GLV endomorphism of (x2, y2) as given (Bandersnatch; not written otherwise)
 * n = 0 returns at once; a null buffer and n >= 2^24 are refused.  The call launches under no profiled name. */
DR_API int dr_te_law_selftest(dr_ctx *ctx, int curve, const int32_t *records /* n*11*9 */, const uint32_t *controls /* n */, size_t n,
                              int32_t *out /* n*17*4*9 */);

/* Ed25519 point decoding with the prime-order check (check = 1: as dr_te_decode_points for DR_CURVE_ED25519) or the codec alone
 * (check = 0: y < p and a root; (0, 1) and (0, p - 1) decode whatever the sign bit, as the reference's constructor takes them).
 * ok[i] = 1 when accepted; out_xy[i] is then x || y, otherwise 64 zero bytes. */
DR_API int dr_ed25519_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*32 */, size_t n, uint8_t *out_xy /* n*64 */, uint8_t *ok /* n */);
/* Diagnostic: the device's arithmetic in GF(2^255 - 19) (csrc/fe25519.hip.h) on RAW limb images — a and b are 9 signed 32-bit limbs
 * each (value sum l[i] 2^(29 i)), so that every operation can be driven at the limb bounds of its contract.  out: n x 11 x 32 bytes
 * of canonical little-endian results: a b, a^2, a + b, a - b, -a, carry(a), a b + b a (fused), a^-1 (0 for 0), sqrt(a) or 0, a,
 * sqrt(a / b) or 0.  flags[i]: bit 0 a is a square, bit 1 a / b is a square, bit 2 a > p - a. */
DR_API int dr_fe25519_ops_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*9 */, const int32_t *b_limbs /* n*9 */, size_t n,
                                   uint8_t *out /* n*352 */, uint8_t *flags /* n */);
/* P-256 point decoding: check = 1 as dr_te_decode_points for DR_CURVE_P256, check = 0 the codec alone (the identity's encoding,
 * 32 zero bytes and 0x40, is then accepted with out_xy = 64 zero bytes).  enc: n x 33 bytes; ok[i] = 1 when accepted. */
DR_API int dr_p256_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*33 */, size_t n, uint8_t *out_xy /* n*64 */, uint8_t *ok /* n */);
/* Diagnostic: the device's arithmetic in GF(p256) (csrc/fp256.hip.h) on RAW limb images — 9 signed 32-bit limbs each, value
 * sum l[i] 2^(29 i), standing for value * 2^-261 mod p (Montgomery form).  out: n x 12 x 32 bytes of canonical little-endian results:
 * a b, a^2, a + b, a - b, -a, carry(a), a b + b a (fused), a^-1 (0 for 0), sqrt(a) or 0, a, reduce(a), reduce(a)^2.  flags[i]: bit 0 a is a
 * square, bit 1 a > p - a, bit 2 a is odd. */
DR_API int dr_p256_field_ops_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*9 */, const int32_t *b_limbs /* n*9 */, size_t n,
                                      uint8_t *out /* n*384 */, uint8_t *flags /* n */);
/* secp256k1 point decoding (SEC1 compressed, 33 bytes): check = 1 as dr_te_decode_points for DR_CURVE_SECP256K1, check = 0 the codec
 * alone — the same strings, since none encodes the identity.  ok[i] = 1 when accepted; out_xy[i] is then x || y, otherwise 64 zero bytes. */
DR_API int dr_secp256k1_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*33 */, size_t n, uint8_t *out_xy /* n*64 */, uint8_t *ok /* n */);
/* Diagnostic: the device's arithmetic in GF(2^256 - 2^32 - 977) (csrc/fsecp256k1.hip.h) on RAW limb images — 9 signed 32-bit limbs each,
 * value sum l[i] 2^(29 i), plain (no Montgomery form).  out: n x 12 x 32 bytes of canonical little-endian results: a b, a^2, a + b, a - b,
 * -a, carry(a), a b + b a (fused), carry(a)^-1 (0 for 0), sqrt(carry(a)) or 0, a, 21 a (mul_small), carry(a)^2.  flags[i]: bit 0 a is a
 * square, bit 1 a is odd. */
DR_API int dr_secp256k1_field_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*9 */, const int32_t *b_limbs /* n*9 */, size_t n,
                                       uint8_t *out /* n*384 */, uint8_t *flags /* n */);
/* The map of RFC 9380 onto secp256k1 (simplified SWU onto the isogenous curve, the 3-isogeny back): n items of per_item field elements
 * (32 bytes little-endian each, below p; 2: the uniform (RO) encoding, 1: the nonuniform one), out_xy[i] = the sum of item i's images,
 * affine x || y.  ok[i] = 0 where a denominator of the isogeny is zero (the reference raises there; hashing cannot reach it in practice). */
DR_API int dr_secp256k1_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*32 */, size_t n, int per_item, uint8_t *out_xy /* n*64 */,
                                     uint8_t *ok /* n */);
/* The map of RFC 9380 onto P-256 (simplified SWU, A = -3, Z = -10, no isogeny), same arguments: out_xy[i] = the sum of item i's images,
 * affine x || y (64 zero bytes if two images cancel); ok[i] is always 1 (no denominator of this map can vanish).  Inputs at or above p
 * are refused with DR_ERR_INVALID. */
DR_API int dr_p256_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*32 */, size_t n, int per_item, uint8_t *out_xy /* n*64 */,
                                uint8_t *ok /* n */);
/* The map of RFC 9380 onto Ed25519 (Elligator 2 onto curve25519 with Z = 2, then x = sqrt(-486664) u / v, y = (u - 1) / (u + 1) with the
 * root the reference takes), same arguments: out_xy[i] = 8 times the sum of item i's images, a point of the prime-order subgroup.
 * ok[i] = 0 where an image has no value (v = 0 or u = -1 on curve25519; the element 0 maps there): the reference's modular inverse
 * fails there and out_xy[i] is meaningless.  Inputs at or above p are refused with DR_ERR_INVALID. */
DR_API int dr_ed25519_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*32 */, size_t n, int per_item, uint8_t *out_xy /* n*64 */,
                                   uint8_t *ok /* n */);
/* Curve25519 (DR_CURVE_CURVE25519_RO / _NU) with the identity flags spelled out (see the curve ids for their meaning; id_in may be NULL:
 * no input is the identity).  The flag is the only form of the identity here: a point whose flag is 0 must have both coordinates below
 * p, so 64 bytes of 0xff — the identity of the generic dr_te_* entry points — are refused with DR_ERR_INVALID like any other
 * non-canonical coordinate.  Scalars are reduced mod l on the device and go through the fixed schedule of the other native suites.
 *   dr_curve25519_scalar_mul_batch  out[i] = k[i] P[i]
 *   dr_curve25519_msm_groups        out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64
 *   dr_curve25519_decode_points     one 64-byte u || v per point: ok[i] = 1 iff u < p, v < p and the curve equation holds (check = 0: all
 *                                   the reference's string_to_point asks, so (0, 0) and the other small-order points pass) and, with
 *                                   check = 1, the point is also a non-identity point of the prime-order subgroup (the VRF layer's
 *                                   dec_point; dr_te_decode_points for these ids).  out_uv[i] = the point, or 64 zero bytes.
 *   dr_curve25519_map_to_curve      RFC 9380 curve25519_XMD:SHA-512_ELL2_RO_ / _NU_ after hash_to_field: the sum of the Elligator 2 images
 *                                   of item i's per_item (2 or 1) elements, times the cofactor 8 unless clear_cofactor = 0.  Every element
 *                                   below p has an image (0 maps to (0, 0)): there is no error flag; elements at or above p are refused. */
DR_API int dr_curve25519_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_uv /* n*64 */, const uint8_t *id_in /* n or NULL */,
                                          const uint8_t *scalars /* n*32 */, size_t n, uint8_t *out_uv /* n*64 */, uint8_t *id_out /* n */);
DR_API int dr_curve25519_msm_groups(dr_ctx *ctx, const uint8_t *pts_uv /* groups*m*64 */, const uint8_t *id_in /* groups*m or NULL */,
                                    const uint8_t *scalars /* groups*m*32 */, size_t groups, size_t m, uint8_t *out_uv /* groups*64 */,
                                    uint8_t *id_out /* groups */);
DR_API int dr_curve25519_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*64 */, size_t n, uint8_t *out_uv /* n*64 */, uint8_t *ok /* n */);
DR_API int dr_curve25519_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*32 */, size_t n, int per_item, int clear_cofactor,
                                      uint8_t *out_uv /* n*64 */, uint8_t *id_out /* n */);
/* Baby JubJub point decoding with the prime-order check (check = 1: as dr_te_decode_points for DR_CURVE_BABYJUBJUB) or the codec
 * alone (check = 0: y < p and a root; (0, 1) and (0, p - 1) decode whatever the sign bit).  ok[i] = 1 when accepted; out_xy[i] is
 * then x || y, otherwise 64 zero bytes. */
DR_API int dr_bjj_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*32 */, size_t n, uint8_t *out_xy /* n*64 */, uint8_t *ok /* n */);
/* Diagnostic: the device's arithmetic in the BN254 scalar field (csrc/fbn254.hip.h) on RAW limb images — 9 signed 32-bit limbs each,
 * value sum l[i] 2^(29 i), standing for value * 2^-261 mod p (Montgomery form).  out: n x 12 x 32 bytes of canonical little-endian
 * results: a b, a^2, a + b, a - b, -a, carry(a), a b + b a (fused), a^-1 (0 for 0), sqrt(a) or 0, a, a b through the LDS word form,
 * a through unpack(pack(a)).  flags[i]: bit 0 a is a square, bit 2 a > p - a. */
DR_API int dr_bjj_field_ops_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*9 */, const int32_t *b_limbs /* n*9 */, size_t n,
                                     uint8_t *out /* n*384 */, uint8_t *flags /* n */);

/* DR_CURVE_BLS12_381_G1 (the reference's BLS12_381_G1 = BLS12_381_G1_RO) and DR_CURVE_BLS12_381_G1_NU (BLS12_381_G1_NU): hashing to
 * BLS12-381's G1 by RFC 9380 (dot_ring/curve/specs/bls12_381_G1.py: E: y^2 = x^3 + 4 over the 381-bit Fq, #E(Fq) = h r,
 * BLS12381G1_XMD:SHA-256_SSWU_RO_ / _NU_: simplified SWU onto the 11-isogenous curve with Z = 11, the isogeny back, the sum of two images
 * for RO and one for NU, then times h_eff = 0xd201000000010001) and the group of E(Fq) — csrc/kernels_g1_h2c.hip.h over the device's Fq
 * (csrc/fq28.hip.h).  The FIRST curve here whose coordinates are 48 bytes, so it has entry points of its own (dr_blsg1_*) and EVERY
 * 64-byte entry point refuses these two ids with DR_ERR_INVALID: dr_te_*, dr_encode_to_curve_batch, dr_hash_to_field_batch, the provers
 * and verifiers, the ring calls, GLV and dr_bsn_*.  There is no VRF over these suites: the reference's point length for this curve (32)
 * contradicts the 49 bytes its points encode to, so no key or proof of it can be decoded.
 *
 * POINTS are affine x || y, 48 + 48 bytes LITTLE-endian, canonical standard form; 96 zero bytes are the identity ((0, 0) is not on the
 * curve).  This is NOT the big-endian record of dr_g1_msm* / dr_srs_* below (seam B), which stays as it is.  A point may be ANY point of
 * E(Fq), in G1 or not: SCALARS are 32 bytes little-endian used AS THEY ARE (0 <= k < 2^256, never reduced mod r).
 *   dr_blsg1_hash_to_field_batch    host only: expand_message_xmd over SHA-256 (Z_pad 64 bytes), L = 64 bytes per element, big-endian, mod
 *                                   p, with the DST of `variant` (one of the two curve ids): two elements per message for RO, one for
 *                                   NU, 48 bytes little-endian each.  msgs / off as dr_hash_to_field_batch (off: count + 1 offsets).
 *   dr_blsg1_map_to_curve           n items of per_item (2 or 1) elements below p: out_xy[i] = the sum of their images, times h_eff if
 *                                   clear (clear = 0: the reference's map_to_curve_simple_swu, the Q0 / Q1 / Q of RFC 9380's vectors).
 *                                   ok[i] = 0 where a denominator of the isogeny vanishes (the reference's modular inverse raises).
 *                                   Elements at or above p and other per_item are refused with DR_ERR_INVALID.
 *   dr_blsg1_encode_to_curve_batch  encode_to_curve(salt_i || msg_i) (salts nullable): hash_to_field on the worker threads and one map
 *                                   launch; DR_ERR_INVALID if a map has no value.
 *   dr_blsg1_scalar_mul_batch       out[i] = k[i] P[i];  dr_blsg1_msm_groups  out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64
 *   dr_blsg1_msm                    ONE sum of n terms k_i P_i, in the forms of dr_blsg1_msm_groups; `curve` is either id.  Below 257 terms
 *                                   it launches dr_blsg1_msm_groups' kernel in chunks of up to 64 and folds them on the host; from there
 *                                   on the bucket method (csrc/wave_msm.hip.h), which is NOT a fixed schedule: secret scalars go through
 *                                   dr_blsg1_scalar_mul_batch and dr_blsg1_msm_groups.  n = 0 gives the identity.
 *   dr_blsg1_decode_points          49-byte SEC1 compressed strings (0x02 / 0x03 by the parity of y, then x BIG-endian, x < p, x^3 + 4 a
 *                                   square).  check = 0 accepts every point of E(Fq), as the reference's string_to_point; check = 1
 *                                   also demands r P = O (the reference's valid_point).  out_xy[i] = the point, or 96 zero bytes.
 *   dr_blsg1_field_selftest         diagnostic: what kernels_g1_h2c.hip.h adds to the field, on RAW limb images (14 signed 32-bit limbs
 *                                   each, value sum l[i] 2^(28 i), standing for value 2^-392 mod p).  out: n x 5 x 48 bytes, each the
 *                                   canonical little-endian value r 2^-392 mod p of: a^((p - 3) / 4); its product with a if that is a
 *                                   root of a, else 0; select(i odd, a, b); 12 a (lazy additions and carries); a b + b a (fused).
 *                                   flags[i]: bit 0 a is a square, bit 1 the canonical a 2^-392 mod p is odd (sgn0), bit 2 a is zero. */
enum { DR_CURVE_BLS12_381_G1 = 15, DR_CURVE_BLS12_381_G1_NU = 16 };
DR_API int dr_blsg1_hash_to_field_batch(int variant, const uint8_t *msgs, const uint64_t *off, size_t count, uint8_t *out /* count*(96|48) */);
DR_API int dr_blsg1_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*48 */, size_t n, int per_item, int clear,
                                 uint8_t *out_xy /* n*96 */, uint8_t *ok /* n */);
DR_API int dr_blsg1_encode_to_curve_batch(dr_ctx *ctx, int variant, const uint8_t *msgs, const uint64_t *off, const uint8_t *salts,
                                          const uint64_t *salt_off, size_t count, uint8_t *out_xy /* count*96 */);
DR_API int dr_blsg1_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_xy /* n*96 */, const uint8_t *scalars /* n*32 */, size_t n,
                                     uint8_t *out_xy /* n*96 */);
DR_API int dr_blsg1_msm_groups(dr_ctx *ctx, const uint8_t *pts_xy /* groups*m*96 */, const uint8_t *scalars /* groups*m*32 */, size_t groups,
                               size_t m, uint8_t *out_xy /* groups*96 */);
DR_API int dr_blsg1_msm(dr_ctx *ctx, int curve, const uint8_t *pts_xy /* n*96 */, const uint8_t *scalars /* n*32 */, size_t n, uint8_t *out_xy /* 96 */);
DR_API int dr_blsg1_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*49 */, size_t n, uint8_t *out_xy /* n*96 */, uint8_t *ok /* n */);
DR_API int dr_blsg1_field_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*14 */, const int32_t *b_limbs /* n*14 */, size_t n,
                                   uint8_t *out /* n*240 */, uint8_t *flags /* n */);

/* DR_CURVE_BLS12_381_G2 (the reference's BLS12_381_G2 = BLS12_381_G2_RO) and DR_CURVE_BLS12_381_G2_NU (BLS12_381_G2_NU): hashing to
 * BLS12-381's G2 by RFC 9380 (dot_ring/curve/specs/bls12_381_G2.py: E: y^2 = x^3 + 4 (1 + i) over Fq2 = Fq[i] / (i^2 + 1), #E(Fq2) = h2 r,
 * BLS12381G2_XMD:SHA-256_SSWU_RO_ / _NU_: simplified SWU onto the 3-isogenous curve with Z = -(2 + i), the isogeny back, the sum of two
 * images for RO and one for NU, then the cofactor clearing of appendix G.3, which equals the multiplication by the 636-bit h_eff) and the
 * group of E(Fq2) — csrc/kernels_g2_h2c.hip.h over csrc/fq2_28.hip.h.  Entry points of their own (dr_blsg2_*); EVERY 64-byte entry point
 * refuses these two ids with DR_ERR_INVALID, as it refuses 15 and 16, and so does every dr_blsg1_* call that takes a variant.  There is no
 * VRF over these suites: the reference has no point codec for this curve.
 *
 * FIELD ELEMENTS are c0 || c1 (c0 + c1 i), 48 + 48 bytes LITTLE-endian, canonical standard form; a component at or above p is refused
 * with DR_ERR_INVALID.  POINTS are affine x || y, 192 bytes; 192 zero bytes are the identity ((0, 0) is not on the curve).  A point may be
 * ANY point of E(Fq2), in G2 or not: SCALARS are 96 bytes little-endian used AS THEY ARE (0 <= k < 2^768, never reduced).
 *   dr_blsg2_hash_to_field_batch    host only: expand_message_xmd over SHA-256 (Z_pad 64 bytes), m = 2, L = 64 bytes per component,
 *                                   big-endian, mod p, with the DST of `variant` (one of the two curve ids): two elements (192 bytes, from
 *                                   256 uniform bytes) per message for RO, one (96, from 128) for NU.  msgs / off as
 *                                   dr_hash_to_field_batch (off: count + 1 offsets).
 *   dr_blsg2_map_to_curve           n items of per_item (2 or 1) elements: out_xy[i] = the sum of their images, cleared if clear (clear = 0:
 *                                   the reference's map_to_curve_simple_swu, the Q0 / Q1 of RFC 9380's vectors).  ok[i] = 0 where a
 *                                   denominator of the isogeny vanishes; no input reaches that (the isogeny's kernel has no point over
 *                                   Fq2 with a rational x on E'), the flag is kept for the shape of the G1 call.  Other per_item are refused.
 *   dr_blsg2_encode_to_curve_batch  encode_to_curve(salt_i || msg_i) (salts nullable): hash_to_field on the worker threads, then the map.
 *   dr_blsg2_scalar_mul_batch       out[i] = k[i] P[i]: a bit-by-bit walk from the top set bit of each wave's largest scalar.  Scalars
 *                                   are treated as PUBLIC (the walk's length and its skipped additions depend on them).
 *   dr_blsg2_msm_groups             out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64, 96-byte scalars: one lane per term on the same walk,
 *                                   the lanes of a group folded by the complete addition.  m = 0 and m > 64 are refused; groups = 0
 *                                   returns at once.
 *   dr_blsg2_msm                    ONE sum of n terms k_i P_i with 32-byte scalars used AS THEY ARE (0 <= k < 2^256; wider scalars are
 *                                   split by the caller); `curve` is either id.  Below 257 terms it launches dr_blsg2_msm_groups'
 *                                   kernel (over 32-byte scalars) in chunks of up to 64 and folds them on the host; from there on the
 *                                   bucket method (csrc/wave_msm.hip.h over csrc/kernels_g2_msm.hip.h).  Neither is a fixed schedule:
 *                                   scalars on this curve are public.  n = 0 gives the identity.
 *   dr_blsg2_check_points           ok[i] = 1 iff point i satisfies the curve equation (the identity does); subgroup = 1 also demands
 *                                   r P = O.
 *   dr_blsg2_field_selftest         diagnostic of csrc/fq2_28.hip.h on RAW limb images (2 x 14 signed 32-bit limbs an element, c0 then c1,
 *                                   value sum l[i] 2^(28 i), standing for value 2^-392 mod p).  out: n x 5 x 96 bytes, each the canonical
 *                                   c0 || c1 of: a b; a^2; a^-1 (0 for 0); 12 (1 + i) a as the group law computes it (folds, additions,
 *                                   carries; a's components in (-2.1 p, 1.1 p)); a root of a, or 0 if a is no square.  flags[i]: bit 0 a
 *                                   is a square, bit 1 sgn0(a) (RFC 9380 4.1, m = 2), bit 2 a is zero. */
enum { DR_CURVE_BLS12_381_G2 = 17, DR_CURVE_BLS12_381_G2_NU = 18 };
DR_API int dr_blsg2_hash_to_field_batch(int variant, const uint8_t *msgs, const uint64_t *off, size_t count, uint8_t *out /* count*(192|96) */);
DR_API int dr_blsg2_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*96 */, size_t n, int per_item, int clear,
                                 uint8_t *out_xy /* n*192 */, uint8_t *ok /* n */);
DR_API int dr_blsg2_encode_to_curve_batch(dr_ctx *ctx, int variant, const uint8_t *msgs, const uint64_t *off, const uint8_t *salts,
                                          const uint64_t *salt_off, size_t count, uint8_t *out_xy /* count*192 */);
DR_API int dr_blsg2_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_xy /* n*192 */, const uint8_t *scalars /* n*96 */, size_t n,
                                     uint8_t *out_xy /* n*192 */);
DR_API int dr_blsg2_msm_groups(dr_ctx *ctx, const uint8_t *pts_xy /* groups*m*192 */, const uint8_t *scalars /* groups*m*96 */, size_t groups,
                               size_t m, uint8_t *out_xy /* groups*192 */);
DR_API int dr_blsg2_msm(dr_ctx *ctx, int curve, const uint8_t *pts_xy /* n*192 */, const uint8_t *scalars /* n*32 */, size_t n, uint8_t *out_xy /* 192 */);
DR_API int dr_blsg2_check_points(dr_ctx *ctx, int subgroup, const uint8_t *pts_xy /* n*192 */, size_t n, uint8_t *ok /* n */);
DR_API int dr_blsg2_field_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*28 */, const int32_t *b_limbs /* n*28 */, size_t n,
                                   uint8_t *out /* n*480 */, uint8_t *flags /* n */);

/* DR_CURVE_ED448_RO (the reference's Ed448 = Ed448_RO) and DR_CURVE_ED448_NU (Ed448_NU): the Edwards curve x^2 + y^2 = 1 - 39081 x^2 y^2
 * over p = 2^448 - 2^224 - 1 (dot_ring/curve/specs/ed448.py), cofactor 4, hashing by RFC 9380's edwards448_XOF:SHAKE256_ELL2_RO_ (two field
 * elements) or ..._NU_ (one) — csrc/kernels_ed448.hip.h over csrc/fe448.hip.h.  Entry points of their own (dr_ed448_*); EVERY 64-byte
 * entry point (dr_te_*, dr_bsn_*, the dr_vrf_suite calls, the ring calls) refuses these two ids with DR_ERR_INVALID, and so do the
 * dr_blsg1_* / dr_blsg2_* calls as variants.  Formats: field elements and coordinates are 56 bytes little-endian, canonical (< p); points
 * are affine x || y, 112 bytes, the identity (0, 1) as itself (a point of the curve: no flag byte, no zero-bytes convention); scalars are
 * 56 bytes used AS THEY ARE (any k < 2^448, no reduction mod the group order: small-order points and images before the cofactor is
 * cleared are multiplied exactly).  Coordinates or elements at or above p and other per_item values give DR_ERR_INVALID.
 *   dr_ed448_hash_to_field_batch    host only: expand_message_xof over SHAKE256, L = 84 bytes per element, the variant's DST
 *                                   (QUUX-V01-CS02-with-edwards448_XOF:SHAKE256_ELL2_RO_ / ..._NU_); two elements (112 bytes) per message
 *                                   for RO, one (56) for NU.
 *   dr_ed448_map_to_curve           n items of per_item (2 or 1) elements: out_xy[i] = the sum of their Elligator 2 images (through the
 *                                   reference's mont_to_ed448), times 4 if clear (clear = 0, per_item = 1: the reference's map_to_curve).
 *                                   ok[i] = 0 and 112 zero bytes where an image has no value: an element in {0, 1, p - 1}, and no other.
 *   dr_ed448_encode_to_curve_batch  encode_to_curve(salt_i || msg_i) (salts nullable): hash_to_field on the worker threads, then the map;
 *                                   DR_ERR_INVALID if a map has no value.
 *   dr_ed448_scalar_mul_batch       out[i] = k[i] P[i], the window loop on a fixed schedule (113 signed 4-bit windows) as for the other native
 *                                   suites; the final inversion of Z (division steps) is not fixed-time.
 *   dr_ed448_msm_groups             out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64.
 *   dr_ed448_decode_points          ok[i] = 1 and out_xy[i] = enc[i] iff both coordinates are below p and the curve equation holds, and
 *                                   with check = 1 also P is not the identity and n P = O; otherwise ok[i] = 0 and 112 zero bytes.
 *   dr_ed448_field_selftest         diagnostic of csrc/fe448.hip.h on RAW limb images (16 signed 32-bit limbs an element): out[i] = eleven
 *                                   56-byte canonical records (a b, a^2, a + b, a - b, -a, carry(a), 39081 a, a^-1, a^((p + 1) / 4), a,
 *                                   156326 a), flags[i]: bit 0 a is a square, bit 1 a is odd, bit 2 a is zero, bit 3 a = b. */
enum { DR_CURVE_ED448_RO = 19, DR_CURVE_ED448_NU = 20 };
DR_API int dr_ed448_hash_to_field_batch(int variant, const uint8_t *msgs, const uint64_t *off, size_t count, uint8_t *out /* count*(112|56) */);
DR_API int dr_ed448_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*56 */, size_t n, int per_item, int clear,
                                 uint8_t *out_xy /* n*112 */, uint8_t *ok /* n */);
DR_API int dr_ed448_encode_to_curve_batch(dr_ctx *ctx, int variant, const uint8_t *msgs, const uint64_t *off, const uint8_t *salts,
                                          const uint64_t *salt_off, size_t count, uint8_t *out_xy /* count*112 */);
DR_API int dr_ed448_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_xy /* n*112 */, const uint8_t *scalars /* n*56 */, size_t n,
                                     uint8_t *out_xy /* n*112 */);
DR_API int dr_ed448_msm_groups(dr_ctx *ctx, const uint8_t *pts_xy, const uint8_t *scalars, size_t groups, size_t m,
                               uint8_t *out_xy /* groups*112 */);
DR_API int dr_ed448_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*112 */, size_t n, uint8_t *out_xy /* n*112 */,
                                  uint8_t *ok /* n */);
DR_API int dr_ed448_field_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*16 */, const int32_t *b_limbs /* n*16 */, size_t n,
                                   uint8_t *out /* n*11*56 */, uint8_t *flags /* n */);

/* DR_CURVE_CURVE448_RO (the reference's Curve448 = Curve448_RO) and DR_CURVE_CURVE448_NU (Curve448_NU): the Montgomery curve
 * v^2 = u^3 + 156326 u^2 + u over p = 2^448 - 2^224 - 1 (dot_ring/curve/specs/curve448.py over montgomery/mg_affine_point.py), cofactor 4,
 * hashing by RFC 9380's curve448_XOF:SHAKE256_ELL2_RO_ (two field elements) or ..._NU_ (one) — csrc/kernels_curve448.hip.h, which computes
 * on the complete Edwards law of csrc/c448_law.hip.h (the curve birational to curve448) over csrc/fe448.hip.h.  Entry points of their own
 * (dr_curve448_*); every 64-byte entry point refuses these two ids with DR_ERR_INVALID, and so do the dr_blsg1_* / dr_blsg2_* /
 * dr_ed448_* calls as variants.  Formats: field elements and coordinates are 56 bytes little-endian, canonical (< p); points are affine
 * u || v, 112 bytes; scalars are 56 bytes used AS THEY ARE (any k < 2^448).  THE IDENTITY has no affine coordinates and (0, 0) is a point
 * of the curve (order 2): at every entry point below the identity is 112 bytes of 0xff, in and out, and there are no flag-byte
 * parameters.  Other coordinates or elements at or above p and other per_item values give DR_ERR_INVALID.
 *   dr_curve448_hash_to_field_batch    host only: expand_message_xof over SHAKE256, L = 84, the variant's DST
 *                                      (QUUX-V01-CS02-with-curve448_XOF:SHAKE256_ELL2_RO_ / ..._NU_); 112 bytes per message for RO, 56 for NU.
 *   dr_curve448_map_to_curve           n items of per_item (2 or 1) elements: out_uv[i] = the sum of their Elligator 2 images, times 4 if
 *                                      clear (clear = 0, per_item = 1: the reference's map_to_curve).  ok[i] = 0 and 112 zero bytes where an
 *                                      image has no value: an element in {1, p - 1}, and no other (0 maps to (0, 0)).
 *   dr_curve448_encode_to_curve_batch  encode_to_curve(salt_i || msg_i) (salts nullable); DR_ERR_INVALID if a map has no value.
 *   dr_curve448_scalar_mul_batch       out[i] = k[i] P[i], the window loop on a fixed schedule (113 signed 4-bit windows); the final
 *                                      inversion (division steps) is not fixed-time.
 *   dr_curve448_msm_groups             out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64.
 *   dr_curve448_decode_points          ok[i] = 1 and out_uv[i] = enc[i] iff both coordinates are below p and the curve equation holds
 *                                      ((0, 0) passes; 112 bytes of 0xff do not), and with check = 1 also n P = O; otherwise ok[i] = 0
 *                                      and 112 zero bytes.
 * The diagnostic of the field is dr_ed448_field_selftest. */
enum { DR_CURVE_CURVE448_RO = 21, DR_CURVE_CURVE448_NU = 22 };
DR_API int dr_curve448_hash_to_field_batch(int variant, const uint8_t *msgs, const uint64_t *off, size_t count, uint8_t *out /* count*(112|56) */);
DR_API int dr_curve448_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*56 */, size_t n, int per_item, int clear,
                                    uint8_t *out_uv /* n*112 */, uint8_t *ok /* n */);
DR_API int dr_curve448_encode_to_curve_batch(dr_ctx *ctx, int variant, const uint8_t *msgs, const uint64_t *off, const uint8_t *salts,
                                             const uint64_t *salt_off, size_t count, uint8_t *out_uv /* count*112 */);
DR_API int dr_curve448_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_uv /* n*112 */, const uint8_t *scalars /* n*56 */, size_t n,
                                        uint8_t *out_uv /* n*112 */);
DR_API int dr_curve448_msm_groups(dr_ctx *ctx, const uint8_t *pts_uv, const uint8_t *scalars, size_t groups, size_t m,
                                  uint8_t *out_uv /* groups*112 */);
DR_API int dr_curve448_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*112 */, size_t n, uint8_t *out_uv /* n*112 */,
                                     uint8_t *ok /* n */);

/* DR_CURVE_P521_RO (the reference's P521 = P521_RO) and DR_CURVE_P521_NU (P521_NU): P-521, y^2 = x^3 - 3 x + b over p = 2^521 - 1
 * (dot_ring/curve/specs/p521.py), prime order, cofactor 1, hashing by RFC 9380's P521_XMD:SHA-512_SSWU_RO_ (two field elements) or
 * ..._NU_ (one) — csrc/kernels_p521.hip.h on the complete law of csrc/sw3_law.hip.h over csrc/fp521.hip.h.  Entry points of their own
 * (dr_p521_*); every 64-byte entry point refuses these two ids with DR_ERR_INVALID, and so do the dr_blsg1_* / dr_blsg2_* / dr_ed448_* /
 * dr_curve448_* calls as variants.  Formats: field elements and coordinates are 68 bytes little-endian, canonical (< p); points are
 * affine x || y, 136 bytes, and 136 ZERO BYTES ARE THE IDENTITY, in and out ((0, 0) is not on the curve); scalars are 68 bytes
 * little-endian below 2^521, used AS THEY ARE (a scalar at or above 2^521 gives DR_ERR_INVALID before anything is uploaded).  Coordinates
 * or elements at or above p and other per_item values give DR_ERR_INVALID.
 *   dr_p521_hash_to_field_batch    host only: expand_message_xmd over SHA-512, L = 98 bytes per element, the variant's DST
 *                                  (QUUX-V01-CS02-with-P521_XMD:SHA-512_SSWU_RO_ / ..._NU_); two elements (136 bytes) per message for RO,
 *                                  one (68) for NU.
 *   dr_p521_map_to_curve           n items of per_item (2 or 1) elements: out_xy[i] = the sum of their simplified SWU images (Z = -4, no
 *                                  isogeny).  ok[i] = 1 always: every element has an image.  The cofactor is 1: `clear` changes nothing.
 *   dr_p521_encode_to_curve_batch  encode_to_curve(salt_i || msg_i) (salts nullable): hash_to_field on the worker threads, then the map.
 *   dr_p521_scalar_mul_batch       out[i] = k[i] P[i], the window loop on a fixed schedule (131 signed 4-bit windows) as for the other
 *                                  native suites; the final inversion of Z (division steps) is not fixed-time.
 *   dr_p521_msm_groups             out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64.
 *   dr_p521_decode_points          SEC1 compressed, 67 bytes: ok[i] = 1 and out_xy[i] = x || y iff byte 0 is 0x02 or 0x03, x (bytes 1..66
 *                                  big-endian) is below p and x^3 - 3 x + b is a square, y of byte 0's parity; otherwise ok[i] = 0 and
 *                                  136 zero bytes.  No string encodes the identity and the cofactor is 1, so check = 0 and check = 1 are
 *                                  the same kernel; the parameter is the suites' common signature.
 *   dr_p521_field_selftest         diagnostic of csrc/fp521.hip.h on RAW limb images (19 signed 32-bit limbs an element): out[i] = eleven
 *                                  68-byte canonical records (a b, a^2, a + b, a - b, -a, carry(a), 4 a, a^-1, carry(a)^((p + 1) / 4), a,
 *                                  -(2^28 - 1) a), flags[i]: bit 0 a is a square, bit 1 a is odd, bit 2 a is zero, bit 3 a = b. */
enum { DR_CURVE_P521_RO = 23, DR_CURVE_P521_NU = 24 };
DR_API int dr_p521_hash_to_field_batch(int variant, const uint8_t *msgs, const uint64_t *off, size_t count, uint8_t *out /* count*(136|68) */);
DR_API int dr_p521_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*68 */, size_t n, int per_item, int clear,
                                uint8_t *out_xy /* n*136 */, uint8_t *ok /* n */);
DR_API int dr_p521_encode_to_curve_batch(dr_ctx *ctx, int variant, const uint8_t *msgs, const uint64_t *off, const uint8_t *salts,
                                         const uint64_t *salt_off, size_t count, uint8_t *out_xy /* count*136 */);
DR_API int dr_p521_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_xy /* n*136 */, const uint8_t *scalars /* n*68 */, size_t n,
                                    uint8_t *out_xy /* n*136 */);
DR_API int dr_p521_msm_groups(dr_ctx *ctx, const uint8_t *pts_xy, const uint8_t *scalars, size_t groups, size_t m,
                              uint8_t *out_xy /* groups*136 */);
DR_API int dr_p521_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*67 */, size_t n, uint8_t *out_xy /* n*136 */,
                                 uint8_t *ok /* n */);
DR_API int dr_p521_field_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*19 */, const int32_t *b_limbs /* n*19 */, size_t n,
                                  uint8_t *out /* n*11*68 */, uint8_t *flags /* n */);

/* DR_CURVE_P384_RO (the reference's P384 = P384_RO) and DR_CURVE_P384_NU (P384_NU): P-384, y^2 = x^3 - 3 x + b over
 * p = 2^384 - 2^128 - 2^96 + 2^32 - 1 (dot_ring/curve/specs/p384.py), prime order, cofactor 1, hashing by RFC 9380's
 * P384_XMD:SHA-384_SSWU_RO_ (two field elements) or ..._NU_ (one) — csrc/kernels_p384.hip.h on the complete law of csrc/sw3_law.hip.h
 * over csrc/fp384.hip.h (Montgomery form inside the kernels only).  Entry points of their own (dr_p384_*); every 64-byte entry point
 * refuses these two ids with DR_ERR_INVALID, and so do the dr_blsg1_* / dr_blsg2_* / dr_ed448_* / dr_curve448_* / dr_p521_* calls as
 * variants; the dr_p384_* calls refuse every other id.  Formats: field elements and coordinates are 48 bytes little-endian, canonical
 * (< p); points are affine x || y, 96 bytes, and 96 ZERO BYTES ARE THE IDENTITY, in and out ((0, 0) is not on the curve); scalars are
 * 48 bytes little-endian used AS THEY ARE, every 384-bit value (none is refused).  Coordinates or elements at or above p and other
 * per_item values give DR_ERR_INVALID.
 *   dr_p384_hash_to_field_batch    host only: expand_message_xmd over SHA-384, L = 72 bytes per element, the variant's DST
 *                                  (QUUX-V01-CS02-with-P384_XMD:SHA-384_SSWU_RO_ / ..._NU_); two elements (96 bytes) per message for RO,
 *                                  one (48) for NU.
 *   dr_p384_map_to_curve           n items of per_item (2 or 1) elements: out_xy[i] = the sum of their simplified SWU images (Z = -12, no
 *                                  isogeny).  ok[i] = 1 always: every element has an image.  The cofactor is 1: `clear` changes nothing.
 *   dr_p384_encode_to_curve_batch  encode_to_curve(salt_i || msg_i) (salts nullable): hash_to_field on the worker threads, then the map.
 *   dr_p384_scalar_mul_batch       out[i] = k[i] P[i], the window loop on a fixed schedule (97 signed 4-bit windows) as for the other
 *                                  native suites; the final inversion of Z (division steps) is not fixed-time.
 *   dr_p384_msm_groups             out[g] = sum_{j<m} k[g m + j] P[g m + j], m <= 64.
 *   dr_p384_decode_points          SEC1 compressed, 49 bytes: ok[i] = 1 and out_xy[i] = x || y iff byte 0 is 0x02 or 0x03, x (bytes 1..48
 *                                  big-endian) is below p and x^3 - 3 x + b is a square, y of byte 0's parity; otherwise ok[i] = 0 and
 *                                  96 zero bytes.  No string encodes the identity and the cofactor is 1, so check = 0 and check = 1 are
 *                                  the same kernel; the parameter is the suites' common signature.
 *   dr_p384_field_selftest         diagnostic of csrc/fp384.hip.h on RAW limb images (14 signed 32-bit limbs; an image stands for its
 *                                  value times 2^-392 mod p): out[i] = thirteen 48-byte canonical records (a b, a^2, a + b, a - b, -a,
 *                                  carry(a), 4 a, a^-1, carry(a)^((p + 1) / 4), a, -(2^28 - 1) a, carry(a)^2, the fused 2 a b), flags[i]:
 *                                  bit 0 a is a square, bit 1 a is odd, bit 2 a is zero, bit 3 a = b. */
enum { DR_CURVE_P384_RO = 25, DR_CURVE_P384_NU = 26 };
DR_API int dr_p384_hash_to_field_batch(int variant, const uint8_t *msgs, const uint64_t *off, size_t count, uint8_t *out /* count*(96|48) */);
DR_API int dr_p384_map_to_curve(dr_ctx *ctx, const uint8_t *us /* n*per_item*48 */, size_t n, int per_item, int clear,
                                uint8_t *out_xy /* n*96 */, uint8_t *ok /* n */);
DR_API int dr_p384_encode_to_curve_batch(dr_ctx *ctx, int variant, const uint8_t *msgs, const uint64_t *off, const uint8_t *salts,
                                         const uint64_t *salt_off, size_t count, uint8_t *out_xy /* count*96 */);
DR_API int dr_p384_scalar_mul_batch(dr_ctx *ctx, const uint8_t *pts_xy /* n*96 */, const uint8_t *scalars /* n*48 */, size_t n,
                                    uint8_t *out_xy /* n*96 */);
DR_API int dr_p384_msm_groups(dr_ctx *ctx, const uint8_t *pts_xy, const uint8_t *scalars, size_t groups, size_t m,
                              uint8_t *out_xy /* groups*96 */);
DR_API int dr_p384_decode_points(dr_ctx *ctx, int check, const uint8_t *enc /* n*49 */, size_t n, uint8_t *out_xy /* n*96 */,
                                 uint8_t *ok /* n */);
DR_API int dr_p384_field_selftest(dr_ctx *ctx, const int32_t *a_limbs /* n*14 */, const int32_t *b_limbs /* n*14 */, size_t n,
                                  uint8_t *out /* n*13*48 */, uint8_t *flags /* n */);

/* ---- one MSM on a wide suite ---------------------------------------------------------------------
 * out = sum_{i<n} k[i] P[i] on P-384, P-521, Ed448 or Curve448: `curve` is one of DR_CURVE_P384_RO / _NU, DR_CURVE_P521_RO / _NU,
 * DR_CURVE_ED448_RO / _NU, DR_CURVE_CURVE448_RO / _NU (RO and NU are one group); every other id gives DR_ERR_INVALID.  Points, scalars and
 * the result are in the forms of that suite's dr_<suite>_msm_groups: affine x || y (u || v) of 96, 136, 112 or 112 bytes, scalars of 48,
 * 68, 56 or 56 bytes used AS THEY ARE (P-521: below 2^521; Ed448 and Curve448: also k >= n, on points outside the prime-order
 * subgroup).  The identity is 96 / 136 zero bytes on P-384 / P-521, (0, 1) on Ed448 and 112 bytes of 0xff INSIDE the point on Curve448, in
 * and out; n = 0 gives it.  The refusals are msm_groups': a coordinate at or above p, a P-521 scalar of 2^521 or more, a null buffer, n at
 * or above the suite's batch limit.
 * Below 256 terms (WIDE_PIP_FROM, csrc/msm_plan.hpp) the call launches dr_<suite>_msm_groups' kernel in chunks of up to 64 terms and adds the
 * partial sums on the host with the suite's law.  From 256 terms on it takes the bucket method (csrc/wave_msm.hip.h): signed window
 * digits of the scalars, one bucket set per (window, index group), bucket walks, running-sum reductions, and the window combination on
 * the host.  The bucket method is NOT a fixed schedule — bucket choice and list lengths depend on the scalars, as in dr_te_msm from 256
 * terms — so it is for public scalars (the batch verifiers'); secret scalars go through scalar_mul_batch and msm_groups. */
DR_API int dr_wide_msm(dr_ctx *ctx, int curve, const uint8_t *pts, const uint8_t *scalars, size_t n, uint8_t *out);

/* ---- diagnostics of the nine group laws on RAW limb images ---------------------------------------
 * csrc/wave_curve.hip.h's wave_law_selftest over the curve's description: no packing, no inversion and no conversion on either side, so a
 * test can put every coordinate at the edge of the limb class its law documents and read the class of what the law returns.  A
 * coordinate is L signed 32-bit limbs (9: Ed25519, Baby JubJub, P-256, secp256k1; 14: BLS12-381 E(Fq), P-384; 16: Ed448, Curve448; 19:
 * P-521) in the field's own form; a point is its C coordinates x, y, z (C = 3) or x, y, z, t (C = 4: Ed25519, Baby JubJub).
 * points[i] = P then Q (2 C L limbs), controls[i] = one word, out[i] = 13 points (13 C L limbs):
 *   0 add(P, Q)   1 add(P, -Q)   2 dbl(P)   3 dbl_no_t(P) (C = 4 only; not written otherwise)   4 cneg(P, true)   6 cneg(P, false)
 *   5 slot 0 through the LDS table of the scalar multiplication (to_lds, from_lds) and back
 *   7 + w, w < 6: the accumulator after window w of the fixed schedule started at P: four doublings, then the table term (slot 0's point,
 *   from LDS) added, negated if bit w of the control word is set, the identity if bit 8 + w is.
 * n = 0 returns at once; a null buffer and n >= 2^24 are refused.  The calls launch under no profiled name. */
DR_API int dr_ed25519_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*4*9 */, const uint32_t *controls /* n */, size_t n,
                                   int32_t *out /* n*13*4*9 */);
DR_API int dr_bjj_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*4*9 */, const uint32_t *controls, size_t n, int32_t *out /* n*13*4*9 */);
DR_API int dr_p256_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*9 */, const uint32_t *controls, size_t n, int32_t *out /* n*13*3*9 */);
DR_API int dr_secp256k1_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*9 */, const uint32_t *controls, size_t n,
                                     int32_t *out /* n*13*3*9 */);
DR_API int dr_blsg1_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*14 */, const uint32_t *controls, size_t n,
                                 int32_t *out /* n*13*3*14 */);
DR_API int dr_ed448_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*16 */, const uint32_t *controls, size_t n,
                                 int32_t *out /* n*13*3*16 */);
DR_API int dr_curve448_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*16 */, const uint32_t *controls, size_t n,
                                    int32_t *out /* n*13*3*16 */);
DR_API int dr_p521_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*19 */, const uint32_t *controls, size_t n,
                                int32_t *out /* n*13*3*19 */);
DR_API int dr_p384_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*14 */, const uint32_t *controls, size_t n,
                                int32_t *out /* n*13*3*14 */);
/* The same for BLS12-381's E(Fq2) (csrc/kernels_g2_msm.hip.h, a kernel of its own: the LDS table of the fixed schedule does not fit this
 * curve): a coordinate is 28 limbs, c0's 14 then c1's, a point x, y, z.  The ABI shape and the slot numbers are the ones above, with the
 * steps of the walks this curve has:
 *   5 slot 0 through a record of the bucket method in device memory (wave_msm_put, wave_msm_get) and back
 *   7 + w, w < 6: the accumulator after step w of the bit walk started at P: ONE doubling, then that record, loaded again, added, negated
 *   if bit w of the control word is set, the identity if bit 8 + w is.
 * Slot 3 is not written. */
DR_API int dr_blsg2_law_selftest(dr_ctx *ctx, const int32_t *points /* n*2*3*28 */, const uint32_t *controls, size_t n,
                                 int32_t *out /* n*13*3*28 */);

/* square root in the Bandersnatch base field; DR_ERR_NOTSQUARE if none exists. Host-side, no ctx. */
DR_API int dr_fr_sqrt(const uint8_t in[32], uint8_t out[32]);

/* ---- seam B: KZG / BLS12-381 G1 -----------------------------------------------------------------
 * Replaces the blst calls behind dot_ring/ring_proof/pcs/kzg.py: commit :152-175 (mult_pippenger over
 * srs.blst_g1_memory[:n]), msm_g1 :147, compress_g1 :129, serialize_g1_uncompressed :133, decompress_g1 :137,
 * and the SRS memory built in dot_ring/ring_proof/pcs/srs.py:98-114.
 */
DR_API int dr_srs_load(dr_ctx *ctx, const uint8_t *g1_be_xy /* m*96 */, size_t m, dr_srs **out);
/* Synthetic bases for sizes no SRS file covers: base[i] = (first+i) * seed (first >= 1), generated on
 * the GPU.  With these bases an MSM has the closed form [sum_i k_i*(first+i)] * seed — a size-independent check. */
DR_API int dr_srs_synthetic(dr_ctx *ctx, const uint8_t seed_be_xy[96], uint32_t first, size_t count, dr_srs **out);
/* Known-tau SRS for domains the shipped file does not cover (test/bench use only — tau is public):
 * bases[i] = tau^i * base, i < count, generated on the GPU.  dr_g2_mul (host) gives the matching tau * G2. */
DR_API int dr_srs_powers(dr_ctx *ctx, const uint8_t base_be_xy[96], const uint8_t tau_le[32], size_t count, dr_srs **out);
DR_API int dr_g2_mul(const uint8_t g2_be[192], const uint8_t scalar_le[32], uint8_t out_be[192]);
/* Fixed-base window table for this SRS, kept in HBM: table[w][i] = 2^(start_w) * base[i] for the W = ceil(256/c)
 * windows of width ~c = window_bits (7..22; 0 drops the table).  Costs W * count * 96 bytes (13 MB for the shipped
 * 6145-point SRS at c = 12, 1.6 GB for 2^20 bases at c = 16) and makes every later MSM over this SRS use ONE bucket
 * set per MSM: a single bucket reduction instead of W and no window combination.  Results are unchanged. */
DR_API int dr_srs_precompute(dr_ctx *ctx, dr_srs *srs, int window_bits);
/* Shape of the table dr_srs_precompute built (all zero: none) and the tiling `batch` MSMs of n points over it would take.  An SRS
 * small enough (256 * count * 128 bytes within DOTRING_SRS_BIT_ROWS_MB, default 512: 201 MB for 6145 points) gets a row for EVERY bit,
 * table[s][i] = 2^s * base[i]; batches of hundreds of MSMs then recode every scalar in width-w non-adjacent form (w chosen per call from
 * n and batch; DOTRING_SRS_TILING=rows keeps the window rows): 256 / (w + 1) odd digits per scalar on average, each one a
 * point of the row of its bit position added to one of 2^(w-2) odd-multiple buckets — against 256 / window_bits additions over the
 * window rows.  Results are unchanged.
 *   info[0] window_bits, info[1] rows of the table (W or 256), info[2] digit rows (windows / slots) per scalar for this (n, batch),
 *   info[3] width w of the per-call tiling (0 = the window rows), info[4] tiling: 0 = window rows, 2 = width-w non-adjacent
 *   form, info[5] expected non-zero digits per scalar x 1000 */
DR_API int dr_srs_table_info(const dr_srs *srs, size_t n, size_t batch, int info[6]);
/* dr_srs_precompute, and where the table gets a row per bit it also gets the rows of the small odd multiples of every base:
 * `multiples` blocks of 256 rows, block t = 2^s * ((2 t + 1) * base[i]) (1, 2, 4, 8, 16 or 32; 0 = the library's default, 8; -1 = the
 * count the library recommends for batched proving, 32; 1 = exactly dr_srs_precompute's table).  Batches of hundreds of MSMs then write
 * a digit as +-(2 t + 1) * b with b the odd bucket value and pick, per digit, the multiplier that clears the most bits of the scalar:
 * 18.1 / 17.3 / 16.6 / 15.9 / 15.1 bucket additions per (base, scalar) pair at w = 13 with 2 / 4 / 8 / 16 / 32 multiples where the plain
 * non-adjacent form has 18.8.  The table is `multiples` times as large (1.6 GB for 6145 points at 8, 6.4 GB at 32); a table beyond
 * DOTRING_SRS_MULTIPLES_MB (default 8192: the 12289 points of a 4096-point domain get 16 blocks, 6.4 GB, where 32 would take 12.9 GB) or
 * the device's free memory gets half the blocks, and half again down to one — never an error.
 * DOTRING_SRS_MULTIPLES (1, 2, 4, 8, 16 or 32) overrides the count asked for.  Results are unchanged. */
DR_API int dr_srs_precompute_multiples(dr_ctx *ctx, dr_srs *srs, int window_bits, int multiples);
/* dr_srs_table_info's six values, then info[6] = multipliers a digit of this (n, batch) may take (1 = none), info[7] = blocks of rows
 * in the table */
DR_API int dr_srs_table_info_multiples(const dr_srs *srs, size_t n, size_t batch, int info[8]);
/* copy `count` bases starting at `offset` back to the host as BE x||y records */
DR_API int dr_srs_download(dr_ctx *ctx, const dr_srs *srs, size_t offset, size_t count, uint8_t *out_be_xy);
DR_API void dr_srs_destroy(dr_srs *srs);
DR_API size_t dr_srs_size(const dr_srs *srs);

/* out = sum_{i<n} scalars[i] * SRS[offset+i] ; *is_inf = 1 and out = zeros when the sum is the identity */
DR_API int dr_g1_msm(dr_ctx *ctx, const dr_srs *srs, size_t offset, const uint8_t *scalars /* n*32 */, size_t n,
              uint8_t out_be_xy[96], int *is_inf);
DR_API int dr_g1_msm_dev(dr_ctx *ctx, const dr_srs *srs, size_t offset, const void *d_scalars, size_t n,
                  uint8_t out_be_xy[96], int *is_inf);
/* `batch` independent MSMs over the same bases SRS[0..n): scalars is batch*n*32, out is batch*96, is_inf batch ints */
DR_API int dr_g1_msm_batch(dr_ctx *ctx, const dr_srs *srs, const uint8_t *scalars, size_t n, size_t batch,
                    uint8_t *out_be_xy, int *is_inf);
DR_API int dr_g1_msm_batch_dev(dr_ctx *ctx, const dr_srs *srs, const void *d_scalars, size_t n, size_t batch,
                        uint8_t *out_be_xy, int *is_inf);
/* MSM over caller-supplied points (verifier folds, kzg.py:295-301,332-338) */
DR_API int dr_g1_msm_points(dr_ctx *ctx, const uint8_t *pts_be_xy /* n*96 */, const uint8_t *scalars, size_t n,
                     uint8_t out_be_xy[96], int *is_inf);

/* host-side sum of a few affine points (combining per-GPU partial MSM results after an all-gather) */
DR_API int dr_g1_sum(const uint8_t *pts_be_xy /* n*96 */, size_t n, uint8_t out_be_xy[96], int *is_inf);

/* ---- multi-GPU: the base-sharded MSM (second mode; the shape of the one MSM to shard is the reference's
 * KZG.commit, dot_ring/ring_proof/pcs/kzg.py:152-175; its process-sharded bench is tests/benchmark/bench_ring_proof.py:168-182).
 * One process per GPU.  Rank g reduces its shard of (base, scalar) pairs to one point; the points are exchanged with RCCL
 * ncclAllGather over xGMI (97 bytes per rank) and every rank folds them with the group law.  librccl is dlopen'ed on first
 * use; no PyTorch anywhere.  dr_comm_unique_id runs on ONE rank, its 128 bytes reach the others through the launcher's
 * channel (dot_ring_amd/parallel.py: a TCP socket on MASTER_ADDR), then every rank calls dr_comm_create (a collective). */
#define DR_COMM_ID_BYTES 128
typedef struct dr_comm dr_comm;
DR_API int dr_comm_unique_id(uint8_t out_id[DR_COMM_ID_BYTES]);
DR_API int dr_comm_create(dr_ctx *ctx, const uint8_t id[DR_COMM_ID_BYTES], int rank, int world, dr_comm **out);
DR_API void dr_comm_destroy(dr_comm *comm);
DR_API int dr_comm_rank(const dr_comm *comm);
DR_API int dr_comm_world(const dr_comm *comm);
/* ranks RCCL itself counts in the communicator (ncclCommCount) */
DR_API int dr_comm_count(const dr_comm *comm, int *out_ranks);
/* host-to-host all-gather of `bytes` bytes per rank (staged through HBM, ncclAllGather on the context's stream) */
DR_API int dr_comm_all_gather(dr_comm *comm, const void *send, size_t bytes, void *recv /* world*bytes */);
/* this rank's n_local pairs (srs[offset..], device-resident scalars) of one MSM sharded over the communicator;
 * the result is the whole MSM, identical on every rank.  A rank whose local part fails still enters the all-gather
 * (status byte in its 97-byte record), so the others return DR_ERR_DEVICE naming it instead of blocking in the collective */
DR_API int dr_g1_msm_sharded_dev(dr_ctx *ctx, dr_comm *comm, const dr_srs *srs, size_t offset, const void *d_scalars, size_t n_local,
                                 uint8_t out_be_xy[96], int *is_inf);

/* Host-side pairing product check: *ok = 1 iff prod_i e(P_i, Q_i) == 1.  G2 points are 192-byte records in the SRS
 * file layout x.c1 || x.c0 || y.c1 || y.c0 (big-endian, dot_ring/ring_proof/pcs/srs.py:78-88).  Replaces
 * blst.PT + PT.finalverify (dot_ring/ring_proof/pcs/pairing.py:24-31); stays on the CPU (2 Miller loops per batch). */
DR_API int dr_pairing_check(const uint8_t *g1_be_xy /* n*96 */, const uint8_t *g2_be /* n*192 */, size_t n, int *ok);
/* diagnostic for tests: *consistent = 1 iff the fast final exponentiation used by dr_pairing_check (Frobenius maps +
 * x-chain, exponent 3(p^12-1)/r) equals the cube of the plain square-and-multiply one on this Miller-loop product */
DR_API int dr_pairing_selfcheck(const uint8_t *g1_be_xy, const uint8_t *g2_be, size_t n, int *consistent);

/* zcash encodings, host-side */
DR_API int dr_g1_compress(const uint8_t xy[96], int is_inf, uint8_t out[48]);
DR_API int dr_g1_decompress(const uint8_t in[48], uint8_t out_xy[96], int *is_inf);   /* on-curve check, no subgroup check (as blst P1_Affine(bytes)) */
DR_API int dr_g1_serialize_check(const uint8_t xy[96]);
/* dr_g1_decompress for n encodings in one kernel launch: out = n BE x||y records (all zero for infinity), ok[i] = 0 for
 * malformed encodings (compression flag missing, x >= p, x not on the curve, non-canonical infinity). */
DR_API int dr_g1_decompress_batch(dr_ctx *ctx, const uint8_t *enc /* n*48 */, size_t n, uint8_t *out_be_xy /* n*96 */, uint8_t *ok /* n */);                              /* DR_OK iff on curve or infinity */

/* Diagnostic: single operations of the base field the G1 kernels compute in (csrc/fq28.hip.h: 14 signed limbs of 28 bits, lazy
 * reduction, Montgomery R = 2^392) on RAW limb images, so that tests can place operands on the edges of each register form.
 * in: n records of 64 int32 — word 0 the op (0 mul a b, 1 sqr a, 2 mul2 a b + c d, 3 add, 4 sub, 5 carry, 6 canon28, 7 is_zero_mod_p,
 * 8 maybe_zero_normal(mul a b), 9 inv, 10 to_mont28, 11 from_mont28, 12 unpack28, 13 cneg a if b[0] is odd), then the 14 limbs
 * of a, b, c, d at words 1, 15, 29, 43 (the word operands of to_mont28 / unpack28 are a's first 12 words).  out: n records of 16
 * int32 — the 14 result limbs (12 canonical words for canon28 / from_mont28), the flag of is_zero_mod_p / maybe_zero_normal
 * at word 14. */
DR_API int dr_fq_ops_selftest(dr_ctx *ctx, const int32_t *in /* n*64 */, size_t n, int32_t *out /* n*16 */);
/* Diagnostic: the XYZZ group law of csrc/g1.hip.h on raw register images.  in: n records of 192 words — P and Q as XYZZ
 * images (x, y, zz, zzz limbs, then the infinity flag: 57 words) at words 0 and 64, an affine A (x, y limbs, flag) at word
 * 128.  out: n records of 32 x 60 words — register images (57 words each, 60-word slots) of P + Q, P + A, 2P, 2A,
 * to_affine(P) (with zz = zzz = R mod p), P stored to memory and loaded back, the 48 canonical words that store wrote, then
 * 24 chained steps from P: madd A, add Q, dbl, repeated. */
DR_API int dr_g1_ops_selftest(dr_ctx *ctx, const uint32_t *in /* n*192 */, size_t n, uint32_t *out /* n*1920 */);

/* ---- seam C: NTT over Fr ------------------------------------------------------------------------
 * Replaces BlsScalarNTTPlan.transform / transform_scaled (dot_ring/ring_proof/polynomial/ntt.pyx:104-163,
 * bls_scalar_ntt_round in bls12_381_scalar.c:333): `batch` in-place radix-2 transforms of size 2^log2n with
 * the primitive root `omega`; when scale != NULL every output is multiplied by it (inverse transform: pass
 * omega^-1 and n^-1).  data: batch * 2^log2n * 32 bytes, natural order in and out.
 */
DR_API int dr_ntt(dr_ctx *ctx, uint8_t *data, unsigned log2n, size_t batch, const uint8_t omega[32], const uint8_t *scale);
DR_API int dr_ntt_dev(dr_ctx *ctx, void *d_data, unsigned log2n, size_t batch, const uint8_t omega[32], const uint8_t *scale);
/* Diagnostic: the same transform in the ring prover's internal element formats, on RAW caller-supplied records, so that tests can
 * place operands on the edges of what each format admits.  Formats (fmt_in 0..3, fmt_out 0 or 1):
 *   0 STD8         8 little-endian words of the canonical value
 *   1 FS9          9 signed 32-bit limbs l_i, v = sum l_i 2^(29 i), standing for v 2^-261 mod p; as input: limbs 0..7 within
 *                  (-2^30, 2^30 + 2^29) and |v| < 3.3 p; as output: v = x 2^261 scale mod p in normal form with a scale, without
 *                  one limbs 0..7 in [0, 2^29) and |v| < 0.51 p
 *   2 STD8_SCALED  input only: transform x reads STD8 vector x / src_div of `src` and multiplies element i by record i of table
 *                  x % src_div of `in_scale` (src_div tables of FS9 records holding s R^2, R = 2^261)
 *   3 FS9_COSETS   input only: point idx of the vector is coset idx % 4, row idx / 4; `src` holds cosets 1..3 coset-major
 *                  ([transform][coset - 1][row], FS9), coset 0 is zero except its last three rows, `special` ([transform][3], FS9)
 * src holds 2^(log2n - pad) elements per source vector (zero-padded to 2^log2n in effect) and is never overwritten; out receives
 * batch * 2^log2n records of fmt_out.  omega and scale (NULL: none) as for dr_ntt.  The word counts must match the format exactly.
 * DR_ERR_INVALID, with nothing launched, for what the kernels do not cover: FS9 / FS9_COSETS input or FS9 output without a scale
 * above log2n = 16, FS9_COSETS below log2n = 4 or without `special`, STD8_SCALED without `in_scale` or with pad != 0. */
DR_API int dr_ntt_formats_selftest(dr_ctx *ctx, const uint32_t *src, size_t src_words, const uint32_t *in_scale, size_t in_scale_words,
                                   const uint32_t *special, size_t special_words, unsigned log2n, size_t batch, const uint8_t omega[32],
                                   const uint8_t *scale, int fmt_in, int fmt_out, int pad, uint32_t src_div, uint32_t *out);

/* ---- batched ring prover ---------------------------------------------------------------------------
 * Device-resident prover for MANY proofs over ONE ring (additive API): replaces the interpreted loops of
 * dot_ring/ring_proof/proof_builder.py:38-315, columns/columns.py:111-167 and constraints/constraints.py:43-151.
 * The Fiat-Shamir transcript stays on the host (hashlib), so proving is four phases, each ending where the
 * reference squeezes challenges; everything between the hashes stays in HBM.
 *   create    ring rows nm_points (N * 64 bytes, x||y LE; rows as built by Ring(): keys, padding, 2^i*B, 4 x (0,0)),
 *             omega_n / omega_4n primitive roots of the N and 4N domains, seed = accumulator base
 *   root      the three fixed-column commitments px, py, s (RingRoot.from_ring, vrf/ring/root.py:21-44)
 *   witness   in: producer row index and blinding factor per proof, optional 12 hidden-row values per proof
 *             (columns b, accip, accx, accy x 3 rows; NULL = test-vector mode, zeros)
 *             out: relation point Y_bar (x||y LE) and the four witness commitments (b, accip, accx, accy)
 *   quotient  in: seven alphas per proof; out: quotient commitment C_q
 *   evals     in: zeta per proof; out: px,py,s,b,accip,accx,accy at zeta and l(zeta*omega)   (8 x 32 bytes LE)
 *   openings  in: eight nus per proof; out: the two opening proofs (at zeta, at zeta*omega)
 * All four phase calls of one batch must use the same `batch`.  Scalars are 32-byte LE canonical field elements.
 */
typedef struct dr_ring_prover dr_ring_prover;
DR_API int dr_ring_prover_create(dr_ctx *ctx, const dr_srs *srs, unsigned log2n, uint32_t max_ring, const uint8_t omega_n[32],
                                 const uint8_t omega_4n[32], const uint8_t *nm_points_xy, const uint8_t seed_xy[64],
                                 dr_ring_prover **out);
/* the same for a ring whose keys live on `curve` (DR_CURVE_*): the constraint system uses that curve's coefficient a and
 * max_ring + bit length of its group order + 4 must fit the domain */
DR_API int dr_ring_prover_create_te(dr_ctx *ctx, int curve, const dr_srs *srs, unsigned log2n, uint32_t max_ring,
                                    const uint8_t omega_n[32], const uint8_t omega_4n[32], const uint8_t *nm_points_xy,
                                    const uint8_t seed_xy[64], dr_ring_prover **out);
DR_API void dr_ring_prover_destroy(dr_ring_prover *p);
DR_API int dr_ring_prover_root(const dr_ring_prover *p, uint8_t out_commitments[3 * 96], int is_inf[3]);
DR_API int dr_ring_prover_fixed_coeffs(dr_ring_prover *p, uint8_t *out /* 3*N*32: px, py, s coefficients */);
/* Diagnostic (like the *_selftest entries; nothing on the proving path calls it): reads back one polynomial of the batch in flight,
 * 32-byte LE standard-form coefficients, proof-major.  `what`:
 *   DR_RING_PEEK_COLUMNS   B * 4 * N * 32 bytes: the coefficients of b, accip, accx, accy; valid after dr_ring_prove_witness
 *   DR_RING_PEEK_QUOTIENT  B * (3N + 1) * 32 bytes: q, zero-padded; valid after dr_ring_prove_quotient
 *   DR_RING_PEEK_LIN       B * N * 32 bytes: the linearisation polynomial; valid after dr_ring_prove_evals
 * Waits for the context's stream and copies; the prover's state, the order of its phases included, is as before.  DR_ERR_INVALID for an
 * unknown selector, for out_bytes below the size above, and when the phase that fills the buffer has not run for the current batch or
 * the batch has been wiped (dr_ring_prove_openings ends with a wipe). */
enum { DR_RING_PEEK_COLUMNS = 0, DR_RING_PEEK_QUOTIENT = 1, DR_RING_PEEK_LIN = 2 };
DR_API int dr_ring_prover_peek(dr_ring_prover *p, int what, uint8_t *out, size_t out_bytes);
DR_API int dr_ring_prove_witness(dr_ring_prover *p, size_t batch, const uint32_t *producer_index, const uint8_t *blinding,
                                 const uint8_t *zk_rows, uint8_t *out_relation_xy, uint8_t *out_commitments, int *is_inf);
DR_API int dr_ring_prove_quotient(dr_ring_prover *p, size_t batch, const uint8_t *alphas, uint8_t *out_cq, int *is_inf);
DR_API int dr_ring_prove_evals(dr_ring_prover *p, size_t batch, const uint8_t *zetas, uint8_t *out_evals);
DR_API int dr_ring_prove_openings(dr_ring_prover *p, size_t batch, const uint8_t *nus, uint8_t *out_openings, int *is_inf);
/* Secrets do not stay in HBM.  dr_ring_prove_openings — the last phase of a batch — ends by zeroing the prover's per-batch state
 * (blinding factors, hidden rows, the witness columns with their bit column, every polynomial derived from them) and the MSM scratch
 * of its context; the batch entry points (dr_ringvrf_prove_batch, dr_pedersen_prove_batch, dr_ietf_prove_batch) also zero the device
 * copies of secret scalars and nonces.  The memsets are ordered behind the batch's last kernel on a stream of their own; the call does not
 * wait for them, and whatever uses the context next is ordered behind them on the device.  dr_ring_prover_wipe does the same on
 * request; dr_ring_prover_residue counts the non-zero 32-bit words left in those buffers (0 after a wipe; a test hook).
 * DOTRING_WIPE=0 disables the wipes (to measure their cost). */
DR_API int dr_ring_prover_wipe(dr_ring_prover *p);
DR_API int dr_ctx_scratch_residue(dr_ctx *ctx, uint64_t *words);    /* the same count for one context's scratch buffers */
DR_API int dr_ring_prover_residue(dr_ring_prover *p, uint64_t *words);


/* ---- native batch orchestration ------------------------------------------------------------------
 * The reference runs the hashing between the arithmetic steps of a proof in interpreted Python (hashlib):
 * hash_to_field (dot_ring/curve/curve.py:110-185), the VRF transcript / nonces / challenge
 * (dot_ring/vrf/primitives.py:26-122, pedersen/vrf.py:86-126) and the ring proof's Fiat-Shamir transcript
 * (ring_proof/transcript/transcript.py:21-136, phases.py:18-69).  For a batch that is ~40 small hashes per proof; here
 * they run on worker threads (DOTRING_HOST_THREADS, default min(16, cores)) inside ONE call per batch, with the GPU
 * phases above in between.  Results are byte-identical to prove() called per proof.
 */
enum { DR_HASH_SHA512 = 0, DR_HASH_SHAKE128 = 1, DR_HASH_SHAKE256 = 2,
       /* diagnostic: `data` = four messages of len / 4 bytes each, `out` = their four SHAKE128 digests of out_len / 4 bytes each
        * (at most 168), computed by the four-in-lockstep sponge the batch transcripts use */
       DR_HASH_SHAKE128_X4 = 3,
       DR_HASH_SHA256 = 4 };
DR_API int dr_host_hash(int kind, const uint8_t *data, size_t len, uint8_t *out, size_t out_len);
/* out = SHAKE256(seed || LE64(0))[0..576) || SHAKE256(seed || LE64(1))[0..576) || ... (len bytes), hashed on the worker threads.
 * dr_ringvrf_prove_batch's zk_random48 for a batch (12 x 48 bytes per proof: the hidden rows of columns/columns.py:139-146, drawn
 * with `secrets` in the reference) comes from one 32-byte OS seed this way. */
DR_API int dr_host_random_expand(const uint8_t seed[32], uint8_t *out, size_t len);
/* moves the secret part of dr_ringvrf_prove_batch's auxiliary records out: the 32-byte blinding factor of record i (offset 256
 * of its DR_RINGVRF_AUX_BYTES) is copied to out_blind + 32 i and zeroed in the record, so that what callers keep per batch holds
 * no secret and what they keep per proof is that proof's own factor only */
DR_API int dr_ringvrf_aux_take_blindings(uint8_t *aux, size_t batch, uint8_t *out_blind /* batch*32 */);

typedef struct dr_vrf_suite {
    const uint8_t *suite_id;        /* e.g. "Bandersnatch-SHA512-ELL2-v1" (bandersnatch.py:74-87) */
    size_t suite_id_len;
    int xof;                        /* 1: SHAKE128 suite, 0: SHA-512 (counter-mode squeeze, expand_message_xmd), 2: SHA-256 (counter-mode
                                       squeeze, the P-256 and secp256k1 suites); other values are refused.  The RFC 9380 suites hash to the
                                       field with the same hash: ids 6 - 9 want 2, ids 10 and 11 want 0 */
    uint8_t generator_xy[64];       /* group generator, x||y little-endian */
    uint8_t blinding_base_xy[64];   /* Pedersen blinding base (bandersnatch.py:89-102) */
    int curve;                      /* DR_CURVE_BANDERSNATCH (Elligator 2 hash-to-curve), DR_CURVE_JUBJUB, DR_CURVE_BANDERSNATCH_SW,
                                       DR_CURVE_ED25519, DR_CURVE_P256 or DR_CURVE_BABYJUBJUB (try-and-increment; for the SW suite and P-256 generator and
                                       blinding base are SW affine), DR_CURVE_SECP256K1 or DR_CURVE_SECP256K1_NU, DR_CURVE_P256_RO or
                                       DR_CURVE_P256_NU (RFC 9380 simplified SWU), DR_CURVE_ED25519_RO or DR_CURVE_ED25519_NU (RFC 9380
                                       Elligator 2) */
} dr_vrf_suite;

/* hash_to_field(msg, 2) for `count` messages msgs[off[i]..off[i+1]): out = count * 2 field elements (32-byte LE),
 * the input format of dr_bsn_encode_to_curve_batch.  For DR_CURVE_SECP256K1 the two elements are those of RFC 9380's
 * expand_message_xmd with SHA-256 (the input format of dr_secp256k1_map_to_curve with per_item = 2); for DR_CURVE_SECP256K1_NU it is
 * hash_to_field(msg, 1): ONE element, 32 bytes, per message.  DR_CURVE_P256_RO / DR_CURVE_ED25519_RO give the two elements of their
 * suites (SHA-256 with P-256's DST and modulus; SHA-512 with a 128-byte Z_pad, edwards25519's DST and 2^255 - 19), the input formats of
 * dr_p256_map_to_curve / dr_ed25519_map_to_curve; DR_CURVE_P256_NU / DR_CURVE_ED25519_NU one element.  Host only: no context. */
DR_API int dr_hash_to_field_batch(const dr_vrf_suite *suite, const uint8_t *msgs, const uint64_t *off /* count+1 */, size_t count,
                                  uint8_t *out_u_pairs);

/* encode_to_curve(salt_i || msg_i) for `count` messages (salts / salt_off nullable), whichever way the suite's curve hashes:
 * Elligator 2 (hash_to_field here + dr_bsn_encode_to_curve_batch) or try-and-increment (dot_ring/curve/point.py:252-296:
 * candidates hashed on worker threads, decompressed and cofactor-cleared on the GPU, several counters per launch) or, for
 * curve ids 6 - 11, RFC 9380 (hash_to_field on worker threads + one launch of the kernel of dr_secp256k1_map_to_curve,
 * dr_p256_map_to_curve or dr_ed25519_map_to_curve; DR_ERR_INVALID if a map has no value for a message). */
DR_API int dr_encode_to_curve_batch(dr_ctx *ctx, const dr_vrf_suite *suite, const uint8_t *msgs, const uint64_t *off /* count+1 */,
                                    const uint8_t *salts, const uint64_t *salt_off, size_t count, uint8_t *out_xy /* count*64 */);

/* RingVRF.prove for `batch` (<= 4096) proofs over the prover's ring: out_proofs = batch * 784 bytes
 * (Pedersen 192 || ring payload 592, dot_ring/vrf/ring/vrf.py:51-58).  alphas/ads/salts are concatenated with
 * (batch+1) offsets (salts may be NULL); secret_scalars batch*32 LE; producer_index = position of each signer's key in
 * the ring; fs_prefix = the bytes the ring-proof transcript has absorbed before "instance" (initial label and verifier
 * key, vrf/ring/root.py:54-72); zk_random48 = batch*12 48-byte random strings for the hidden rows (reduced mod p
 * here), or NULL for the deterministic test-vector mode.  out_aux (nullable, batch * DR_RINGVRF_AUX_BYTES): per proof
 * the affine Pedersen points O, Y_bar, R, O_k (4*64), the blinding factor (32) and the seven G1 commitments
 * serialised uncompressed (7*96: C_b, C_accip, C_accx, C_accy, C_q, Phi_zeta, Phi_zeta_omega). */
#define DR_RINGVRF_AUX_BYTES 960
DR_API int dr_ringvrf_prove_batch(dr_ring_prover *p, const dr_vrf_suite *suite, size_t batch, const uint8_t *alphas,
                                  const uint64_t *alpha_off, const uint8_t *ads, const uint64_t *ad_off, const uint8_t *salts,
                                  const uint64_t *salt_off, const uint8_t *secret_scalars, const uint32_t *producer_index,
                                  const uint8_t *fs_prefix, size_t fs_prefix_len, const uint8_t *zk_random48, uint8_t *out_proofs,
                                  uint8_t *out_aux);


/* PedersenVRF.prove / batch_verify for a batch (dot_ring/vrf/pedersen/vrf.py:86-126, 171-242): the Pedersen halves of the
 * two Ring-VRF calls on their own.  Proofs are 4 points and 2 scalars (gamma || Y_bar || R || O_k || s || s_b): the size per suite, 192
 * bytes for the TE suites, 196 for DR_CURVE_BANDERSNATCH_SW (whose aux points are SW affine).  out_aux (nullable,
 * batch * DR_PEDERSEN_AUX_BYTES): O, Y_bar, R, O_k affine (4*64) and the blinding factor (32).  The verifier decodes and
 * subgroup-checks the proof points on the GPU; *ok = 1 iff every proof verifies (malformed input: *ok = 0, DR_OK). */
#define DR_PEDERSEN_AUX_BYTES 288
DR_API int dr_pedersen_prove_batch(dr_ctx *ctx, const dr_vrf_suite *suite, size_t batch, const uint8_t *alphas, const uint64_t *alpha_off,
                                   const uint8_t *ads, const uint64_t *ad_off, const uint8_t *salts, const uint64_t *salt_off,
                                   const uint8_t *secret_scalars, uint8_t *out_proofs, uint8_t *out_aux);
DR_API int dr_pedersen_verify_batch(dr_ctx *ctx, const dr_vrf_suite *suite, size_t batch, const uint8_t *proofs, const uint8_t *inputs,
                                    const uint64_t *in_off, const uint8_t *ads, const uint64_t *ad_off, const uint8_t *salts,
                                    const uint64_t *salt_off, int *ok);

/* TinyVRF.prove (thin = 0: proofs O || c || s, 80 bytes for the TE suites, dot_ring/vrf/ietf/tiny.py:35-70) or ThinVRF.prove (thin = 1:
 * O || R || s, 96 bytes) for a batch — sizes per suite: 81 / 98 bytes for DR_CURVE_BANDERSNATCH_SW (aux points SW affine); arguments as for dr_pedersen_prove_batch.  out_aux (nullable, batch * 128): O and R affine. */
DR_API int dr_ietf_prove_batch(dr_ctx *ctx, const dr_vrf_suite *suite, int thin, size_t batch, const uint8_t *alphas,
                               const uint64_t *alpha_off, const uint8_t *ads, const uint64_t *ad_off, const uint8_t *salts,
                               const uint64_t *salt_off, const uint8_t *secret_scalars, uint8_t *out_proofs, uint8_t *out_aux);

/* TinyVRF.verify / ThinVRF.verify (dot_ring/vrf/ietf/tiny.py:72-88, thin.py:96-118) for `batch` ENCODED proofs (80 bytes O || c || s, or
 * 96 bytes O || R || s with thin = 1), proof i under the compressed public key public_keys[32 i ..]: verdict[i] = 1 verifies, 0 does
 * not, 2 the public key does not decode to a prime-order point, 3 the proof is malformed (a point that does not decode, a scalar >= n)
 * — the cases the reference raises ValueError for.  Each proof is checked on its own, one per worker thread, on HOST cores: this is the
 * single-proof entry point (one proof: ~0.6 ms against three kernel launch chains); the relation of MANY Thin proofs at once is
 * ThinVRF.batch_verify's one MSM on the GPU (dr_te_msm).  Elligator suites of Bandersnatch only.
 *
 * Small calls in general: up to DOTRING_SMALL_HOST_MAX proofs (default 64; 0 = never) dr_ietf_prove_batch, dr_pedersen_prove_batch and
 * dr_pedersen_verify_batch run the same protocol on host cores too (csrc/hostsigma.hpp) — secret scalars on fixed-schedule
 * multiplications — and give the same bytes and verdicts as the kernels. */
DR_API int dr_ietf_verify_batch(dr_ctx *ctx, const dr_vrf_suite *suite, int thin, size_t batch, const uint8_t *proofs,
                                const uint8_t *public_keys /* batch*32 */, const uint8_t *inputs, const uint64_t *in_off, const uint8_t *ads,
                                const uint64_t *ad_off, const uint8_t *salts, const uint64_t *salt_off, uint8_t *verdict /* batch */);

/* What a verifier knows about one ring (RingRoot + RingProofParams + SRS verifier part). */
typedef struct dr_ring_verifier_key {
    unsigned log2n;                      /* domain size N = 2^log2n */
    uint8_t omega_n[32];                 /* primitive N-th root of unity, LE */
    uint8_t seed_xy[64];                 /* accumulator base point (bandersnatch.py:89-102), x||y LE */
    uint8_t fixed_commitments[3 * 96];   /* C_px, C_py, C_s serialised uncompressed (BE x||y; infinity = 0x40 || 0) */
    uint8_t g1_generator[96];            /* SRS G1[0], BE x||y */
    uint8_t g2[2 * 192];                 /* SRS [1]G2, [tau]G2 in file byte order (pcs/srs.py:78-88) */
    const uint8_t *fs_prefix;            /* as for dr_ringvrf_prove_batch */
    size_t fs_prefix_len;
} dr_ring_verifier_key;

/* RingVRF.batch_verify (dot_ring/vrf/ring/vrf.py:239-283) over `batch` (<= 4096) ENCODED proofs (784 bytes each):
 * decoding and validating every point (Bandersnatch: canonical, on curve, prime-order subgroup; G1: zcash
 * decompression) runs on the GPU, the transcript replay and the verifier's scalar pass on worker threads, then one
 * (5B+2)-point Bandersnatch MSM (Pedersen part) and two G1 MSMs + one pairing equation (ring part).  seed32 = fresh
 * verifier randomness for the random linear combination.  *ok = 1 iff every proof verifies; malformed proofs give
 * *ok = 0 with DR_OK. */
DR_API int dr_ringvrf_verify_batch(dr_ctx *ctx, const dr_vrf_suite *suite, const dr_ring_verifier_key *vk, size_t batch,
                                   const uint8_t *proofs, const uint8_t *inputs, const uint64_t *in_off, const uint8_t *ads,
                                   const uint64_t *ad_off, const uint8_t *salts, const uint64_t *salt_off,
                                   const uint8_t seed32[32], int *ok);

/* ---- one batch over several GPUs of ONE process (SURVEY 8(b) additive row: a device set instead of one device; 8(e) first mode) -----
 * The same two calls over a set of devices: provers[g] / ctxs[g] live on the devices the caller chose (dr_ctx_create(device_id), one
 * dr_srs and one dr_ring_prover of the SAME ring per device — the SRS and the per-ring tables are replicated in each HBM, < 250 MB).
 * Device g takes proofs [g B / G, (g + 1) B / G) (sizes differ by at most one; B < G leaves shards empty) on a host thread of its own
 * and writes its results straight into the caller's buffers: all B proofs come back in order, byte-identical to the one-device call
 * (in test-vector mode; with hidden rows, zk_random48 is consumed by proof index, so the bytes do not depend on G either).  No collective
 * and no exchange between the devices.  The verifier ANDs the shards' verdicts; every shard folds with randomness of its own derived
 * from seed32.  Entries of the set may be several contexts on ONE device (how the one-GPU tests run it).  The host worker pool
 * (DOTRING_HOST_THREADS) is shared by the shards: give it about 16 threads per device.
 * One process PER GPU (torch.distributed / any launcher) shards the same way through dot_ring_amd.parallel.prove_batch_sharded, with the
 * 784-byte proofs gathered over the communicator; the reference's own multi-worker shape is tests/benchmark/bench_ring_proof.py:168-182. */
DR_API int dr_ringvrf_prove_batch_multi(dr_ring_prover *const *provers, size_t n_provers, const dr_vrf_suite *suite, size_t batch,
                                        const uint8_t *alphas, const uint64_t *alpha_off, const uint8_t *ads, const uint64_t *ad_off,
                                        const uint8_t *salts, const uint64_t *salt_off, const uint8_t *secret_scalars,
                                        const uint32_t *producer_index, const uint8_t *fs_prefix, size_t fs_prefix_len,
                                        const uint8_t *zk_random48, uint8_t *out_proofs, uint8_t *out_aux);
DR_API int dr_ringvrf_verify_batch_multi(dr_ctx *const *ctxs, size_t n_ctxs, const dr_vrf_suite *suite, const dr_ring_verifier_key *vk,
                                         size_t batch, const uint8_t *proofs, const uint8_t *inputs, const uint64_t *in_off,
                                         const uint8_t *ads, const uint64_t *ad_off, const uint8_t *salts, const uint64_t *salt_off,
                                         const uint8_t seed32[32], int *ok);

/* ---- RingVRF.verify_each: a verdict PER PROOF from one batch pass -----
 * dr_ringvrf_verify_batch answers with one bit; this call says which proofs fail.  Same arguments, refusals and phases; then
 *  - a malformed proof (non-canonical scalar, a point that does not decode, zeta inside the domain) no longer rejects the call:
 *    its verdict is 0 and it leaves the combination (scalars zero, undecodable points the identity);
 *  - ring part: per proof the claim points L_i (seven claim scalars on its own points, four on C_px, C_py, C_s, G1[0]) and
 *    R_i (r1, r2 on its opening proofs) and the tree of their subset sums are computed on the GPU (csrc/kernels_g1_claims.hip.h) and
 *    downloaded in one copy; e(L, G2[0]) e(-R, G2[1]) == 1 is tested at the root — if it holds, every proof left in passes with ONE
 *    equation, as in batch_verify — and otherwise down the tree, only below nodes that fail (csrc/verify_tree.hpp);
 *  - Pedersen part: per proof exactly, O_k = s I - c O and R = s G + s_b B - c Y_bar, 2 * batch groups of three terms in one launch.
 * verdicts[i] = 1 iff proof i verifies.  stats (nullable, 4 words): [0] pairing equations evaluated, [1] proofs excluded before
 * the fold, [2] depth of the tree (ceil(log2 batch)), [3] reserved, 0.  Up to DOTRING_VERIFY_HOST_MAX proofs the points and
 * the tree come from the host route of dr_ringvrf_verify_batch.  The _multi form shards as dr_ringvrf_verify_batch_multi does: every
 * shard writes its slice of `verdicts`; stats are summed, the depth is the largest. */
DR_API int dr_ringvrf_verify_each(dr_ctx *ctx, const dr_vrf_suite *suite, const dr_ring_verifier_key *vk, size_t batch,
                                  const uint8_t *proofs, const uint8_t *inputs, const uint64_t *in_off, const uint8_t *ads,
                                  const uint64_t *ad_off, const uint8_t *salts, const uint64_t *salt_off,
                                  const uint8_t seed32[32], uint8_t *verdicts /* batch */, uint32_t *stats /* nullable, 4 words */);
DR_API int dr_ringvrf_verify_each_multi(dr_ctx *const *ctxs, size_t n_ctxs, const dr_vrf_suite *suite, const dr_ring_verifier_key *vk,
                                        size_t batch, const uint8_t *proofs, const uint8_t *inputs, const uint64_t *in_off,
                                        const uint8_t *ads, const uint64_t *ad_off, const uint8_t *salts, const uint64_t *salt_off,
                                        const uint8_t seed32[32], uint8_t *verdicts, uint32_t *stats);

/* Diagnostic: the claim-point and tree kernels on caller-supplied groups.  `groups` (1..4096) groups of m (1..64) terms: points
 * affine standard-form little-endian x || y (96 bytes, coordinates below p, all zero = infinity), scalars 32 bytes little-endian,
 * any value below 2^256.  Leaf g is the sum of its group's m terms.  Node array: 2 * Bp - 1 nodes, Bp = groups rounded up to a power
 * of two (the padding leaves are the identity), in heap order — node 0 is the root, the children of node k are 2k + 1 and 2k + 2,
 * leaf g is node Bp - 1 + g.  out_nodes_le_xy: 96 bytes per node as the input points; out_inf: one byte per node, 1 for the identity. */
DR_API int dr_g1_claim_tree_selftest(dr_ctx *ctx, const uint8_t *pts_le_xy /* groups*m*96 */, const uint8_t *scalars /* groups*m*32 */,
                                     size_t groups, size_t m, uint8_t *out_nodes_le_xy /* (2*Bp-1)*96 */, uint8_t *out_inf /* 2*Bp-1 */);

#ifdef __cplusplus
}
#endif
#endif /* DOTRING_HIP_H */
