"""Curve layer of the API mirror: the Bandersnatch suites (and JubJub), points, codecs, hash-to-curve.

Mirrors (names, argument meaning, error behaviour) the parts of the reference the Ring-VRF path touches:
  dot_ring/curve/specs/bandersnatch.py:57-306   suites, BandersnatchPoint.__mul__/msm, CurveVariant objects
  dot_ring/curve/specs/jubjub.py:17-66          JubJub: same field, a = -1, cofactor 8, try-and-increment
  dot_ring/curve/specs/bandersnatch_sw.py       Bandersnatch_SW: Bandersnatch's group in short Weierstrass form, 33-byte codec,
                                                try-and-increment; the kernels compute on its twisted Edwards image
  dot_ring/curve/specs/p256.py                  P256 (= P256_TAI): NIST P-256, its own field, 33-byte codec with a SEC1 fallback,
                                                try-and-increment with SHA-256; kernels of their own (DR_CURVE_P256)
  dot_ring/curve/specs/secp256k1.py             Secp256k1 (= Secp256k1_RO), Secp256k1_NU: its own field, plain SEC1 33-byte codec, RFC 9380
                                                hashing to the curve (SHA-256 XMD, simplified SWU, 3-isogeny); kernels of their own
                                                (DR_CURVE_SECP256K1 / DR_CURVE_SECP256K1_NU)
  dot_ring/curve/specs/baby_jubjub.py           BabyJubJub: a = 1 over the BN254 scalar field, cofactor 8, try-and-increment with
                                                SHA-512 (candidates masked to the field's 254 bits); kernels of their own (DR_CURVE_BABYJUBJUB)
  dot_ring/curve/specs/curve25519.py            Curve25519 (= Curve25519_RO), Curve25519_NU: Montgomery affine points over Ed25519's field,
                                                64-byte u || v codec, RFC 9380 Elligator 2 with SHA-512; kernels of their own over the
                                                Ed25519 group law (DR_CURVE_CURVE25519_RO / _NU)
  dot_ring/curve/specs/ed448.py                 Ed448 (= Ed448_RO), Ed448_NU: a = 1, d = -39081 over 2^448 - 2^224 - 1, cofactor 4, 112-byte
                                                x || y codec, 56-byte scalars, RFC 9380 Elligator 2 with SHAKE256; kernels of their own
                                                (DR_CURVE_ED448_RO / _NU), the first suite wider than 256 bits in both
  dot_ring/curve/specs/curve448.py              Curve448 (= Curve448_RO), Curve448_NU: Montgomery affine points over Ed448's field, 112-byte
                                                u || v codec, 56-byte scalars, RFC 9380 Elligator 2 with SHAKE256; kernels of their own on
                                                the Edwards curve birational to it (DR_CURVE_CURVE448_RO / _NU)
  dot_ring/curve/point.py:150-214               compressed codec
  dot_ring/curve/twisted_edwards/*              affine law, Elligator2 encode_to_curve
  dot_ring/curve/curve.py:56-67,110-237,384-401 valid_point, hash_to_field, key derivation
Scalar multiplications and MSMs run on the GPU (seam A of include/dotring_hip.h); single affine additions,
hashing and the Elligator map stay host-side big-int code exactly as they are in the reference.
"""
from __future__ import annotations

import dataclasses
import hashlib
from dataclasses import dataclass
from typing import Callable

from . import _native, runtime

FIELD_MODULUS = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
SUBGROUP_ORDER = 0x1CFB69D4CA675F520CCE760202687600FF8F87007419047174FD06B52876E7E1
_P, _N = FIELD_MODULUS, SUBGROUP_ORDER
_A = -5
_D = 0x6389C12633C267CBC66E3BF86BE3B6D8CB66677177E54F92B369F2F5188D58E7


@dataclass(frozen=True)
class AuxiliaryPoints:
    blinding_base: tuple
    accumulator_base: tuple
    padding_point: tuple


@dataclass(frozen=True)
class Encoding:
    endian: str = "little"
    point_len: int = 32
    challenge_len: int = 16
    uncompressed: bool = False


@dataclass(frozen=True)
class SuiteParams:
    """The fields of the reference's BandersnatchParams that callers read (bandersnatch.py:46-106)."""
    suite_id: bytes
    hash_fn: Callable
    auxiliary_points: AuxiliaryPoints
    xof: bool
    field_modulus: int = FIELD_MODULUS
    subgroup_order: int = SUBGROUP_ORDER
    cofactor: int = 4
    a: int = _A
    d: int = _D
    generator: tuple = (
        18886178867200960497001835917649091219057080094937609519140440539760939937304,
        19188667384257783945677642223292697773471335439753913231509108946878080696678,
    )
    encoding: Encoding = Encoding()
    curve_id: int = _native.CURVE_BANDERSNATCH      # DR_CURVE_* of include/dotring_hip.h
    e2c: str = "ell2"                               # "ell2" / "ell2_nu" (Elligator 2), "tai" (try and increment), "sswu" / "sswu_nu" (RFC 9380)

    @property
    def h2c_dst(self) -> bytes:
        return self.suite_id + b"\x60"


def _sqrt_5mod8(v: int, p: int) -> int:
    """a square root mod p = 5 (mod 8) (Ed25519's field), host big-int code as the reference's curve.mod_sqrt"""
    if v == 0:
        return 0
    r = pow(v, (p + 3) // 8, p)
    if r * r % p != v:
        r = r * pow(2, (p - 1) // 4, p) % p
    if r * r % p != v:
        raise ValueError("No square root exists")
    return r


def _sqrt_tonelli_shanks(v: int, p: int) -> int:
    """a square root mod p by Tonelli-Shanks (the reference's curve.mod_sqrt; Baby JubJub's field, p - 1 = Q 2^28), host big-int code"""
    v %= p
    if v == 0:
        return 0
    if pow(v, (p - 1) // 2, p) != 1:
        raise ValueError("No square root exists")
    q, s = p - 1, 0
    while q % 2 == 0:
        q, s = q // 2, s + 1
    z = 2
    while pow(z, (p - 1) // 2, p) != p - 1:
        z += 1
    m, c, t, r = s, pow(z, q, p), pow(v, q, p), pow(v, (q + 1) // 2, p)
    while t != 1:
        i, t2 = 1, t * t % p
        while t2 != 1:
            i, t2 = i + 1, t2 * t2 % p
        b = pow(c, 1 << (m - i - 1), p)
        m, c, t, r = i, b * b % p, t * b * b % p, r * b % p
    return r


class _Rfc9380:
    """Hashing to the curve by RFC 9380 as every suite here does it: hash_to_field natively on the host, the map on the GPU.  The default
    hooks are the 256-bit suites' (the library's dr_vrf_suite entry points); a class supplies what differs:
      _mapped(us, per_item)       the device half: points for packed field elements, per_item of them each
      _hash_to_field(msgs)        the library's hash_to_field for many messages, packed little-endian
      _encoded(msgs, salts)       the library's encode_to_curve for many messages, unpacked"""
    __slots__ = ()

    @classmethod
    def _per_item(cls) -> int:
        return 1 if cls.curve.params.e2c.endswith("_nu") else 2

    @classmethod
    def _hash_to_field(cls, msgs) -> bytes:
        return _native.hash_to_field_batch(cls._suite_struct(), msgs)

    @classmethod
    def _encoded(cls, msgs, salts):
        # (a message whose image has no value comes back as DR_ERR_INVALID: a ValueError, as the reference's failing step is)
        return unpack_points(cls, runtime.context().encode_to_curve_batch(cls._suite_struct(), msgs, salts))

    @classmethod
    def hash_to_field_pairs(cls, alpha_strings, salts=None) -> bytes:
        """Host half of encode_to_curve for many inputs: two field elements per input (one for the NU variant), packed little-endian."""
        salts = salts or [b""] * len(alpha_strings)
        return cls._hash_to_field([bytes(s) + bytes(a) for a, s in zip(alpha_strings, salts)])

    @classmethod
    def encode_to_curve_from_field(cls, us: bytes):
        """Device half: the maps, for RO the sum of the two images, and the cofactor, for packed canonical field elements."""
        return cls._mapped(us, cls._per_item()) if us else []

    @classmethod
    def encode_to_curve(cls, alpha_string: bytes, salt: bytes = b""):
        return cls.encode_to_curve_batch([alpha_string], [salt])[0]

    @classmethod
    def encode_to_curve_batch(cls, alpha_strings, salts=None):
        return cls._encoded(list(alpha_strings), salts) if alpha_strings else []


class _WideRfc9380(_Rfc9380):
    """... over a wide suite's own entry points (_native._WIDE): the class names its suite (_SUITE), unpacks the points (_unpack) and words
    the refusal of a field element without an image as the reference's failing step does (_NO_IMAGE)."""
    __slots__ = ()

    @classmethod
    def _mapped(cls, us: bytes, per_item: int, clear: bool = True):
        raw, ok = runtime.context()._wide_map_to_curve(cls._SUITE, us, per_item, clear)
        if 0 in ok:
            raise ValueError(cls._NO_IMAGE)
        return cls._unpack(raw)

    @classmethod
    def _hash_to_field(cls, msgs) -> bytes:
        return _native._wide_hash_to_field_batch(cls._SUITE, cls.curve.params.curve_id, msgs)

    @classmethod
    def _encoded(cls, msgs, salts):
        return cls._unpack(runtime.context()._wide_encode_to_curve_batch(cls._SUITE, cls.curve.params.curve_id, msgs, salts))


class BandersnatchCurve:
    def __init__(self, params: SuiteParams):
        self.params = params

    # -- curve.py:110-237
    def hash_to_field(self, msg: bytes, count: int) -> list[int]:
        if count < 0:
            raise ValueError("Count must be non-negative")
        if msg is None:
            raise ValueError("Message cannot be None")
        length = 48 * count
        dst_prime = self.params.h2c_dst + bytes([len(self.params.h2c_dst)])
        if self.params.xof:
            raw = hashlib.shake_128(msg + length.to_bytes(2, "big") + dst_prime).digest(length)
        else:
            # expand_message_xmd with SHA-512; Z_pad is 48 zero bytes in this suite (bandersnatch.py:85, curve.py:170)
            b0 = hashlib.sha512(bytes(48) + msg + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
            blocks = [hashlib.sha512(b0 + b"\x01" + dst_prime).digest()]
            for i in range(2, -(-length // 64) + 1):
                blocks.append(hashlib.sha512(bytes(x ^ y for x, y in zip(b0, blocks[-1])) + bytes([i]) + dst_prime).digest())
            raw = b"".join(blocks)[:length]
        return [int.from_bytes(raw[48 * i : 48 * i + 48], "big") % _P for i in range(count)]

    def mod_sqrt(self, val: int) -> int:
        p = self.params.field_modulus
        if p == _P:
            return _native.fr_sqrt(val % _P)    # raises ValueError("No square root exists")
        if p % 4 == 3:                          # P-256's field
            r = pow(val % p, (p + 1) // 4, p)
            if r * r % p != val % p:
                raise ValueError("No square root exists")
            return r
        if p % 8 == 5:                          # Ed25519's field
            return _sqrt_5mod8(val % p, p)
        return _sqrt_tonelli_shanks(val, p)     # Baby JubJub's

    def is_square(self, val: int) -> bool:
        p = self.params.field_modulus
        val %= p
        return val == 0 or pow(val, (p - 1) // 2, p) == 1

    def valid_point(self, point: "BandersnatchPoint") -> bool:
        """Non-identity member of the prime-order subgroup (curve.py:56)."""
        return bool(valid_points([point])[0])


class _AffinePoint:
    """Root of every point type: two coordinates and what no curve form changes.  A family below it (twisted Edwards, short
    Weierstrass, Montgomery, E(Fq2)) gives __init__, _on_curve, _trusted, __eq__ with __hash__, __add__ and __neg__; a concrete class
    gives `curve`, _N, _H, _CV, its codec and whatever runs on kernels of its own.  The identity is (None, None) unless a family says
    otherwise."""
    curve: BandersnatchCurve
    _WIDE = False                     # coordinates or scalars wider than the 64-byte entry points': the class brings its own hooks
    _IDENTITY_BYTES = bytes(64)       # how pack_points sends an identity whose coordinates are None
    __slots__ = ("x", "y")

    def __repr__(self):
        return f"{type(self).__name__}({self.x}, {self.y})"

    @classmethod
    def identity(cls):
        return cls(None, None)

    @classmethod
    def generator_point(cls):
        return cls(*cls.curve.params.generator)

    def is_identity(self) -> bool:
        return self.x is None and self.y is None

    def is_on_curve(self) -> bool:
        return self.is_identity() or self._on_curve(self.x, self.y)

    def __sub__(self, other):
        return self + (-other)

    # -- scalar multiplication / MSM on the GPU
    def __mul__(self, scalar: int):
        return scalar_mul_batch([self], [scalar])[0]

    __rmul__ = __mul__

    @classmethod
    def msm(cls, points, scalars):
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        if not points:
            return cls.identity()
        raw = runtime.context().bsn_msm(pack_points(points), pack_scalars(scalars, cls._N), cls._CV)
        return cls._trusted(int.from_bytes(raw[:32], "little"), int.from_bytes(raw[32:], "little"))

    @classmethod
    def _suite_struct(cls):
        """dr_vrf_suite of this point type's suite (cached on the class)."""
        st = cls.__dict__.get("_suite_cache")
        if st is None:
            sp = cls.curve.params
            le = lambda pt: pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little")  # noqa: E731
            st = _native.vrf_suite(sp.suite_id, sp.hash_fn, le(sp.generator), le(sp.auxiliary_points.blinding_base), sp.curve_id)
            cls._suite_cache = st
        return st

    # -- what the module-level batch helpers ask a point type: here over the 64-byte entry points, a wide type has its own
    @classmethod
    def _scalar_mul_batch(cls, points, scalars):
        first = points[0]
        if all(p is first for p in points) and (first.x, first.y) in _fixed_bases(cls):
            # k_i * G (key derivation, curve.py:384) or k_i * B: the constant's fixed-base window table — 64 table additions
            # over four lanes instead of ~250 dependent doublings (dr_te_fixed_base_msm_groups)
            raw = runtime.context().te_fixed_base_msm_groups(pack_points([first]), pack_scalars(scalars, cls._N), cls._CV)
            return unpack_points(cls, raw)
        raw = runtime.context().bsn_scalar_mul_batch(pack_points(points), pack_scalars(scalars, cls._N), cls._CV)
        return unpack_points(cls, raw)

    @classmethod
    def _msm_groups(cls, points, scalars, m: int):
        raw = runtime.context().bsn_msm_groups(pack_points(points), pack_scalars(scalars, cls._N), m, cls._CV)
        return unpack_points(cls, raw)

    @classmethod
    def _valid_points(cls, points) -> list[bool]:
        """[h]P != O and [h^-1 mod n][h]P == P (h the cofactor), one launch for all points"""
        live = [i for i, p in enumerate(points) if not p.is_identity() and p.is_on_curve()]
        out = [False] * len(points)
        if not live:
            return out
        h, order = type(points[live[0]])._H, type(points[live[0]])._N
        if h == 1:                               # prime order (P-256, secp256k1): on the curve and not the identity (curve.py:61)
            for i in live:
                out[i] = True
            return out
        cleared = scalar_mul_batch_raw([points[i] for i in live], [h] * len(live))
        back = scalar_mul_batch([c for c in cleared], [pow(h, -1, order)] * len(live))
        for i, c, b in zip(live, cleared, back):
            out[i] = (not c.is_identity()) and b == points[i]
        return out


class BandersnatchPoint(_AffinePoint):
    """Affine twisted Edwards point, the identity (0, 1); `curve` and the coefficient shortcuts are bound per suite by the subclasses
    below (the class keeps its Bandersnatch name: that is what the reference's callers import)."""
    _A, _D, _N, _H, _CV = _A, _D, _N, 4, _native.CURVE_BANDERSNATCH
    _P = _P                       # the suite's base field (Ed25519's differs)
    __slots__ = ()

    def __init__(self, x: int, y: int):
        self.x, self.y = x, y
        if (x, y) != (0, 1):
            if not (0 <= x < self._P and 0 <= y < self._P):
                raise ValueError("Invalid point coordinates")
            if not self._on_curve(x, y):
                raise ValueError("Point is not on the curve")

    @classmethod
    def _on_curve(cls, x: int, y: int) -> bool:
        p = cls._P
        return (cls._A * x * x + y * y) % p == (1 + cls._D * x * x % p * y * y) % p

    @classmethod
    def _trusted(cls, x: int, y: int):
        """Construct from coordinates that are already known to be on the curve (kernel outputs): skips the
        range / on-curve checks of __init__."""
        pt = object.__new__(cls)
        pt.x, pt.y = x, y
        return pt

    # -- basics
    def __eq__(self, other):
        return isinstance(other, BandersnatchPoint) and self.x == other.x and self.y == other.y

    def __hash__(self):
        return (self.x + self.y) % self._N

    @classmethod
    def identity(cls):
        return cls(0, 1)

    def is_identity(self) -> bool:
        return self.x == 0 and self.y == 1

    # -- group law: single additions are host big-int code, as in te_affine_point.py:69-167
    def __add__(self, other):
        if not isinstance(other, BandersnatchPoint):
            raise TypeError("Can only add TEAffinePoints")
        if self.is_identity():
            return other
        if other.is_identity():
            return self
        if self == other:
            return self.double()
        x1, y1, x2, y2 = self.x, self.y, other.x, other.y
        a, d, p = self._A, self._D, self._P
        t = d * x1 % p * x2 % p * y1 % p * y2 % p
        return type(self)((x1 * y2 + x2 * y1) * pow(1 + t, -1, p) % p, (y1 * y2 - a * x1 * x2) * pow(1 - t, -1, p) % p)

    def double(self):
        x1, y1, a, p = self.x, self.y, self._A, self._P
        if y1 == 0:
            return self.identity()
        dx, dy = (a * x1 * x1 + y1 * y1) % p, (2 - a * x1 * x1 - y1 * y1) % p
        if dx == 0 or dy == 0:
            return self.identity()
        return type(self)(2 * x1 * y1 * pow(dx, -1, p) % p, (y1 * y1 - a * x1 * x1) * pow(dy, -1, p) % p)

    def __neg__(self):
        return type(self)(-self.x % self._P, self.y)

    @classmethod
    def msm(cls, points, scalars):
        s = super().msm(points, scalars)
        return cls(s.x, s.y)             # (through the checking constructor, as the reference's)

    # -- codec (point.py:150-214)
    def point_to_string(self) -> bytes:
        raw = bytearray(self.y.to_bytes(32, "little"))
        if self.x > -self.x % self._P:
            raw[31] |= 0x80
        return bytes(raw)

    @classmethod
    def string_to_point(cls, octet_string: bytes):
        if not octet_string:
            raise ValueError("Empty octet string")
        sign = (octet_string[-1] >> 7) & 1
        raw = bytearray(octet_string)
        raw[-1] &= 0x7F
        y, p = int.from_bytes(raw, "little"), cls._P
        if y >= p:
            raise ValueError("Invalid point encoding")
        den = (cls._A - cls._D * y * y) % p
        if den == 0:
            raise ValueError("Invalid point encoding")
        try:
            x = cls.curve.mod_sqrt((1 - y * y) * pow(den, -1, p) % p)
        except ValueError:
            raise ValueError("Invalid point encoding") from None
        lo, hi = sorted((x, -x % p))
        return cls(hi if sign else lo, y)

    # -- hash to curve (te_affine_point.py:212-295, te_curve.py:48-95)
    @classmethod
    def encode_to_curve(cls, alpha_string: bytes, salt: bytes = b""):
        if cls.curve.params.e2c == "tai":          # point.py:252-296, through the batch entry point (hashing native, sqrt on the GPU)
            return cls.encode_to_curve_batch([alpha_string], [salt])[0]
        u0, u1 = cls.curve.hash_to_field(salt + alpha_string, 2)
        r = cls.map_to_curve(u0) + cls.map_to_curve(u1)
        return r.double().double()

    @classmethod
    def hash_to_field_pairs(cls, alpha_strings, salts=None) -> bytes:
        """Host half of encode_to_curve for many inputs: two field elements per input, packed little-endian."""
        salts = salts or [b""] * len(alpha_strings)
        return b"".join(u.to_bytes(32, "little") for a, s in zip(alpha_strings, salts) for u in cls.curve.hash_to_field(s + a, 2))

    @classmethod
    def encode_to_curve_from_field(cls, us: bytes):
        """Device half: Elligator2 maps, addition and cofactor clearing for packed (u0, u1) pairs."""
        if not us:
            return []
        return unpack_points(cls, runtime.context().bsn_encode_to_curve_batch(us))

    @classmethod
    def encode_to_curve_batch(cls, alpha_strings, salts=None):
        """encode_to_curve for many inputs: hash_to_field on the host, Elligator2 + cofactor clearing on the GPU; for a
        try-and-increment suite the candidates are hashed natively and decompressed + cofactor-cleared on the GPU."""
        if cls.curve.params.e2c == "tai":
            if not alpha_strings:
                return []
            return unpack_points(cls, runtime.context().encode_to_curve_batch(cls._suite_struct(), list(alpha_strings), salts))
        return cls.encode_to_curve_from_field(cls.hash_to_field_pairs(alpha_strings, salts))

    @classmethod
    def map_to_curve(cls, u: int):
        inv_den = pow((_A - _D) % _P, -1, _P)
        mont_a, mont_b = 2 * (_A + _D) * inv_den % _P, 4 * inv_den % _P
        a_over_b = mont_a * pow(mont_b, -1, _P) % _P
        inv_b2 = pow(mont_b * mont_b % _P, -1, _P)
        tv1 = 5 * u * u % _P
        if tv1 == _P - 1:
            tv1 = 0
        x1 = -a_over_b * pow(tv1 + 1, -1, _P) % _P
        gx1 = ((x1 + a_over_b) * x1 + inv_b2) * x1 % _P
        e2 = cls.curve.is_square(gx1)
        x, y2 = (x1, gx1) if e2 else ((-x1 - a_over_b) % _P, tv1 * gx1 % _P)
        y = cls.curve.mod_sqrt(y2)
        if e2 ^ (y % 2 == 1):
            y = -y % _P
        s, t = x * mont_b % _P, y * mont_b % _P
        # Montgomery (s,t) -> twisted Edwards (v,w)
        tv1 = (s + 1) % _P
        tv2 = tv1 * t % _P
        tv2 = pow(tv2, -1, _P) if tv2 else 0
        v, w = tv2 * tv1 % _P * s % _P, tv2 * t % _P * (s - 1) % _P
        return cls(v, 1 if tv2 == 0 else w)


class _ShortWeierstrassPoint(_AffinePoint):
    """Affine point of y^2 = x^3 + a x + b over the integers mod _P (short_weierstrass/sw_affine_point.py), the identity (None, None):
    the constructor's checks, equality and the host big-int group law.  A subclass gives _P, _SW_A, _SW_B, _N, _H, its codec and
    whatever runs on its own kernels.  Points of different curves — different (p, a, b) — neither compare equal nor add; the
    variants of one curve do both."""
    __slots__ = ()

    def __init__(self, x, y):
        self.x, self.y = x, y
        if x is None and y is None:
            return
        if x is None or y is None or not (0 <= x < self._P and 0 <= y < self._P):
            raise ValueError("Invalid point coordinates")
        if not self._on_curve(x, y):
            raise ValueError("Point is not on the curve")

    @classmethod
    def _on_curve(cls, x: int, y: int) -> bool:
        return (y * y - (x * x * x + cls._SW_A * x + cls._SW_B)) % cls._P == 0

    @classmethod
    def _trusted(cls, x: int, y: int):
        """Kernel outputs: 64 zero bytes are the identity."""
        pt = object.__new__(cls)
        pt.x, pt.y = (None, None) if x == 0 and y == 0 else (x, y)
        return pt

    def _same_curve(self, other) -> bool:
        return type(other) is type(self) or (isinstance(other, _ShortWeierstrassPoint) and self._P == other._P
                                             and self._SW_A == other._SW_A and self._SW_B == other._SW_B)

    def __eq__(self, other):
        return self._same_curve(other) and self.x == other.x and self.y == other.y

    def __hash__(self):
        return 0 if self.x is None else (self.x + self.y) % self._N

    # -- group law (sw_affine_point.py)
    def __add__(self, other):
        if not self._same_curve(other):
            raise TypeError("Can only add SWAffinePoint instances")
        if self.is_identity():
            return other
        if other.is_identity():
            return self
        p = self._P
        if self.x == other.x:
            return self.double() if self.y == other.y else self.identity()
        lam = (other.y - self.y) * pow(other.x - self.x, -1, p) % p
        x3 = (lam * lam - self.x - other.x) % p
        return type(self)(x3, (lam * (self.x - x3) - self.y) % p)

    def double(self):
        if self.is_identity() or self.y == 0:
            return self.identity()
        p = self._P
        lam = (3 * self.x * self.x + self._SW_A) * pow(2 * self.y, -1, p) % p
        x3 = (lam * lam - 2 * self.x) % p
        return type(self)(x3, (lam * (self.x - x3) - self.y) % p)

    def __neg__(self):
        return self if self.is_identity() else type(self)(self.x, -self.y % self._P)

    def clear_cofactor(self):
        return scalar_mul_batch_raw([self], [self._H])[0]          # host doublings: none, and self, where the cofactor is 1

    # -- hash to curve: try-and-increment (point.py:252-296), candidates hashed natively, decoded and cofactor-cleared on the GPU; an
    # RFC 9380 suite puts its mixin in front
    @classmethod
    def encode_to_curve(cls, alpha_string: bytes, salt: bytes = b""):
        return cls.encode_to_curve_batch([alpha_string], [salt])[0]

    @classmethod
    def encode_to_curve_batch(cls, alpha_strings, salts=None):
        if not alpha_strings:
            return []
        return unpack_points(cls, runtime.context().encode_to_curve_batch(cls._suite_struct(), list(alpha_strings), salts))


class _Sec1Codec:
    """The SEC1 strings of a short Weierstrass point type (sw_affine_point.py point_to_string / string_to_point): 0x00 the identity,
    0x02 / 0x03 compressed, 0x04 uncompressed and, where the class sets _SEC1_HYBRID, 0x06 / 0x07 (both coordinates and the parity of
    y).  Coordinates are _SEC1_LEN big-endian bytes; _sec1_decompress turns a compressed (prefix, x < p) into a point."""
    __slots__ = ()
    _SEC1_LEN = 32
    _SEC1_HYBRID = False

    def point_to_string(self, compressed: bool = True) -> bytes:
        if self.is_identity():
            return b"\x00"
        x = self.x.to_bytes(self._SEC1_LEN, "big")
        if compressed:
            return (b"\x03" if self.y % 2 else b"\x02") + x
        return b"\x04" + x + self.y.to_bytes(self._SEC1_LEN, "big")

    @classmethod
    def _sec1_decompress(cls, prefix: int, x: int):
        """a host square root, the root of the prefix's parity"""
        p = cls._P
        try:
            y = cls.curve.mod_sqrt((x * x * x + cls._SW_A * x + cls._SW_B) % p)
        except ValueError:
            raise ValueError("Invalid point encoding") from None
        return cls(x, y if y % 2 == prefix % 2 else p - y)

    @classmethod
    def string_to_point(cls, data):
        if isinstance(data, str):
            data = bytes.fromhex(data)
        data = bytes(data)
        if len(data) == 0:
            raise ValueError("Empty octet string")
        prefix, p, n = data[0], cls._P, cls._SEC1_LEN
        if prefix == 0x00:
            if len(data) != 1:
                raise ValueError("Point at infinity must be single byte 0x00")
            return cls.identity()
        if prefix in (0x02, 0x03):
            if len(data) != n + 1:
                raise ValueError(f"Invalid compressed point length: expected {n + 1}, got {len(data)}")
            x = int.from_bytes(data[1:], "big")
            if x >= p:
                raise ValueError(f"x-coordinate {x} is not in field Fp (p={p})")
            return cls._sec1_decompress(prefix, x)
        if prefix == 0x04 or (cls._SEC1_HYBRID and prefix in (0x06, 0x07)):
            if len(data) != 2 * n + 1:
                kind = "uncompressed" if prefix == 0x04 else "hybrid"
                raise ValueError(f"Invalid {kind} point length: expected {2 * n + 1}, got {len(data)}")
            x, y = int.from_bytes(data[1 : n + 1], "big"), int.from_bytes(data[n + 1 :], "big")
            if x >= p:
                raise ValueError(f"x-coordinate {x} is not in field Fp (p={p})")
            if y >= p:
                raise ValueError(f"y-coordinate {y} is not in field Fp (p={p})")
            if prefix != 0x04 and y % 2 != prefix % 2:
                raise ValueError("Hybrid format: y parity doesn't match prefix")
            if not cls._on_curve(x, y):
                raise ValueError(f"Point ({x}, {y}) is not on curve")
            return cls(x, y)
        raise ValueError(f"Invalid point encoding prefix: 0x{prefix:02x}")


class BandersnatchSWPoint(_ShortWeierstrassPoint):
    """Affine short Weierstrass point of Bandersnatch_SW (dot_ring/curve/specs/bandersnatch_sw.py) over the module's field.  Scalar
    multiplications, MSMs, decoding and hash-to-curve run on the GPU under DR_CURVE_BANDERSNATCH_SW, whose kernels map to and from the
    twisted Edwards image."""
    _P = _P
    _N, _H, _CV = _N, 4, _native.CURVE_BANDERSNATCH_SW
    _SW_A = 10773120815616481058602537765553212789256758185246796157495669123169359657269
    _SW_B = 29569587568322301171008055308580903175558631321415017492731745847794083609535
    __slots__ = ()

    # -- codec (bandersnatch_sw.py: point_to_string / string_to_point): x little-endian, then a flag byte
    def point_to_string(self) -> bytes:
        if self.is_identity():
            return bytes(32) + b"\x40"
        return self.x.to_bytes(32, "little") + (b"\x00" if self.y <= -self.y % _P else b"\x80")

    @classmethod
    def string_to_point(cls, data):
        if isinstance(data, str):
            data = bytes.fromhex(data)
        if len(data) == 0:
            raise ValueError("Empty octet string")
        x = int.from_bytes(data[:-1], "little")
        try:
            y = cls.curve.mod_sqrt((x * x * x + cls._SW_A * x + cls._SW_B) % _P)
        except ValueError:
            y = 0
        if not y:
            raise ValueError("Invalid point: no y-coordinate found for x")
        small, large = sorted((y, -y % _P))
        flag = data[-1]
        if flag & 0x3F:
            raise ValueError("Invalid canonical point flags")
        if (flag >> 6) & 1:
            if (flag >> 7) & 1:
                raise ValueError("Invalid infinity point: negative flag is set")
            raise ValueError("Invalid infinity point: not supported")
        try:
            return cls(x, large if (flag >> 7) & 1 else small)
        except ValueError:
            raise ValueError("Invalid point") from None


class P256Point(_ShortWeierstrassPoint):
    """Affine point of P-256 (dot_ring/curve/specs/p256.py, P256_TAI): y^2 = x^3 - 3 x + b over its own field, cofactor 1.  Scalar
    multiplications, MSMs, decoding and hash-to-curve run on the GPU under DR_CURVE_P256 (kernels_p256.hip.h)."""
    _P = 0xFFFFFFFF00000001000000000000000000000000FFFFFFFFFFFFFFFFFFFFFFFF
    _N = 0xFFFFFFFF00000000FFFFFFFFFFFFFFFFBCE6FAADA7179E84F3B9CAC2FC632551
    _H, _CV = 1, _native.CURVE_P256
    _SW_A = -3
    _SW_B = 0x5AC635D8AA3A93E7B3EBBD55769886BC651D06B0CC53B0F63BCE3C3E27D2604B
    __slots__ = ()

    # -- codec (p256.py point_to_string / string_to_point / _string_to_canonical_point)
    def point_to_string(self) -> bytes:
        if self.is_identity():
            return bytes(32) + b"\x40"
        return self.x.to_bytes(32, "little") + (b"\x80" if self.y > -self.y % self._P else b"\x00")

    @classmethod
    def _y_pair(cls, x: int):
        """(smaller, larger) root of x^3 - 3 x + b, or None"""
        p = cls._P
        try:
            y = cls.curve.mod_sqrt((x * x * x + cls._SW_A * x + cls._SW_B) % p)
        except ValueError:
            return None
        return tuple(sorted((y, -y % p)))

    @classmethod
    def _string_to_canonical_point(cls, data: bytes):
        flag = data[-1]
        if flag & 0x3F:
            raise ValueError("Invalid canonical point flags")
        if (flag >> 6) & 1:
            if (flag >> 7) & 1 or any(data[:-1]):
                raise ValueError("Invalid infinity encoding")
            return cls.identity()
        x = int.from_bytes(data[:-1], "little")
        if x >= cls._P:
            raise ValueError("x-coordinate is not in field")
        ys = cls._y_pair(x)
        if ys is None:
            raise ValueError("Invalid point")
        return cls(x, ys[1] if (flag >> 7) & 1 else ys[0])

    @classmethod
    def _string_to_sec1_point(cls, data: bytes):
        """SWAffinePoint.string_to_point for a 0x02 / 0x03 prefix: x = the big-endian bytes after it, y of that parity"""
        x = int.from_bytes(data[1:], "big")
        if x >= cls._P:
            raise ValueError(f"x-coordinate {x} is not in field Fp (p={cls._P})")
        ys = cls._y_pair(x)
        if ys is None:
            raise ValueError("Invalid point encoding")
        y = ys[0] if ys[0] % 2 == data[0] % 2 else ys[1]
        return cls(x, y)

    @classmethod
    def string_to_point(cls, data):
        if isinstance(data, str):
            data = bytes.fromhex(data)
        data = bytes(data)
        if len(data) == 33 and data[0] in (0x02, 0x03):
            # canonical encodings put their flags in the last byte, so they can start with a SEC1 marker byte: the canonical
            # reading first, SEC1 compressed if that fails (the reference's fallback, which try-and-increment reaches too)
            try:
                return cls._string_to_canonical_point(data)
            except ValueError:
                return cls._string_to_sec1_point(data)
        if len(data) != 33:
            raise ValueError(f"Invalid compressed point length: expected 33, got {len(data)}")
        return cls._string_to_canonical_point(data)


class ShortWeierstrassA0Point(_ShortWeierstrassPoint):
    """y^2 = x^3 + b: secp256k1 and BLS12-381's E(Fq)"""
    _SW_A = 0
    __slots__ = ()


class Secp256k1Point(_Rfc9380, _Sec1Codec, ShortWeierstrassA0Point):
    """Affine point of secp256k1 (dot_ring/curve/specs/secp256k1.py): y^2 = x^3 + 7 over its own field, cofactor 1, SEC1 strings.
    Scalar multiplications (secp256k1.py:85-93: the scalar reduced mod n, a negative one through -P, 0 gives the identity), MSMs,
    decoding and hashing to the curve (RFC 9380: simplified SWU and the 3-isogeny) run on the GPU under the suite's curve id
    (kernels_secp256k1.hip.h)."""
    _P = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEFFFFFC2F
    _N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFEBAAEDCE6AF48A03BBFD25E8CD0364141
    _H, _CV = 1, _native.CURVE_SECP256K1
    _SW_B = 7
    __slots__ = ()

    # -- hash to curve (RFC 9380; sw_affine_point.py:428-562): expand_message_xmd natively on the host, the map on the GPU
    @classmethod
    def _mapped(cls, us: bytes, per_item: int):
        raw, ok = runtime.context().secp256k1_map_to_curve(us, per_item)
        if 0 in ok:
            raise ValueError("base is not invertible for the given modulus")      # pow(x_den, -1, p) of apply_isogeny
        return unpack_points(cls, raw)

    @classmethod
    def map_to_curve_simple_swu(cls, u: int):
        return cls._mapped((int(u) % cls._P).to_bytes(32, "little"), 1)[0]


class Bls12381G1Point(_WideRfc9380, _Sec1Codec, ShortWeierstrassA0Point):
    """Affine point of E(Fq): y^2 = x^3 + 4 over BLS12-381's 381-bit base field (dot_ring/curve/specs/bls12_381_G1.py), the identity is
    (None, None).  It has Secp256k1Point's surface (the host big-int additions are the shared a = 0 base class's) with 48-byte
    coordinates.  E(Fq) has order h r: a point need not lie in G1, so scalars are NEVER reduced mod r — `P * k` is exact for every
    integer k and every point.  Scalar multiplications, MSMs, decoding of compressed strings and hashing to the curve (RFC 9380:
    simplified SWU, the 11-isogeny, h_eff) run on the GPU (kernels_g1_h2c.hip.h, the dr_blsg1_* entry points)."""
    _P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    _N = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    _H = 0xD201000000010001                              # h_eff of RFC 9380 8.8.1: the reference's `cofactor`, what clear_cofactor multiplies by
    _COFACTOR = 0x396C8C005555E1568C00AAAB0000AAAB       # #E(Fq) = _COFACTOR * _N
    _CV = _native.CURVE_BLS12_381_G1
    _SW_B = 4
    _SEC1_LEN, _SEC1_HYBRID = 48, True
    _SUITE, _NO_IMAGE = "blsg1", "base is not invertible for the given modulus"     # pow(x_den, -1, p) of apply_isogeny
    __slots__ = ()

    # -- kernels: points cross as x || y, 48 + 48 bytes little-endian, 96 zero bytes the identity; scalars as they are
    @staticmethod
    def _pack(points) -> bytes:
        return b"".join((p.x or 0).to_bytes(48, "little") + (p.y or 0).to_bytes(48, "little") for p in points)

    @classmethod
    def _unpack(cls, raw: bytes):
        frm, mk = int.from_bytes, cls._trusted
        return [mk(frm(raw[i : i + 48], "little"), frm(raw[i + 48 : i + 96], "little")) for i in range(0, len(raw), 96)]

    @classmethod
    def _terms(cls, points, scalars):
        """(points, scalars below 2^256) with the same sum of products: a scalar outside [0, 2^256) is reduced mod #E(Fq) = h r (381
        bits, the exponent of every point) and, if still 2^256 or more, split as k_lo + 2^192 k_hi over P and 2^192 P"""
        pts, ks, wide = [], [], []
        for pt, k in zip(points, scalars):
            k = int(k)
            if not 0 <= k < 1 << 256:
                k %= cls._COFACTOR * cls._N
            if k < 1 << 256:
                pts.append(pt)
                ks.append(k)
            else:
                wide.append((pt, k))
        if wide:
            shifted = cls._unpack(runtime.context().blsg1_scalar_mul_batch(cls._pack([pt for pt, _ in wide]),
                                                                           (1 << 192).to_bytes(32, "little") * len(wide)))
            for (pt, k), hi in zip(wide, shifted):
                pts += [pt, hi]
                ks += [k & ((1 << 192) - 1), k >> 192]
        return pts, ks

    def __mul__(self, scalar: int):
        """exact for every integer: negative k negates, 0 <= k < 2^256 is one kernel entry, larger k goes mod h r through two terms"""
        k = int(scalar)
        if k < 0:
            return (-self) * (-k)
        pts, ks = self._terms([self], [k])
        if len(pts) == 1:
            raw = runtime.context().blsg1_scalar_mul_batch(self._pack(pts), ks[0].to_bytes(32, "little"))
        else:
            raw = runtime.context().blsg1_msm_groups(self._pack(pts), b"".join(v.to_bytes(32, "little") for v in ks), 2)
        return self._unpack(raw)[0]

    __rmul__ = __mul__

    @classmethod
    def msm(cls, points, scalars):
        """sum k_i P_i for any integers k_i: groups of up to 64 terms in one launch, then their partial sums the same way; from
        NARROW_PIP_FROM terms on the bucket method of dr_blsg1_msm (not a fixed schedule: for public scalars)"""
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        pts, ks = cls._terms(points, scalars)
        if not pts:
            return cls.identity()
        if len(pts) >= _native.NARROW_PIP_FROM:      # dr_blsg1_msm: the bucket method
            return cls._unpack(runtime.context().blsg1_msm(cls._pack(pts), b"".join(v.to_bytes(32, "little") for v in ks)))[0]
        while True:
            parts = -(-len(pts) // 64)
            m = len(pts) if parts == 1 else 64
            pad = parts * m - len(pts)                                     # padding: 0 * identity
            raw = runtime.context().blsg1_msm_groups(cls._pack(pts) + bytes(96 * pad),
                                                     b"".join(v.to_bytes(32, "little") for v in ks) + bytes(32 * pad), m)
            pts = cls._unpack(raw)
            if parts == 1:
                return pts[0]
            ks = [1] * parts

    def clear_cofactor(self):
        return self * self._H

    # -- codec: SEC1 with 48-byte coordinates and the hybrid forms; any point of E(Fq) decodes, in G1 or not (curve.valid_point asks that)
    @classmethod
    def _sec1_decompress(cls, prefix: int, x: int):
        """the decode kernel"""
        raw, ok = runtime.context().blsg1_decode_points(bytes([prefix]) + x.to_bytes(48, "big"), check=False)
        if not ok[0]:
            raise ValueError("Invalid point encoding")
        return cls._unpack(raw)[0]

    # -- hash to curve (RFC 9380 BLS12381G1_XMD:SHA-256_SSWU_RO_ / _NU_): expand_message_xmd natively on the host, the map on the GPU
    @classmethod
    def map_to_curve_simple_swu(cls, u: int):
        """one image on E, before the cofactor clearing (a point of E(Fq), in general outside G1)"""
        return cls._mapped((int(u) % cls._P).to_bytes(48, "little"), 1, clear=False)[0]

    # -- what the module-level batch helpers ask a wide point type
    @classmethod
    def _scalar_mul_batch(cls, points, scalars):
        pts, ks = cls._terms(points, scalars)
        if len(pts) != len(points):              # a scalar of 2^256 or more became two terms: point by point
            return [p * k for p, k in zip(points, scalars)]
        return cls._unpack(runtime.context().blsg1_scalar_mul_batch(cls._pack(pts), b"".join(k.to_bytes(32, "little") for k in ks)))

    @classmethod
    def _msm_groups(cls, points, scalars, m: int):
        return [cls.msm(points[i : i + m], scalars[i : i + m]) for i in range(0, len(points), m)]

    @classmethod
    def _valid_points(cls, points) -> list[bool]:
        """the reference's valid_point for a batch: on the curve, not the identity and r P = O — the CHECK mode of the decoder"""
        live = [i for i, pt in enumerate(points) if not pt.is_identity() and pt.is_on_curve()]
        out = [False] * len(points)
        if live:
            _, ok = runtime.context().blsg1_decode_points(b"".join(points[i].point_to_string() for i in live), check=True)
            for i, flag in zip(live, ok):
                out[i] = bool(flag)
        return out


class Fp2:
    """An element re + im i of Fp2 = Fp[i] / (i^2 + 1) with the surface of the reference's dot_ring/curve/fp2.py: re, im, p, the
    arithmetic operators (integers act as elements of Fp), inv, is_square, sqrt, sgn0, to_tuple.  Host big-integer code."""
    __slots__ = ("re", "im", "p")

    def __init__(self, re: int, im: int, p: int):
        self.p = int(p)
        self.re, self.im = int(re) % self.p, int(im) % self.p

    def _coerce(self, other):
        if isinstance(other, Fp2):
            if other.p != self.p:
                raise ValueError("Fp2 operands use different fields")
            return other
        if isinstance(other, int):
            return Fp2(other, 0, self.p)
        return None

    def __eq__(self, other):
        if isinstance(other, Fp2):
            return self.p == other.p and self.re == other.re and self.im == other.im
        if isinstance(other, int):
            return self.im == 0 and self.re == other % self.p
        return NotImplemented

    def __hash__(self):
        return hash((self.re, self.im, self.p))

    def __repr__(self):
        return f"Fp2({self.re}, {self.im})"

    def __add__(self, other):
        other = self._coerce(other)
        return NotImplemented if other is None else Fp2(self.re + other.re, self.im + other.im, self.p)

    __radd__ = __add__

    def __neg__(self):
        return Fp2(-self.re, -self.im, self.p)

    def __sub__(self, other):
        other = self._coerce(other)
        return NotImplemented if other is None else Fp2(self.re - other.re, self.im - other.im, self.p)

    def __rsub__(self, other):
        other = self._coerce(other)
        return NotImplemented if other is None else other - self

    def __mul__(self, other):
        other = self._coerce(other)
        if other is None:
            return NotImplemented
        return Fp2(self.re * other.re - self.im * other.im, self.re * other.im + self.im * other.re, self.p)

    __rmul__ = __mul__

    def __pow__(self, e: int):
        if e < 0:
            return self.inv() ** -e
        acc, base = Fp2(1, 0, self.p), self
        while e:
            if e & 1:
                acc = acc * base
            base = base * base
            e >>= 1
        return acc

    def conj(self):
        return Fp2(self.re, -self.im, self.p)

    def norm(self) -> int:
        return (self.re * self.re + self.im * self.im) % self.p

    def is_zero(self) -> bool:
        return self.re == 0 and self.im == 0

    def inv(self):
        n = self.norm()
        if n == 0:
            raise ZeroDivisionError("Fp2 zero has no inverse")
        ni = pow(n, -1, self.p)
        return Fp2(self.re * ni, -self.im * ni, self.p)

    def __truediv__(self, other):
        other = self._coerce(other)
        return NotImplemented if other is None else self * other.inv()

    def __rtruediv__(self, other):
        other = self._coerce(other)
        return NotImplemented if other is None else other * self.inv()

    def is_square(self) -> bool:
        """through the norm (p = 3 mod 4): a^((p^2 - 1) / 2) = norm(a)^((p - 1) / 2); zero is a square"""
        return pow(self.norm(), (self.p - 1) // 2, self.p) != self.p - 1

    def sqrt(self):
        """a root, or None: the norm route the device takes (csrc/fq2_28.hip.h) — roots in Fp of the norm and of (re +- s) / 2, one
        division; an element of Fp has the root (r, 0) or (0, r)"""
        p = self.p
        if p % 4 != 3:
            raise NotImplementedError("Fp2.sqrt needs p = 3 mod 4")
        root = lambda v: pow(v, (p + 1) // 4, p)  # noqa: E731
        if self.im == 0:
            r = root(self.re)                      # r^2 = +-re: (0, r)^2 = -r^2
            return Fp2(r, 0, p) if r * r % p == self.re else Fp2(0, r, p)
        s = root(self.norm())
        if s * s % p != self.norm():
            return None
        d = (self.re + s) * pow(2, -1, p) % p
        r = root(d)
        t = self.im * pow(2 * r, -1, p) % p
        return Fp2(r, t, p) if r * r % p == d else Fp2(t, r, p)

    def sgn0(self) -> int:
        return (self.re & 1) | ((self.re == 0) & (self.im & 1))

    def to_tuple(self):
        return self.re, self.im


class Bls12381G2Point(_WideRfc9380, _AffinePoint):
    """Affine point of E(Fq2): y^2 = x^3 + 4 (1 + i) over BLS12-381's quadratic extension (dot_ring/curve/specs/bls12_381_G2.py), the
    identity is (None, None); coordinates are Fp2 values ((re, im) tuples are accepted).  E(Fq2) has order h2 r (762 bits): a point need
    not lie in G2, so scalars are never reduced mod r.  Single additions are host big-integer code; scalar multiplications, sums of
    scalar multiples (msm, msm_groups: kernels_g2_msm.hip.h), the subgroup check and hashing to the curve (RFC 9380: simplified SWU, the
    3-isogeny, the clearing by psi) run on the GPU (kernels_g2_h2c.hip.h, the dr_blsg2_* entry points).  Scalars on this curve are
    public: none of it is a fixed schedule.  There is no point codec, as in the reference."""
    _P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    _N = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
    # h_eff of RFC 9380 8.8.2: the reference's `cofactor`, what clear_cofactor multiplies by (636 bits)
    _H = 0xBC69F08F2EE75B3584C6A0EA91B352888E2A8E9145AD7689986FF031508FFE1329C2F178731DB956D82BF015D1212B02EC0EC69D7477C1AE954CBC06689F6A359894C0ADEBBF6B4E8020005AAA95551
    # #E(Fq2) = _COFACTOR * _N
    _COFACTOR = 0x5D543A95414E7F1091D50792876A202CD91DE4547085ABAA68A205B2E5A7DDFA628F1CB4D9E82EF21537E293A6691AE1616EC6E786F0C70CF1C38E31C7238E5
    _CV = _native.CURVE_BLS12_381_G2
    __slots__ = ()

    def __init__(self, x, y):
        self.x, self.y = self._coord(x), self._coord(y)
        if self.x is None and self.y is None:
            return
        if self.x is None or self.y is None:
            raise ValueError("Invalid point coordinates")
        if not self._on_curve(self.x, self.y):
            raise ValueError("Point is not on the curve")

    @classmethod
    def _coord(cls, value):
        if value is None:
            return None
        if isinstance(value, Fp2):
            if value.p != cls._P:
                raise ValueError("Fp2 coordinate uses the wrong field")
            return value
        if isinstance(value, tuple) and len(value) == 2:
            return Fp2(value[0], value[1], cls._P)
        raise TypeError("BLS12-381 G2 coordinates must be Fp2 values")

    @classmethod
    def _on_curve(cls, x: Fp2, y: Fp2) -> bool:
        return y * y == x * x * x + Fp2(4, 4, cls._P)

    @classmethod
    def _trusted(cls, x: Fp2, y: Fp2):
        """Kernel outputs: 192 zero bytes are the identity."""
        pt = object.__new__(cls)
        pt.x, pt.y = (None, None) if x.is_zero() and y.is_zero() else (x, y)
        return pt

    def __eq__(self, other):
        return isinstance(other, Bls12381G2Point) and self.x == other.x and self.y == other.y

    def __hash__(self):
        return 0 if self.x is None else hash((self.x.to_tuple(), self.y.to_tuple()))

    # -- group law on the host
    def __add__(self, other):
        if not isinstance(other, Bls12381G2Point):
            raise TypeError("Can only add BLS12_381_G2Point instances")
        if self.is_identity():
            return other
        if other.is_identity():
            return self
        if self.x == other.x:
            if (self.y + other.y).is_zero():
                return self.identity()
            lam = 3 * self.x * self.x / (2 * self.y)
        else:
            lam = (other.y - self.y) / (other.x - self.x)
        x3 = lam * lam - self.x - other.x
        return self._trusted(x3, lam * (self.x - x3) - self.y)

    def __neg__(self):
        return self if self.is_identity() else self._trusted(self.x, -self.y)

    def __sub__(self, other):
        if not isinstance(other, Bls12381G2Point):
            raise TypeError("Can only subtract BLS12_381_G2Point instances")
        return self + (-other)

    # -- kernels: Fq2 elements cross as c0 || c1, points as x || y, 4 x 48 bytes little-endian, 192 zero bytes the identity
    @staticmethod
    def _pack_fp2(a: Fp2) -> bytes:
        return a.re.to_bytes(48, "little") + a.im.to_bytes(48, "little")

    @classmethod
    def _pack(cls, points) -> bytes:
        return b"".join(bytes(192) if p.is_identity() else cls._pack_fp2(p.x) + cls._pack_fp2(p.y) for p in points)

    @classmethod
    def _unpack(cls, raw: bytes):
        frm = lambda i: Fp2(int.from_bytes(raw[i : i + 48], "little"), int.from_bytes(raw[i + 48 : i + 96], "little"), cls._P)  # noqa: E731
        return [cls._trusted(frm(i), frm(i + 96)) for i in range(0, len(raw), 192)]

    def __mul__(self, scalar: int):
        """exact for every integer: negative k negates, 0 <= k < 2^768 is one kernel entry with k as it is, larger k goes mod h2 r"""
        k = int(scalar)
        if k < 0:
            return (-self) * (-k)
        if k >> 768:
            k %= self._COFACTOR * self._N
        return self._unpack(runtime.context().blsg2_scalar_mul_batch(self._pack([self]), k.to_bytes(96, "little")))[0]

    __rmul__ = __mul__

    @classmethod
    def _wide_scalar(cls, k) -> int:
        """a scalar as the 96-byte entry points take it: negative or 2^768 and more goes mod #E(Fq2) = h2 r, the exponent of every point"""
        k = int(k)
        return k if 0 <= k < 1 << 768 else k % (cls._COFACTOR * cls._N)

    @classmethod
    def _terms(cls, points, scalars):
        """(points, scalars below 2^256) with the same sum of products: a scalar outside [0, 2^256) is reduced mod #E(Fq2) = h2 r (762
        bits) and, if still 2^256 or more, split as k0 + 2^256 k1 + 2^512 k2 over P, 2^256 P and 2^512 P; the shifted points of all such
        terms come from one scalar_mul_batch"""
        pts, ks, wide = [], [], []
        for pt, k in zip(points, scalars):
            k = int(k)
            if not 0 <= k < 1 << 256:
                k %= cls._COFACTOR * cls._N
            if k < 1 << 256:
                pts.append(pt)
                ks.append(k)
            else:
                wide.append((pt, k))
        if wide:
            shifts = [s for _, k in wide for s in ((256, 512) if k >> 512 else (256,))]
            bases = [pt for pt, k in wide for _ in ((256, 512) if k >> 512 else (256,))]
            shifted = iter(cls._unpack(runtime.context().blsg2_scalar_mul_batch(cls._pack(bases),
                                                                                b"".join((1 << s).to_bytes(96, "little") for s in shifts))))
            mask = (1 << 256) - 1
            for pt, k in wide:
                pts += [pt, next(shifted)]
                ks += [k & mask, (k >> 256) & mask]
                if k >> 512:
                    pts.append(next(shifted))
                    ks.append(k >> 512)
        return pts, ks

    @classmethod
    def msm(cls, points, scalars):
        """sum k_i P_i for any integers k_i and any points of E(Fq2): dr_blsg2_msm on terms with scalars below 2^256 — msm_groups' kernel
        in chunks of 64 below BLSG2_PIP_FROM terms, the bucket method from there on.  For public scalars, as everything on this curve."""
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        pts, ks = cls._terms(points, scalars)
        if not pts:
            return cls.identity()
        return cls._unpack(runtime.context().blsg2_msm(cls._pack(pts), b"".join(k.to_bytes(32, "little") for k in ks)))[0]

    # -- the batch operations of this type, as classmethods of its own.  They are NOT hooked under the module-level helpers
    # (scalar_mul_batch, msm_groups, valid_points, curve.valid_point): what those do on a point of this type is part of the recorded
    # point surface (tests/golden/point_surface_*.json) and stays as it is.
    @classmethod
    def scalar_mul_batch(cls, points, scalars):
        """[k_i P_i] in one launch; negative scalars and scalars of 2^768 or more as __mul__ treats them"""
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        if not points:
            return []
        ks = b"".join(cls._wide_scalar(k).to_bytes(96, "little") for k in scalars)
        return cls._unpack(runtime.context().blsg2_scalar_mul_batch(cls._pack(points), ks))

    @classmethod
    def msm_groups(cls, points, scalars, m: int):
        """[sum_{j<m} k_{g m + j} P_{g m + j}] for consecutive groups of m terms: one launch of dr_blsg2_msm_groups for m <= 64 (96-byte
        scalars, reduced mod h2 r only where they are negative or 2^768 and more), one msm per group above that"""
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        if not points:
            return []
        if m > 64:
            return [cls.msm(points[i : i + m], scalars[i : i + m]) for i in range(0, len(points), m)]
        ks = b"".join(cls._wide_scalar(k).to_bytes(96, "little") for k in scalars)
        return cls._unpack(runtime.context().blsg2_msm_groups(cls._pack(points), ks, m))

    @classmethod
    def valid_points(cls, points) -> list[bool]:
        """the reference's valid_point for a batch: false for the identity and for what is off the curve, otherwise r P = O by the
        subgroup mode of check_points.  The reference asks h_eff P != O and (h_eff^-1 mod r) h_eff P = P.  #E(Fq2) = h2 r with r prime and
        not dividing h2, so a point of the curve is P = P_r + P_h in one way with r P_r = O and h2 P_h = O.  h_eff (_H) is a multiple of
        h2 (_COFACTOR) and prime to r: h_eff P = h_eff P_r, and c = h_eff^-1 mod r gives c h_eff P = P_r.  So the two conditions say
        P_r != O and P_r = P, which is P != O and r P = O."""
        live = [i for i, pt in enumerate(points) if not pt.is_identity() and pt.is_on_curve()]
        out = [False] * len(points)
        if live:
            ok = runtime.context().blsg2_check_points(cls._pack([points[i] for i in live]), subgroup=True)
            for i, flag in zip(live, ok):
                out[i] = bool(flag)
        return out

    def clear_cofactor(self):
        return self * self._H

    def point_to_string(self) -> bytes:
        raise NotImplementedError("BLS12-381 G2 point serialization is not implemented")

    @classmethod
    def string_to_point(cls, data):
        raise NotImplementedError("BLS12-381 G2 point deserialization is not implemented")

    # -- hash to curve (RFC 9380 BLS12381G2_XMD:SHA-256_SSWU_RO_ / _NU_): expand_message_xmd natively on the host, the map on the GPU
    # (no input reaches _NO_IMAGE: the isogeny's kernel has no point of E'(Fq2))
    _SUITE, _NO_IMAGE = "blsg2", "base is not invertible for the given modulus"

    @classmethod
    def map_to_curve_simple_swu(cls, u):
        """one image on E, before the cofactor clearing (a point of E(Fq2), in general outside G2)"""
        return cls._mapped(cls._pack_fp2(cls._coord(u)), 1, clear=False)[0]


class P256SswuPoint(_Rfc9380, _Sec1Codec, P256Point):
    """Affine point of P256_RO / P256_NU (dot_ring/curve/specs/p256.py with E2C_Variant.SSWU / SSWU_NU): P-256's group and kernels under
    the variant's curve id, the reference's generic SEC1 codec in place of P256_TAI's (P256Point.point_to_string defers to
    SWAffinePoint's for these variants), and hashing to the curve by RFC 9380's simplified SWU map (k_p256_map_to_curve)."""
    __slots__ = ()

    # -- hash to curve (RFC 9380; sw_affine_point.py:428-533): expand_message_xmd natively on the host, the map on the GPU
    @classmethod
    def _mapped(cls, us: bytes, per_item: int):
        raw, _ = runtime.context().p256_map_to_curve(us, per_item)          # (no denominator of this map can vanish)
        return unpack_points(cls, raw)

    @classmethod
    def map_to_curve_simple_swu(cls, u: int):
        return cls._mapped((int(u) % cls._P).to_bytes(32, "little"), 1)[0]


def _ell2_curve25519(u: int):
    """RFC 9380's Elligator 2 onto curve25519, v^2 = u^3 + 486662 u^2 + u (te_curve.py:48-95, mg_affine_point.py:289-346): the
    Montgomery coordinates of ONE image, host big-int code"""
    p, a = 2**255 - 19, 486662
    tv1 = 2 * u * u % p
    if tv1 == p - 1:
        tv1 = 0
    x1 = -a * pow(tv1 + 1, -1, p) % p
    gx1 = ((x1 + a) * x1 + 1) * x1 % p
    e2 = gx1 == 0 or pow(gx1, (p - 1) // 2, p) == 1
    x, y2 = (x1, gx1) if e2 else ((-x1 - a) % p, tv1 * gx1 % p)
    y = _sqrt_5mod8(y2, p)
    if e2 ^ (y % 2 == 1):                     # (the parity picks the root: whichever the square-root routine returned)
        y = -y % p
    return x, y


class Ed25519Ell2Point(_Rfc9380, BandersnatchPoint):
    """Affine point of Ed25519_RO / Ed25519_NU (dot_ring/curve/specs/ed25519.py with E2C_Variant.ELL2 / ELL2_NU): Ed25519's group, kernels
    and codec under the variant's curve id, hashing to the curve by RFC 9380's Elligator 2 (k_ed25519_map_to_curve: the map onto
    curve25519, the reference's mont_to_ed25519, the sum of two images for RO, the cofactor cleared)."""
    __slots__ = ()

    @classmethod
    def _mapped(cls, us: bytes, per_item: int):
        raw, ok = runtime.context().ed25519_map_to_curve(us, per_item)
        if 0 in ok:
            raise ValueError("base is not invertible for the given modulus")      # pow(v, -1, p) / pow(u + 1, -1, p) of mont_to_ed25519
        return unpack_points(cls, raw)

    @classmethod
    def map_to_curve(cls, u: int):
        """Ed25519Point.map_to_curve (te_curve.py:48-95, then mont_to_ed25519): ONE image with its cofactor not cleared, host big-int code
        as BandersnatchPoint.map_to_curve is; the batched path (encode_to_curve_from_field) runs the same steps in the kernel"""
        p = cls._P
        x, y = _ell2_curve25519(u)
        # pow raises ValueError where y = 0 or x = -1, as the reference does
        return cls(_sqrt_tonelli_shanks(-486664, p) * x % p * pow(y, -1, p) % p, (x - 1) * pow(x + 1, -1, p) % p)


class Ed448Point(_WideRfc9380, BandersnatchPoint):
    """Affine point of Ed448_RO / Ed448_NU (dot_ring/curve/specs/ed448.py): x^2 + y^2 = 1 - 39081 x^2 y^2 over p = 2^448 - 2^224 - 1,
    cofactor 4, the identity (0, 1).  Coordinates and scalars are 56 bytes, so nothing here goes through the 64-byte entry points: scalar
    multiplications, MSMs, the subgroup check and hashing to the curve run on the dr_ed448_* kernels (kernels_ed448.hip.h), whose scalars
    are used as they are — the reduction mod n of the reference's __mul__ happens here.  Single additions are host big-int code
    (BandersnatchPoint's affine formulas with this curve's a and d)."""
    _P = 2**448 - 2**224 - 1
    _N = 2**446 - 0x8335DC163BB124B65129C96FDE933D8D723A70AADC873D6D54A7BB0D
    _A, _D, _H, _CV = 1, -39081, 4, _native.CURVE_ED448_RO
    _MG_A = 156326
    _WIDE = True                  # the VRF classes keep their Python orchestration: the native batch provers carry 32-byte scalars
    _SUITE, _NO_IMAGE = "ed448", "Point is not on the curve"      # mont_to_ed448 with inv(0) = 0 gives (0, 0): u in {0, 1, p - 1}
    __slots__ = ()

    # -- the C ABI's forms
    @staticmethod
    def _pack(points) -> bytes:
        return b"".join(p.x.to_bytes(56, "little") + p.y.to_bytes(56, "little") for p in points)

    @classmethod
    def _unpack(cls, raw: bytes):
        """Kernel outputs are group elements by construction: no per-point curve check."""
        frm, mk = int.from_bytes, cls._trusted
        return [mk(frm(raw[i : i + 56], "little"), frm(raw[i + 56 : i + 112], "little")) for i in range(0, len(raw), 112)]

    @classmethod
    def _scalars(cls, scalars) -> bytes:
        return b"".join((int(k) % cls._N).to_bytes(56, "little") for k in scalars)

    # -- MSM on the GPU (te_affine_point.py:163: the scalars reduced mod n)
    @classmethod
    def msm(cls, points, scalars):
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        if len(points) >= _native.WIDE_PIP_FROM:      # dr_wide_msm: the bucket method
            return cls._unpack(runtime.context().wide_msm("ed448", cls._pack(points), cls._scalars(scalars)))[0]
        # below it the dispatch that tests/golden/point_surface_cpu.json records for this class stays as it was
        acc = cls.identity()
        for lo in range(0, len(points), 64):          # groups of up to 64 terms on the device, their sums added on the host
            part = points[lo : lo + 64]
            acc = acc + msm_groups(part, scalars[lo : lo + 64], len(part))[0]
        return acc

    def clear_cofactor(self):
        return scalar_mul_batch_raw([self], [self._H])[0]

    # -- codec (point.py: uncompressed_p2s / uncompressed_s2p): x || y, 56 little-endian bytes each
    def point_to_string(self) -> bytes:
        return self.x.to_bytes(56, "little") + self.y.to_bytes(56, "little")

    @classmethod
    def string_to_point(cls, octet_string):
        if isinstance(octet_string, str):
            octet_string = bytes.fromhex(octet_string)
        octet_string = bytes(octet_string)
        return cls(int.from_bytes(octet_string[:56], "little"), int.from_bytes(octet_string[56:], "little"))

    # -- hash to curve (RFC 9380 edwards448_XOF:SHAKE256_ELL2_RO_ / _NU_): expand_message_xof natively on the host, the map on the GPU
    @classmethod
    def map_to_curve(cls, u: int):
        """Ed448Point.map_to_curve (te_curve.py map_to_curve_ell2, then mont_to_ed448): ONE image with its cofactor not cleared"""
        return cls._mapped((int(u) % cls._P).to_bytes(56, "little"), 1, clear=False)[0]

    # -- what the module-level batch helpers ask a wide point type
    @classmethod
    def _scalar_mul_batch(cls, points, scalars):
        return cls._unpack(runtime.context().ed448_scalar_mul_batch(cls._pack(points), cls._scalars(scalars)))

    @classmethod
    def _msm_groups(cls, points, scalars, m: int):
        if m > 64:                               # the kernel folds up to 64 terms in a wave: longer groups are one msm each (dr_wide_msm)
            return [cls.msm(points[i : i + m], scalars[i : i + m]) for i in range(0, len(points), m)]
        return cls._unpack(runtime.context().ed448_msm_groups(cls._pack(points), cls._scalars(scalars), m))

    @classmethod
    def _valid_points(cls, points) -> list[bool]:
        """curve.py:56 for a batch: on the curve, not the identity and n P = O (dr_ed448_decode_points with check = 1)"""
        _, ok = runtime.context().ed448_decode_points(cls._pack(points), True)
        return [bool(f) for f in ok]


class _MontgomeryPoint(_AffinePoint):
    """Affine point of a Montgomery curve y^2 = x^3 + A x^2 + x (montgomery/mg_affine_point.py with B = 1; x, y are the reference's names
    for u, v): the constructor's checks, the affine chord-and-tangent law and the uncompressed codec u || v, by the field's byte width.
    The identity is (None, None) and has no encoding; (0, 0) is a point (order 2), so inside the library the identity travels as bytes of
    0xff.  A concrete class gives _P, _N, _H, _CV, _MG_A, _FE_BYTES and its hashing."""
    __slots__ = ()

    def __init__(self, x, y):
        self.x, self.y = x, y
        if x is None and y is None:
            return
        if x is None or y is None or not (0 <= x < self._P and 0 <= y < self._P):
            raise ValueError("Invalid point coordinates")
        if not self._on_curve(x, y):
            raise ValueError("Point is not on the curve")

    @classmethod
    def _on_curve(cls, x: int, y: int) -> bool:
        return (y * y - ((x + cls._MG_A) * x + 1) * x) % cls._P == 0

    @classmethod
    def _trusted(cls, x: int, y: int):
        """Kernel outputs: coordinates of 0xff bytes are the identity."""
        ones = (1 << (8 * cls._FE_BYTES)) - 1
        pt = object.__new__(cls)
        pt.x, pt.y = (None, None) if x == y == ones else (x, y)
        return pt

    def __eq__(self, other):
        return isinstance(other, _MontgomeryPoint) and self._P == other._P and self.x == other.x and self.y == other.y

    def __hash__(self):
        return 0 if self.x is None else (self.x + self.y) % self._N

    def is_identity(self) -> bool:
        return self.x is None or self.y is None

    # -- group law (mg_affine_point.py:38-116, B = 1)
    def __add__(self, other):
        if not isinstance(other, _MontgomeryPoint) or self._P != other._P:
            return NotImplemented
        if self.is_identity():
            return other
        if other.is_identity():
            return self
        p, a = self._P, self._MG_A
        x1, y1, x2, y2 = self.x, self.y, other.x, other.y
        if x1 == x2:
            if y1 != y2 or y1 == 0:
                return self.identity()
            lam = (3 * x1 * x1 + 2 * a * x1 + 1) * pow(2 * y1, -1, p) % p
        else:
            lam = (y2 - y1) * pow(x2 - x1, -1, p) % p
        x3 = (lam * lam - a - x1 - x2) % p
        return type(self)(x3, (lam * (x1 - x3) - y1) % p)

    def double(self):
        return self + self

    def __neg__(self):
        return self if self.is_identity() else type(self)(self.x, -self.y % self._P)

    def clear_cofactor(self):
        return scalar_mul_batch_raw([self], [self._H])[0]

    # -- codec (mg_affine_point.py:348-389): u || v, little-endian; no compressed form, no encoding of the identity
    def point_to_string(self) -> bytes:
        if self.is_identity():
            raise ValueError("Cannot serialize point at infinity")
        if not self.curve.params.encoding.uncompressed:
            raise NotImplementedError("Compressed encoding not implemented")
        return self.x.to_bytes(self._FE_BYTES, "little") + self.y.to_bytes(self._FE_BYTES, "little")

    @classmethod
    def string_to_point(cls, data):
        if isinstance(data, str):
            data = bytes.fromhex(data)
        data = bytes(data)
        if not cls.curve.params.encoding.uncompressed:
            raise NotImplementedError("Compressed encoding not implemented")
        w = cls._FE_BYTES
        if len(data) != 2 * w:
            raise ValueError(f"Invalid point length: expected {2 * w}, got {len(data)}")
        return cls(int.from_bytes(data[:w], "little"), int.from_bytes(data[w:], "little"))


class Curve25519Point(_Rfc9380, _MontgomeryPoint):
    """Affine point of Curve25519_RO / Curve25519_NU (dot_ring/curve/specs/curve25519.py, montgomery/mg_affine_point.py):
    y^2 = x^3 + 486662 x^2 + x over 2^255 - 19 (x, y are the reference's names for u, v), cofactor 8, the identity is (None, None).
    (0, 0) is a point of the curve (order 2), so the identity cannot travel as 64 zero bytes: it packs as 64 bytes of 0xff for the generic
    entry points and as a flag byte for the dr_curve25519_* ones (pack_points_flagged).  Single additions are host big-int code with the
    reference's affine formulas; scalar multiplications, MSMs, decoding and hashing to the curve run on the GPU (kernels_curve25519.hip.h,
    which computes on the Ed25519 group law through the birational map)."""
    _P = 2**255 - 19
    _N = 2**252 + 0x14DEF9DEA2F79CD65812631A5CF5D3ED
    _H, _CV = 8, _native.CURVE_CURVE25519_RO
    _MG_A, _FE_BYTES = 486662, 32
    _IDENTITY_BYTES = b"\xff" * 64
    __slots__ = ()

    # -- hash to curve (RFC 9380 curve25519_XMD:SHA-512_ELL2_RO_ / _NU_): expand_message_xmd natively on the host, the map on the GPU
    @classmethod
    def map_to_curve(cls, u: int):
        """MGAffinePoint.map_to_curve (mg_affine_point.py:289-346): ONE image with its cofactor not cleared, host big-int code as the
        other suites' map_to_curve is; the batched path (encode_to_curve_from_field) runs the same steps in the kernel"""
        return cls(*_ell2_curve25519(u))

    @classmethod
    def _mapped(cls, us: bytes, per_item: int):
        return unpack_points_flagged(cls, *runtime.context().curve25519_map_to_curve(us, per_item))


class Curve448Point(_WideRfc9380, _MontgomeryPoint):
    """Affine point of Curve448_RO / Curve448_NU (dot_ring/curve/specs/curve448.py): y^2 = x^3 + 156326 x^2 + x over
    p = 2^448 - 2^224 - 1, cofactor 4.  Coordinates and scalars are 56 bytes, so nothing goes through the 64-byte entry points: scalar
    multiplications, MSMs, the subgroup check and hashing to the curve run on the dr_curve448_* kernels (kernels_curve448.hip.h, on the
    complete Edwards law birational to this curve), where the identity is 112 bytes of 0xff in and out.  The kernels use scalars as
    they are; MGAffinePoint.__mul__ does not reduce its scalar (P * k is exact for every integer, a negative k negating the point), so
    scalars go out reduced mod 4 n, the order of the whole group."""
    _P = 2**448 - 2**224 - 1
    _N = 2**446 - 0x8335DC163BB124B65129C96FDE933D8D723A70AADC873D6D54A7BB0D
    _H, _CV = 4, _native.CURVE_CURVE448_RO
    _MG_A, _FE_BYTES = 156326, 56
    _WIDE = True                  # the VRF classes keep their Python orchestration: the native batch provers carry 32-byte scalars
    _SUITE, _NO_IMAGE = "curve448", "No inverse exists"           # mod_inverse(0) of map_to_curve: u in {1, p - 1}
    _IDENTITY_BYTES = b"\xff" * 112
    __slots__ = ()

    # -- the C ABI's forms
    @classmethod
    def _pack(cls, points) -> bytes:
        return b"".join(cls._IDENTITY_BYTES if p.is_identity() else p.x.to_bytes(56, "little") + p.y.to_bytes(56, "little") for p in points)

    @classmethod
    def _unpack(cls, raw: bytes):
        """Kernel outputs are group elements by construction: no per-point curve check."""
        frm, mk = int.from_bytes, cls._trusted
        return [mk(frm(raw[i : i + 56], "little"), frm(raw[i + 56 : i + 112], "little")) for i in range(0, len(raw), 112)]

    @classmethod
    def _scalars(cls, scalars) -> bytes:
        return b"".join((int(k) % (cls._H * cls._N)).to_bytes(56, "little") for k in scalars)

    @classmethod
    def msm(cls, points, scalars):
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        if not points:
            return cls.identity()
        if len(points) <= 64:                         # one launch: a wave folds up to 64 terms
            return msm_groups(points, scalars, len(points))[0]
        # more: dr_wide_msm — chunks of 64 folded natively below 256 terms, the bucket method from there on
        return cls._unpack(runtime.context().wide_msm("curve448", cls._pack(points), cls._scalars(scalars)))[0]

    # -- hash to curve (RFC 9380 curve448_XOF:SHAKE256_ELL2_RO_ / _NU_): expand_message_xof natively on the host, the map on the GPU
    @classmethod
    def map_to_curve(cls, u: int):
        """MGAffinePoint.map_to_curve: ONE image with its cofactor not cleared; ValueError("No inverse exists") for u in {1, p - 1}"""
        return cls._mapped((int(u) % cls._P).to_bytes(56, "little"), 1, clear=False)[0]

    # -- what the module-level batch helpers ask a wide point type
    @classmethod
    def _scalar_mul_batch(cls, points, scalars):
        return cls._unpack(runtime.context().curve448_scalar_mul_batch(cls._pack(points), cls._scalars(scalars)))

    @classmethod
    def _msm_groups(cls, points, scalars, m: int):
        if m > 64:                               # the kernel folds up to 64 terms in a wave: longer groups are one msm each (dr_wide_msm)
            return [cls.msm(points[i : i + m], scalars[i : i + m]) for i in range(0, len(points), m)]
        return cls._unpack(runtime.context().curve448_msm_groups(cls._pack(points), cls._scalars(scalars), m))

    @classmethod
    def _valid_points(cls, points) -> list[bool]:
        """curve.py:56 for a batch: on the curve, not the identity and n P = O (dr_curve448_decode_points with check = 1)"""
        _, ok = runtime.context().curve448_decode_points(cls._pack(points), True)
        return [bool(f) for f in ok]


# ------------------------------------------------------------------ batched helpers over the C ABI
class _WidePrimeSwPoint(_WideRfc9380, _Sec1Codec, _ShortWeierstrassPoint):
    """What P-521 and P-384 share: a short Weierstrass curve of prime order (cofactor 1) over p = 3 mod 4 whose coordinates and scalars do
    not fit the 64-byte entry points, so scalar multiplications, MSMs, decoding and hashing to the curve run on the dr_<_SUITE>_* kernels.
    Coordinates and scalars are _ABI_LEN bytes little-endian at the C ABI, 2 _ABI_LEN zero bytes the identity; the kernels use scalars as
    they are — the reduction mod n happens here and is exact for every point, the group having prime order n.  Single additions are the
    shared host big-int law; SEC1 strings carry _SEC1_LEN-byte coordinates.  A concrete class gives _P, _N, _SW_B, _CV, _SEC1_LEN,
    _ABI_LEN and _SUITE."""
    _H, _SW_A = 1, -3
    _WIDE = True                  # the VRF classes keep their Python orchestration: the native batch provers carry 32-byte scalars
    _NO_IMAGE = "the map to the curve has no value"       # (never raised: every field element has an image)
    __slots__ = ()

    # -- the C ABI's forms: x || y little-endian, zero bytes the identity
    @classmethod
    def _pack(cls, points) -> bytes:
        n = cls._ABI_LEN
        return b"".join((p.x or 0).to_bytes(n, "little") + (p.y or 0).to_bytes(n, "little") for p in points)

    @classmethod
    def _unpack(cls, raw: bytes):
        """Kernel outputs are group elements by construction: no per-point curve check."""
        frm, mk, n = int.from_bytes, cls._trusted, cls._ABI_LEN
        return [mk(frm(raw[i : i + n], "little"), frm(raw[i + n : i + 2 * n], "little")) for i in range(0, len(raw), 2 * n)]

    @classmethod
    def _scalars(cls, scalars) -> bytes:
        return b"".join((int(k) % cls._N).to_bytes(cls._ABI_LEN, "little") for k in scalars)

    def __mul__(self, scalar: int):
        return self._scalar_mul_batch([self], [scalar])[0]

    __rmul__ = __mul__

    @classmethod
    def msm(cls, points, scalars):
        if len(points) != len(scalars):
            raise ValueError("Points and scalars must have same length")
        if not points:
            return cls.identity()
        if len(points) <= 64:                         # one launch: a wave folds up to 64 terms
            return msm_groups(points, scalars, len(points))[0]
        # more: dr_wide_msm — chunks of 64 folded natively below 256 terms, the bucket method from there on
        return cls._unpack(runtime.context().wide_msm(cls._SUITE, cls._pack(points), cls._scalars(scalars)))[0]

    def clear_cofactor(self):
        return self                                   # the cofactor is 1

    # -- codec: a compressed string's root is p = 3 mod 4's, on the host
    @classmethod
    def _sec1_decompress(cls, prefix: int, x: int):
        p = cls._P
        v = (x * x * x + cls._SW_A * x + cls._SW_B) % p
        y = pow(v, (p + 1) // 4, p)
        if y * y % p != v:
            raise ValueError("Invalid point encoding")
        return cls(x, y if y % 2 == prefix % 2 else p - y)

    # -- hash to curve (RFC 9380 ..._XMD:SHA-..._SSWU_RO_ / _NU_): expand_message_xmd natively on the host, the map on the GPU
    @classmethod
    def map_to_curve_simple_swu(cls, u: int):
        return cls._mapped((int(u) % cls._P).to_bytes(cls._ABI_LEN, "little"), 1, clear=False)[0]

    # -- what the module-level batch helpers ask a wide point type
    @classmethod
    def _scalar_mul_batch(cls, points, scalars):
        return cls._unpack(runtime.context()._wide_scalar_mul_batch(cls._SUITE, cls._pack(points), cls._scalars(scalars)))

    @classmethod
    def _msm_groups(cls, points, scalars, m: int):
        if m > 64:                               # the kernel folds up to 64 terms in a wave: longer groups are one msm each (dr_wide_msm)
            return [cls.msm(points[i : i + m], scalars[i : i + m]) for i in range(0, len(points), m)]
        return cls._unpack(runtime.context()._wide_msm_groups(cls._SUITE, cls._pack(points), cls._scalars(scalars), m))

    @classmethod
    def _valid_points(cls, points) -> list[bool]:
        """curve.py:56 for a batch: on the curve and not the identity (prime order: nothing else to ask)"""
        return [not pt.is_identity() and pt.is_on_curve() for pt in points]


class P521Point(_WidePrimeSwPoint):
    """Affine point of P521_RO / P521_NU (dot_ring/curve/specs/p521.py): y^2 = x^3 - 3 x + b over p = 2^521 - 1, the identity (None, None).
    Coordinates and scalars are 66 bytes (68 at the C ABI, scalars below 2^521); the kernels are kernels_p521.hip.h's."""
    _P = 2**521 - 1
    _N = 0x01FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFA51868783BF2F966B7FCC0148F709A5D03BB5C9B8899C47AEBB6FB71E91386409
    _CV = _native.CURVE_P521_RO
    _SW_B = 0x0051953EB9618E1C9A1F929A21A0B68540EEA2DA725B99B315F3B8B489918EF109E156193951EC7E937B1652C0BD3BB1BF073573DF883D2C34F1EF451FD46B503F00
    _SEC1_LEN, _ABI_LEN, _SUITE = 66, 68, "p521"
    __slots__ = ()


class P384Point(_WidePrimeSwPoint):
    """Affine point of P384_RO / P384_NU (dot_ring/curve/specs/p384.py): y^2 = x^3 - 3 x + b over p = 2^384 - 2^128 - 2^96 + 2^32 - 1, the
    identity (None, None).  Coordinates and scalars are 48 bytes, at the C ABI too; the kernels are kernels_p384.hip.h's, whose 97 windows
    take every 384-bit value."""
    _P = 2**384 - 2**128 - 2**96 + 2**32 - 1
    _N = 0xFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFC7634D81F4372DDF581A0DB248B0A77AECEC196ACCC52973
    _CV = _native.CURVE_P384_RO
    _SW_B = 0xB3312FA7E23EE7E4988E056BE3F82D19181D9C6EFE8141120314088F5013875AC656398D8A2ED19D2A85C8EDD3EC2AEF
    _SEC1_LEN, _ABI_LEN, _SUITE = 48, 48, "p384"
    __slots__ = ()


def pack_points(points) -> bytes:
    """x || y little-endian per point; an SW identity ((None, None)) packs as 64 zero bytes, as the ABI takes it, Curve25519's — where
    (0, 0) is a point — as 64 bytes of 0xff."""
    return b"".join(p._IDENTITY_BYTES if p.x is None
                    else (p.x or 0).to_bytes(32, "little") + (p.y or 0).to_bytes(32, "little") for p in points)


def pack_points_flagged(points):
    """(u || v bytes, identity flag bytes) of Curve25519 points as the dr_curve25519_* entry points take them: the identity is 64 zero
    bytes with its flag byte 1."""
    return (b"".join((p.x or 0).to_bytes(32, "little") + (p.y or 0).to_bytes(32, "little") for p in points),
            bytes(1 if p.is_identity() else 0 for p in points))


def unpack_points_flagged(cls, raw: bytes, flags: bytes):
    """Curve25519 kernel outputs with their identity flags: group elements by construction, no per-point curve check."""
    frm = int.from_bytes
    return [cls.identity() if flags[i] else cls._trusted(frm(raw[64 * i : 64 * i + 32], "little"), frm(raw[64 * i + 32 : 64 * i + 64], "little"))
            for i in range(len(flags))]


def pack_scalars(scalars, order: int = _N) -> bytes:
    return b"".join((int(s) % order).to_bytes(32, "little") for s in scalars)


def unpack_points(cls, raw: bytes):
    """Kernel outputs are group elements by construction: no per-point curve check."""
    frm, mk = int.from_bytes, cls._trusted
    return [mk(frm(raw[i : i + 32], "little"), frm(raw[i + 32 : i + 64], "little")) for i in range(0, len(raw), 64)]


def scalar_mul_batch(points, scalars):
    """[k_i * P_i] in one kernel launch."""
    if len(points) != len(scalars):
        raise ValueError("Points and scalars must have same length")
    return type(points[0])._scalar_mul_batch(points, scalars) if points else []


def _fixed_bases(cls):
    """the suite's constant points that get a fixed-base table: generator and Pedersen blinding base"""
    params = cls.curve.params
    bb = params.auxiliary_points.blinding_base
    return (tuple(params.generator),) + ((tuple(bb),) if bb else ())


def msm_groups(points, scalars, m: int):
    """[sum_{j<m} k_{g*m+j} * P_{g*m+j}] for consecutive groups of m terms, one launch."""
    return type(points[0])._msm_groups(points, scalars, m) if points else []


def valid_points(points) -> list[bool]:
    """curve.py:56 for a whole batch: non-identity members of the prime-order subgroup, one launch for all points (on G1, where E(Fq)
    is not h x (prime) for a small h, the decoder's subgroup check is the only sound one)."""
    return type(points[0])._valid_points(points) if points else []


def scalar_mul_batch_raw(points, small_scalars):
    """Scalar multiplication WITHOUT reduction mod n for points that may lie outside the prime-order subgroup:
    the kernel reduces scalars mod n, which is only sound on the subgroup, so small cofactor multiples are done
    with host doublings (4P = two doublings, 8P = three, as te_affine_point.py:235 clear_cofactor)."""
    out = []
    for p, k in zip(points, small_scalars):
        if k != type(p)._H:
            raise ValueError("only the cofactor multiple is supported here")
        for _ in range(k.bit_length() - 1):
            p = p.double()
        out.append(p)
    return out


# ------------------------------------------------------------------ suites / curve variants
def _variant(base, name: str, params: SuiteParams, **class_attrs):
    """the variant `name`: a curve object over params and the point type f"{name}Point" below base, bound to it"""
    curve = BandersnatchCurve(params)
    return CurveVariant(name, curve, type(f"{name}Point", (base,), {"__slots__": (), "curve": curve, "_CV": params.curve_id, **class_attrs}))


def _te_variant(base, name: str, params: SuiteParams):
    """... of a 256-bit twisted Edwards suite: the class takes its coefficients, order, cofactor and field from params"""
    return _variant(base, name, params, _A=params.a, _D=params.d, _N=params.subgroup_order, _H=params.cofactor, _P=params.field_modulus)


def _suite(name: str, suite_id: bytes, xof: bool, bb, ab, pp, **curve_consts):
    return _te_variant(BandersnatchPoint, name, SuiteParams(
        suite_id=suite_id, hash_fn=hashlib.shake_128 if xof else hashlib.sha512, auxiliary_points=AuxiliaryPoints(bb, ab, pp), xof=xof,
        **curve_consts))


def _nu(params: SuiteParams, curve_id: int) -> SuiteParams:
    """the suite's non-uniform (one field element) variant: it travels in the curve id"""
    return dataclasses.replace(params, curve_id=curve_id, e2c=params.e2c + "_nu")


class CurveVariant:
    """curve.py:353 — name, curve, point_type + key derivation."""

    def __init__(self, name, curve, point_type):
        self.name, self.curve, self.point_type = name, curve, point_type

    def point(self, x, y=None):
        if isinstance(x, _AffinePoint):
            return x
        if y is None:
            x, y = x
        return self.point_type(x, y)

    def public_key_from_secret(self, secret_key: bytes) -> bytes:
        if not isinstance(secret_key, (bytes, bytearray)):
            raise TypeError("secret_key must be bytes")
        return (self.point_type.generator_point() * int.from_bytes(secret_key, "little")).point_to_string()

    def secret_from_seed(self, seed: bytes):
        if not isinstance(seed, (bytes, bytearray)):
            raise TypeError("seed must be bytes")
        from .vrf.codec import enc_scalar
        from .vrf.primitives import secret_from_seed_scalar

        secret_key = enc_scalar(self, secret_from_seed_scalar(self, bytes(seed)))
        return self.public_key_from_secret(secret_key), secret_key


Bandersnatch = _suite(
    "Bandersnatch", b"Bandersnatch-SHA512-ELL2-v1", False,
    (23335687741101763108036518445642207119627658113885888016488710494487028845889,
     5552214580375038693022409684979828600325210968745774080859660443337357929963),
    (14056632001415368875257708737821299882600475929746323097150942355715730684350,
     10322661992765989500407719465917595459409463902187386706652408883505670839210),
    (26913883415342152801331916189968962157924271221160514298872262294143390094043,
     30874728313203001508631936119690348239461579770372782660098261717479009115354),
)
Bandersnatch_SHAKE128 = _suite(
    "Bandersnatch_SHAKE128", b"Bandersnatch-SHAKE128-ELL2-v1", True,
    (6153734995852631824944342602386415873379775188383988340041079006556670120775,
     27204351599954061630605768787803524395123895650061061132592995395630473050754),
    (27631238720955528589004064829276283990465032040945349648037876197995278250917,
     37605358688136619817560700742505556266961225274493904038881144193539047100140),
    (1834402953989431481748983728202937234471322740714585873803966488035889514523,
     52100941849053769665273763352270294131006971127418863694682093199651869272752),
)
# dot_ring/curve/specs/jubjub.py:17-66 — the other twisted Edwards curve over the BLS12-381 scalar field
JubJub = _suite(
    "JubJub", b"JubJub-SHA512-TAI-v1", False,
    (38206460563694846719174258613922853630278999941532690543235578292520143148532,
     34254498978062207918041301829525626783549813531091321004550549786528984401675),
    (48142684311216766702182564801462043940571084233680216669499475549492432046964,
     34380560660182334518990118617091967209302636551264477863958902286043397647879),
    (17348704025397475127937572481155408456556065464328870407269802701696798733683,
     24318278422173803457621119807961883607097742387673491974779969503617097905596),
    subgroup_order=0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7,
    cofactor=8,
    a=-1,
    d=19257038036680949359750312669786877991949435402254120286184196891950884077233,
    generator=(8076246640662884909881801758704306714034609987455869804520522091855516602923,
               13262374693698910701929044844600465831413122818447359594527400194675274060458),
    curve_id=_native.CURVE_JUBJUB,
    e2c="tai",
)

# dot_ring/curve/specs/bandersnatch_sw.py — Bandersnatch's prime-order group in short Weierstrass form (same n, cofactor 4), 33-byte
# points, try-and-increment hash-to-curve.  Ring proofs refuse it (RingProofParams), as the reference does.
_SW_PARAMS = SuiteParams(
    suite_id=b"Bandersnatch-SW-SHA512-TAI-v1", hash_fn=hashlib.sha512, xof=False,
    auxiliary_points=AuxiliaryPoints(
        (28115362618644671219696075022370511395136332234538034358311199318506963235315,
         3900851469868158154936962463930962496000252801946757953905982128670530185313),
        (13189182432637108534251278524663360416811744717379968387043749958796254980045,
         14483286006782706188671626508232161325054303360192563232232823772738911894793),
        (20496180070424734470560955314776462366297546779079302509428101119888111900885,
         8839106592405352067483360946162273985142890146060814748321063063028225641813)),
    a=BandersnatchSWPoint._SW_A,
    d=0,
    generator=(30900340493481298850216505686589334086208278925799850409469406976849338430199,
               12663882780877899054958035777720958383845500985908634476792678820121468453298),
    encoding=Encoding(point_len=33),
    curve_id=_native.CURVE_BANDERSNATCH_SW,
    e2c="tai",
)
Bandersnatch_SW = _variant(BandersnatchSWPoint, "Bandersnatch_SW", _SW_PARAMS)

# dot_ring/curve/specs/ed25519.py, the Ed25519_TAI variant (the reference exports it as Ed25519): its own field 2^255 - 19, a = -1,
# cofactor 8, try-and-increment with SHA-512; no accumulator base or padding point, so RingProofParams refuses it.  Every group
# operation runs on the Ed25519 kernels (DR_CURVE_ED25519).
Ed25519_TAI = _suite(
    "Ed25519_TAI", b"Ed25519-SHA512-TAI-v1", False,
    (45003173884697328536089278691112838614164406922820087464913813433380838325453,
     31256014272390301975555524011230972931324093235775711248505761870355310252869),
    None, None,
    field_modulus=0x7FFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFFED,
    subgroup_order=2**252 + 0x14DEF9DEA2F79CD65812631A5CF5D3ED,
    cofactor=8,
    a=-1,
    d=0x52036CEE2B6FFE738CC740797779E89800700A4D4141D8AB75EB4DCA135978A3,
    generator=(0x216936D3CD6E53FEC0A4E231FDD6DC5C692CC7609525A7B2C9562D608F25D51A,
               0x6666666666666666666666666666666666666666666666666666666666666658),
    curve_id=_native.CURVE_ED25519,
    e2c="tai",
)
Ed25519 = Ed25519_TAI


# Ed25519_RO / Ed25519_NU (specs/ed25519.py: the same params, E2C_Variant.ELL2 / ELL2_NU): hashing to the curve by RFC 9380's
# edwards25519_XMD:SHA-512_ELL2_RO_ (two field elements) or ..._NU_ (one); the suite id is the TAI variant's, as in the reference, so the
# variant travels in the curve id (DR_CURVE_ED25519_RO / DR_CURVE_ED25519_NU).
_ED25519_RO_PARAMS = dataclasses.replace(Ed25519_TAI.curve.params, curve_id=_native.CURVE_ED25519_RO, e2c="ell2")
Ed25519_RO = _te_variant(Ed25519Ell2Point, "Ed25519_RO", _ED25519_RO_PARAMS)
Ed25519_NU = _te_variant(Ed25519Ell2Point, "Ed25519_NU", _nu(_ED25519_RO_PARAMS, _native.CURVE_ED25519_NU))

# dot_ring/curve/specs/p256.py, the P256_TAI variant (the reference exports it as P256): NIST P-256 over its own field, a = -3,
# cofactor 1, 33-byte points, try-and-increment with SHA-256; no accumulator base or padding point, and not twisted Edwards, so
# RingProofParams refuses it.  Every group operation runs on the P-256 kernels (DR_CURVE_P256).
_P256_PARAMS = SuiteParams(
    suite_id=b"Secp256r1-SHA256-TAI-v1", hash_fn=hashlib.sha256, xof=False,
    auxiliary_points=AuxiliaryPoints(
        (100063053743935619201936855760019111820847755970243670581468062459849338000,
         113675507039234898358330549589155441528265243038226986303017485279501143145422),
        None, None),
    field_modulus=P256Point._P,
    subgroup_order=P256Point._N,
    cofactor=1,
    a=-3,
    d=0,
    generator=(0x6B17D1F2E12C4247F8BCE6E563A440F277037D812DEB33A0F4A13945D898C296,
               0x4FE342E2FE1A7F9B8EE7EB4A7C0F9E162BCE33576B315ECECBB6406837BF51F5),
    encoding=Encoding(point_len=33),
    curve_id=_native.CURVE_P256,
    e2c="tai",
)
P256_TAI = _variant(P256Point, "P256_TAI", _P256_PARAMS)
P256 = P256_TAI


# P256_RO / P256_NU (specs/p256.py: the same params, E2C_Variant.SSWU / SSWU_NU): hashing to the curve by RFC 9380's
# P256_XMD:SHA-256_SSWU_RO_ (two field elements) or ..._NU_ (one), points in SEC1 form; the suite id is the TAI variant's, as in the
# reference, so the variant travels in the curve id (DR_CURVE_P256_RO / DR_CURVE_P256_NU).  Not twisted Edwards: RingProofParams refuses them.
_P256_RO_PARAMS = dataclasses.replace(_P256_PARAMS, curve_id=_native.CURVE_P256_RO, e2c="sswu")
P256_RO = _variant(P256SswuPoint, "P256_RO", _P256_RO_PARAMS)
P256_NU = _variant(P256SswuPoint, "P256_NU", _nu(_P256_RO_PARAMS, _native.CURVE_P256_NU))

# dot_ring/curve/specs/baby_jubjub.py: a = 1 over the BN254 scalar field, cofactor 8, try-and-increment with SHA-512 (the candidates lose
# bit 254, as the reference masks them to the field's bit length).  It carries all three auxiliary points, but RingProofParams refuses
# it as the reference does: the 2048-th root of unity of the ring proofs is not one mod this p.  Every group operation runs on the Baby
# JubJub kernels (DR_CURVE_BABYJUBJUB).
BabyJubJub = _suite(
    "BabyJubJub", b"BabyJubJub-SHA512-TAI-v1", False,
    (15549380791300914366206471199568039679131690710803662429646809536753521087193,
     15218614024055502695611547593111691164731001864276292210438920202280814188379),
    (6402374321243162085389111671722843560682527921646684137786768606010797479351,
     9735581299071570006712034490635195155689931359428941496570758703259384062170),
    (11167490195257431015694161063225325511805242064780376648595733691987293447528,
     18403369502642103292159933062507105566469227524991433735553439433605496057425),
    field_modulus=21888242871839275222246405745257275088548364400416034343698204186575808495617,
    subgroup_order=2736030358979909402780800718157159386076813972158567259200215660948447373041,
    cofactor=8,
    a=1,
    d=9706598848417545097372247223557719406784115219466060233080913168975159366771,
    generator=(19698561148652590122159747500897617769866003486955115824547446575314762165298,
               19298250018296453272277890825869354524455968081175474282777126169995084727839),
    curve_id=_native.CURVE_BABYJUBJUB,
    e2c="tai",
)

# dot_ring/curve/specs/secp256k1.py: y^2 = x^3 + 7 over 2^256 - 2^32 - 977, cofactor 1, 33-byte SEC1 points, SHA-256, hashing to the curve by
# RFC 9380's secp256k1_XMD:SHA-256_SSWU_RO_ (two field elements) or ..._NU_ (one); both variants carry the RO suite id, as in the
# reference.  No accumulator base or padding point, and not twisted Edwards, so RingProofParams refuses them.  Every group operation and
# the map run on the secp256k1 kernels (DR_CURVE_SECP256K1 / DR_CURVE_SECP256K1_NU).
_SECP256K1_PARAMS = SuiteParams(
    suite_id=b"secp256k1_XMD:SHA-256_SSWU_RO_", hash_fn=hashlib.sha256, xof=False,
    auxiliary_points=AuxiliaryPoints(
        (0x50929B74C1A04954B78B4B6035E97A5E078A5A0F28EC96D547BFEE9ACE803AC0,
         0x31D3C6863973926E049E637CB1B5F40A36DAC28AF1766968C30C2313F3A38904),
        None, None),
    field_modulus=Secp256k1Point._P,
    subgroup_order=Secp256k1Point._N,
    cofactor=1,
    a=0,
    d=0,
    generator=(0x79BE667EF9DCBBAC55A06295CE870B07029BFCDB2DCE28D959F2815B16F81798,
               0x483ADA7726A3C4655DA4FBFC0E1108A8FD17B448A68554199C47D08FFB10D4B8),
    encoding=Encoding(point_len=33),
    curve_id=_native.CURVE_SECP256K1,
    e2c="sswu",
)
Secp256k1_RO = _variant(Secp256k1Point, "Secp256k1_RO", _SECP256K1_PARAMS)
Secp256k1_NU = _variant(Secp256k1Point, "Secp256k1_NU", _nu(_SECP256K1_PARAMS, _native.CURVE_SECP256K1_NU))
Secp256k1 = Secp256k1_RO

# dot_ring/curve/specs/curve25519.py: v^2 = u^3 + 486662 u^2 + u over 2^255 - 19, Ed25519's group (cofactor 8) in Montgomery form, points
# 64 bytes u || v (point_len 32, uncompressed), SHA-512, hashing to the curve by RFC 9380's curve25519_XMD:SHA-512_ELL2_RO_ (two field
# elements) or ..._NU_ (one); both variants share the RO suite id and the generator as Pedersen blinding base, as in the reference.  No
# accumulator base or padding point, and not twisted Edwards, so RingProofParams refuses them.
_CURVE25519_G = (9, 14781619447589544791020593568409986887264606134616475288964881837755586237401)
_CURVE25519_PARAMS = SuiteParams(
    suite_id=b"curve25519_XMD:SHA-512_ELL2_RO_", hash_fn=hashlib.sha512, xof=False,
    auxiliary_points=AuxiliaryPoints(_CURVE25519_G, None, None),
    field_modulus=Curve25519Point._P,
    subgroup_order=Curve25519Point._N,
    cofactor=8,
    a=Curve25519Point._MG_A,
    d=1,                                       # (the Montgomery B)
    generator=_CURVE25519_G,
    encoding=Encoding(point_len=32, uncompressed=True),
    curve_id=_native.CURVE_CURVE25519_RO,
    e2c="ell2",
)
Curve25519_RO = _variant(Curve25519Point, "Curve25519_RO", _CURVE25519_PARAMS)
Curve25519_NU = _variant(Curve25519Point, "Curve25519_NU", _nu(_CURVE25519_PARAMS, _native.CURVE_CURVE25519_NU))
Curve25519 = Curve25519_RO


# dot_ring/curve/specs/bls12_381_G1.py: E: y^2 = x^3 + 4 over the 381-bit Fq, #E(Fq) = h r, hashing by RFC 9380's
# BLS12381G1_XMD:SHA-256_SSWU_RO_ (two field elements) or ..._NU_ (one), `cofactor` = h_eff; both variants carry the RO suite id, as in the
# reference.  Encoding(point_len=32, challenge_len=48) are the reference's own figures; its points encode to 49 bytes, which point_len =
# 32 contradicts, so the reference can decode no key or proof of this curve — the VRF classes refuse these two suites (vrf/base.py) and
# what is served is the point type and curve.valid_point.  No auxiliary points, not twisted Edwards: RingProofParams refuses them too.
_BLS12_381_G1_PARAMS = SuiteParams(
    suite_id=b"BLS12381G1_XMD:SHA-256_SSWU_RO_", hash_fn=hashlib.sha256, xof=False,
    auxiliary_points=AuxiliaryPoints(None, None, None),
    field_modulus=Bls12381G1Point._P,
    subgroup_order=Bls12381G1Point._N,
    cofactor=Bls12381G1Point._H,
    a=0,
    d=0,
    generator=(0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
               0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1),
    encoding=Encoding(point_len=32, challenge_len=48),
    curve_id=_native.CURVE_BLS12_381_G1,
    e2c="sswu",
)
BLS12_381_G1_RO = _variant(Bls12381G1Point, "BLS12_381_G1_RO", _BLS12_381_G1_PARAMS)
BLS12_381_G1_NU = _variant(Bls12381G1Point, "BLS12_381_G1_NU", _nu(_BLS12_381_G1_PARAMS, _native.CURVE_BLS12_381_G1_NU))
BLS12_381_G1 = BLS12_381_G1_RO


# dot_ring/curve/specs/bls12_381_G2.py: E: y^2 = x^3 + 4 (1 + i) over Fq2, #E(Fq2) = h2 r, hashing by RFC 9380's
# BLS12381G2_XMD:SHA-256_SSWU_RO_ (two field elements) or ..._NU_ (one), `cofactor` = the 636-bit h_eff; both variants carry the RO suite
# id, as in the reference.  Encoding(point_len=32, challenge_len=32) are the reference's own figures; it has NO point codec for this curve
# (point_to_string / string_to_point raise), so no key or proof can be encoded — the VRF classes refuse these two suites (vrf/base.py)
# and what is served is the point type.  No auxiliary points, not twisted Edwards: RingProofParams refuses them too.
_fp2 = lambda re, im: Fp2(re, im, Bls12381G2Point._P)  # noqa: E731
_BLS12_381_G2_PARAMS = SuiteParams(
    suite_id=b"BLS12381G2_XMD:SHA-256_SSWU_RO_", hash_fn=hashlib.sha256, xof=False,
    auxiliary_points=AuxiliaryPoints(None, None, None),
    field_modulus=Bls12381G2Point._P,
    subgroup_order=Bls12381G2Point._N,
    cofactor=Bls12381G2Point._H,
    a=0,
    d=0,
    generator=(_fp2(0x024AA2B2F08F0A91260805272DC51051C6E47AD4FA403B02B4510B647AE3D1770BAC0326A805BBEFD48056C8C121BDB8,
                    0x13E02B6052719F607DACD3A088274F65596BD0D09920B61AB5DA61BBDC7F5049334CF11213945D57E5AC7D055D042B7E),
               _fp2(0x0CE5D527727D6E118CC9CDC6DA2E351AADFD9BAA8CBDD3A76D429A695160D12C923AC9CC3BACA289E193548608B82801,
                    0x0606C4A02EA734CC32ACD2B02BC28B99CB3E287E85A763AF267492AB572E99AB3F370D275CEC1DA1AAA9075FF05F79BE)),
    encoding=Encoding(point_len=32, challenge_len=32),
    curve_id=_native.CURVE_BLS12_381_G2,
    e2c="sswu",
)
BLS12_381_G2_RO = _variant(Bls12381G2Point, "BLS12_381_G2_RO", _BLS12_381_G2_PARAMS)
BLS12_381_G2_NU = _variant(Bls12381G2Point, "BLS12_381_G2_NU", _nu(_BLS12_381_G2_PARAMS, _native.CURVE_BLS12_381_G2_NU))
BLS12_381_G2 = BLS12_381_G2_RO


# dot_ring/curve/specs/ed448.py: x^2 + y^2 = 1 - 39081 x^2 y^2 over 2^448 - 2^224 - 1, cofactor 4, points 112 bytes x || y (point_len 56,
# uncompressed), 56-byte scalars, SHAKE256 as transcript XOF, hashing to the curve by RFC 9380's edwards448_XOF:SHAKE256_ELL2_RO_ (two
# field elements) or ..._NU_ (one); both variants share the RO suite id and the generator as Pedersen blinding base, as in the reference.
# No accumulator base or padding point, so RingProofParams refuses them.
_ED448_G = (117812161263436946737282484343310064665180535357016373416879082147939404277809514858788439644911793978499419995990477371552926308078495,
            19)
_ED448_PARAMS = SuiteParams(
    suite_id=b"edwards448_XOF:SHAKE256_ELL2_RO_", hash_fn=hashlib.shake_256, xof=True,
    auxiliary_points=AuxiliaryPoints(_ED448_G, None, None),
    field_modulus=Ed448Point._P,
    subgroup_order=Ed448Point._N,
    cofactor=4,
    a=1,
    d=-39081,
    generator=_ED448_G,
    encoding=Encoding(point_len=56, challenge_len=64, uncompressed=True),
    curve_id=_native.CURVE_ED448_RO,
    e2c="ell2",
)
Ed448_RO = _variant(Ed448Point, "Ed448_RO", _ED448_PARAMS)
Ed448_NU = _variant(Ed448Point, "Ed448_NU", _nu(_ED448_PARAMS, _native.CURVE_ED448_NU))
Ed448 = Ed448_RO


# dot_ring/curve/specs/curve448.py: v^2 = u^3 + 156326 u^2 + u over 2^448 - 2^224 - 1, cofactor 4, points 112 bytes u || v (point_len 56,
# uncompressed), SHAKE256 transcript; no accumulator base and no padding point (no ring proofs).  Both variants share the suite id, as in
# the reference.  challenge_len = 28 is the reference's own figure; its VRF layer squeezes 16 bytes whatever this says, and so does this one.
_CURVE448_G = (5, 355293926785568175264127502063783334808976399387714271831880898435169088786967410002932673765864550910142774147268105838985595290606362)
_CURVE448_PARAMS = SuiteParams(
    suite_id=b"curve448_XOF:SHAKE256_ELL2_RO_", hash_fn=hashlib.shake_256, xof=True,
    auxiliary_points=AuxiliaryPoints(_CURVE448_G, None, None),
    field_modulus=Curve448Point._P,
    subgroup_order=Curve448Point._N,
    cofactor=4,
    a=156326,
    d=1,                          # (the reference's b)
    generator=_CURVE448_G,
    encoding=Encoding(point_len=56, challenge_len=28, uncompressed=True),
    curve_id=_native.CURVE_CURVE448_RO,
    e2c="ell2",
)
Curve448_RO = _variant(Curve448Point, "Curve448_RO", _CURVE448_PARAMS)
Curve448_NU = _variant(Curve448Point, "Curve448_NU", _nu(_CURVE448_PARAMS, _native.CURVE_CURVE448_NU))
Curve448 = Curve448_RO


# dot_ring/curve/specs/p521.py: y^2 = x^3 - 3 x + b over 2^521 - 1, prime order, cofactor 1, SEC1 compressed points of 67 bytes, 66-byte
# scalars, SHA-512 transcripts, hashing to the curve by RFC 9380's P521_XMD:SHA-512_SSWU_RO_ (two field elements, L = 98, Z = -4) or
# ..._NU_ (one); both variants share the RO suite id, and the Pedersen blinding base IS the generator, as in the reference.  No accumulator
# base or padding point and not twisted Edwards: RingProofParams refuses them.  challenge_len = 32 is the reference's own figure; its VRF
# layer squeezes 16 bytes whatever this says, and so does this one.
_P521_G = (0x00C6858E06B70404E9CD9E3ECB662395B4429C648139053FB521F828AF606B4D3DBAA14B5E77EFE75928FE1DC127A2FFA8DE3348B3C1856A429BF97E7E31C2E5BD66,
           0x011839296A789A3BC0045C8A5FB42C7D1BD998F54449579B446817AFBD17273E662C97EE72995EF42640C550B9013FAD0761353C7086A272C24088BE94769FD16650)
_P521_PARAMS = SuiteParams(
    suite_id=b"P521_XMD:SHA-512_SSWU_RO_", hash_fn=hashlib.sha512, xof=False,
    auxiliary_points=AuxiliaryPoints(_P521_G, None, None),
    field_modulus=P521Point._P,
    subgroup_order=P521Point._N,
    cofactor=1,
    a=-3,
    d=P521Point._SW_B,            # (the reference's b)
    generator=_P521_G,
    encoding=Encoding(point_len=67, challenge_len=32),
    curve_id=_native.CURVE_P521_RO,
    e2c="sswu",
)
P521_RO = _variant(P521Point, "P521_RO", _P521_PARAMS)
P521_NU = _variant(P521Point, "P521_NU", _nu(_P521_PARAMS, _native.CURVE_P521_NU))
P521 = P521_RO


# dot_ring/curve/specs/p384.py: y^2 = x^3 - 3 x + b over 2^384 - 2^128 - 2^96 + 2^32 - 1, prime order, cofactor 1, SEC1 compressed points
# of 49 bytes, 48-byte scalars, SHA-384 transcripts (the first suite with a 48-byte digest), hashing to the curve by RFC 9380's
# P384_XMD:SHA-384_SSWU_RO_ (two field elements, L = 72, Z = -12) or ..._NU_ (one); both variants share the RO suite id, and the Pedersen
# blinding base IS the generator, as in the reference.  Not twisted Edwards: RingProofParams refuses them.  challenge_len = 24 is the
# reference's own figure; its VRF layer squeezes 16 bytes whatever this says, and so does this one.
_P384_G = (0xAA87CA22BE8B05378EB1C71EF320AD746E1D3B628BA79B9859F741E082542A385502F25DBF55296C3A545E3872760AB7,
           0x3617DE4A96262C6F5D9E98BF9292DC29F8F41DBD289A147CE9DA3113B5F0B8C00A60B1CE1D7E819D7A431D7C90EA0E5F)
_P384_PARAMS = SuiteParams(
    suite_id=b"P384_XMD:SHA-384_SSWU_RO_", hash_fn=hashlib.sha384, xof=False,
    auxiliary_points=AuxiliaryPoints(_P384_G, None, None),
    field_modulus=P384Point._P,
    subgroup_order=P384Point._N,
    cofactor=1,
    a=-3,
    d=P384Point._SW_B,            # (the reference's b)
    generator=_P384_G,
    encoding=Encoding(point_len=49, challenge_len=24),
    curve_id=_native.CURVE_P384_RO,
    e2c="sswu",
)
P384_RO = _variant(P384Point, "P384_RO", _P384_PARAMS)
P384_NU = _variant(P384Point, "P384_NU", _nu(_P384_PARAMS, _native.CURVE_P384_NU))
P384 = P384_RO
