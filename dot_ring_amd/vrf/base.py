"""Common base of the four schemes: `Scheme[curve_variant]` yields the scheme bound to one suite
(reference behaviour: dot_ring/vrf/vrf.py:10-48).  Bound classes are created once per (scheme, suite) and reused, so
dataclass equality between proofs works and per-class memos survive."""
from __future__ import annotations

from .. import _native
from ..curve import CurveVariant

_BOUND: dict = {}


def _unsupported(owner, what: str):
    name = owner.__name__ if isinstance(owner, type) else type(owner).__name__
    return NotImplementedError(f"{name} does not implement {what}")


class VRF:
    cv = None
    RING = False                  # RingVRF alone: the scheme carries a ring proof

    def __class_getitem__(cls, variant):
        if not isinstance(variant, CurveVariant):
            return cls
        if variant.curve.params.curve_id in (_native.CURVE_BLS12_381_G1, _native.CURVE_BLS12_381_G1_NU):
            # a deliberate deviation: the reference binds the class and can then decode nothing
            raise ValueError(f"{cls.__name__} has no {variant.name} suite: the reference's point length for this curve is 32 while its points "
                             "encode to 49 bytes, so no key or proof of it can be decoded")
        if variant.curve.params.curve_id in (_native.CURVE_BLS12_381_G2, _native.CURVE_BLS12_381_G2_NU):
            #  the reference binds the class and then fails at its first point_to_string
            raise ValueError(f"{cls.__name__} has no {variant.name} suite: the curve has no point codec (point_to_string and "
                             "string_to_point are not implemented), so no key or proof of it can be encoded")
        if cls.RING and variant.curve.params.curve_id in (_native.CURVE_ED448_RO, _native.CURVE_ED448_NU):
            #  no accumulator base or padding point, as RingProofParams says, and the ring proof's columns are 32-byte scalars
            raise ValueError(f"{cls.__name__} has no {variant.name} suite: the curve has no accumulator base and no padding point, and its "
                             "56-byte coordinates do not fit the ring proof's columns")
        if cls.RING and variant.curve.params.curve_id in (_native.CURVE_CURVE448_RO, _native.CURVE_CURVE448_NU):
            # a Montgomery curve, as RingProofParams says, and the ring proof's columns are 32-byte scalars
            raise ValueError(f"{cls.__name__} has no {variant.name} suite: ring proofs require a Twisted Edwards curve, and its 56-byte "
                             "coordinates do not fit the ring proof's columns")
        if cls.RING and variant.curve.params.curve_id in (_native.CURVE_P521_RO, _native.CURVE_P521_NU, _native.CURVE_P384_RO, _native.CURVE_P384_NU):
            # a short Weierstrass curve, as RingProofParams says, and the ring proof's columns are 32-byte scalars
            raise ValueError(f"{cls.__name__} has no {variant.name} suite: ring proofs require a Twisted Edwards curve, and its "
                             f"{variant.point_type._SEC1_LEN}-byte coordinates do not fit the ring proof's columns")
        bound = _BOUND.get((cls, variant.name))
        if bound is None or bound.cv is not variant:
            bound = _BOUND[(cls, variant.name)] = type(f"{cls.__name__}[{variant.name}]", (cls,), {"cv": variant})
        return bound

    # the interface every scheme fills in
    @classmethod
    def prove(cls, *args, **kwargs):
        raise _unsupported(cls, "prove")

    def verify(self, *args, **kwargs):
        raise _unsupported(self, "verify")

    def encode(self) -> bytes:
        raise _unsupported(self, "encode")

    @classmethod
    def decode(cls, data: bytes):
        raise _unsupported(cls, "from_bytes")

    @classmethod
    def batch_verify(cls, *args, **kwargs):
        raise _unsupported(cls, "batch_verify")
