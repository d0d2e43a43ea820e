"""dot_ring_amd — MI355X-native (gfx950) Ring-VRF hot path behind dot-ring's Python API.

The arithmetic lives in libdotring_hip.so (hand-written HIP, see dot_ring_amd/csrc and include/dotring_hip.h);
this package mirrors the reference's public names (dot_ring/__init__.py:3-19) for the Bandersnatch suites, JubJub, Ed25519, P-256,
Baby JubJub, secp256k1, Curve25519, Ed448, Curve448, P-521, P-384 and (the point types and hashing only: no VRF) BLS12-381 G1 and G2:
    TinyVRF, ThinVRF, PedersenVRF, RingVRF, Ring, RingRoot, RingProofParams, Bandersnatch, Bandersnatch_SHAKE128, JubJub, Bandersnatch_SW,
    Ed25519 (= Ed25519_TAI), Ed25519_RO, Ed25519_NU, P256 (= P256_TAI), P256_RO, P256_NU, BabyJubJub, Secp256k1 (= Secp256k1_RO),
    Secp256k1_NU, Curve25519 (= Curve25519_RO), Curve25519_NU, BLS12_381_G1 (= BLS12_381_G1_RO), BLS12_381_G1_NU,
    BLS12_381_G2 (= BLS12_381_G2_RO), BLS12_381_G2_NU, Ed448 (= Ed448_RO), Ed448_NU
plus the additive prove_batch() entry points.  Curve448 (= Curve448_RO), Curve448_RO and Curve448_NU, and likewise P521 (= P521_RO), P521_RO
and P521_NU and P384 (= P384_RO), P384_RO and P384_NU, are module attributes that __all__ does not list yet: the recorded point surface (tests/golden/point_surface_cpu.json) names the variants of __all__ one by one.  There is no CPU fallback for the kernels.
"""
from . import _native  # noqa: F401
from .curve import (BLS12_381_G1, BLS12_381_G1_NU, BLS12_381_G1_RO, BLS12_381_G2, BLS12_381_G2_NU, BLS12_381_G2_RO, P256, P256_NU, P256_RO, P256_TAI, BabyJubJub, Bandersnatch, Bandersnatch_SHAKE128, Bandersnatch_SW, Curve25519,
                    Curve25519_NU, Curve25519_RO, Ed448, Ed448_NU, Ed448_RO, Ed25519, Ed25519_NU, Ed25519_RO, Ed25519_TAI, JubJub, Secp256k1, Secp256k1_NU, Secp256k1_RO)
from .curve import Curve448, Curve448_NU, Curve448_RO  # noqa: F401  (attributes, not in __all__: see above)
from .curve import P521, P521_NU, P521_RO  # noqa: F401  (the same convention)
from .curve import P384, P384_NU, P384_RO  # noqa: F401  (the same convention)
from .ring_proof.params import RingProofParams
from .ring_proof.pcs import KZG
from .vrf.pedersen import PedersenVRF
from .vrf.ring_vrf import Ring, RingRoot, RingVRF
from .vrf.thin import ThinVRF
from .vrf.tiny import TinyVRF

__all__ = ["TinyVRF", "ThinVRF", "PedersenVRF", "RingVRF", "Ring", "RingRoot", "RingProofParams", "KZG",
           "Bandersnatch", "Bandersnatch_SHAKE128", "JubJub", "Bandersnatch_SW", "Ed25519", "Ed25519_TAI", "P256", "P256_TAI",
           "BabyJubJub", "Secp256k1", "Secp256k1_RO", "Secp256k1_NU", "P256_RO", "P256_NU", "Ed25519_RO", "Ed25519_NU",
           "Curve25519", "Curve25519_RO", "Curve25519_NU", "BLS12_381_G1", "BLS12_381_G1_RO", "BLS12_381_G1_NU",
           "BLS12_381_G2", "BLS12_381_G2_RO", "BLS12_381_G2_NU", "Ed448", "Ed448_RO", "Ed448_NU"]
