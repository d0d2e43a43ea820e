"""ctypes binding of libdotring_hip.so (include/dotring_hip.h) — the only door from Python to the GPU kernels.

No CPU fallback exists: if the shared library is missing, or there is no gfx950 device, the calls raise.
Error mapping follows the reference's exception types at these seams (ValueError / MemoryError).
"""
from __future__ import annotations

import array
import ctypes
import functools
import itertools
import threading
import os
from ctypes import POINTER, byref, c_char_p, c_double, c_int, c_size_t, c_uint, c_void_p
from typing import NamedTuple

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libdotring_hip.so")

DR_OK, DR_ERR_INVALID, DR_ERR_NOMEM, DR_ERR_DEVICE, DR_ERR_NOTSQUARE = 0, -1, -2, -3, -4


class DotRingHipError(RuntimeError):
    """HIP runtime failure, or no usable MI355X device."""


_lib = None

# name -> (restype, argtypes); mirrors include/dotring_hip.h one to one
_PROTOTYPES = {
    "dr_version": (c_char_p, []),
    "dr_last_error": (c_char_p, []),
    "dr_device_count": (c_int, []),
    "dr_ctx_create": (c_int, [c_int, POINTER(c_void_p)]),
    "dr_ctx_destroy": (None, [c_void_p]),
    "dr_ctx_sync": (c_int, [c_void_p]),
    "dr_dev_alloc": (c_int, [c_void_p, c_size_t, POINTER(c_void_p)]),
    "dr_dev_free": (c_int, [c_void_p, c_void_p]),
    "dr_dev_upload": (c_int, [c_void_p, c_void_p, c_char_p, c_size_t]),
    "dr_dev_download": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t]),
    "dr_prof_enable": (c_int, [c_void_p, c_int]),
    "dr_prof_reset": (c_int, [c_void_p]),
    "dr_prof_get": (c_int, [c_void_p, c_char_p, POINTER(c_double), POINTER(c_int)]),
    "dr_bsn_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p]),
    "dr_bsn_scalar_mul_batch_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p]),
    "dr_bsn_msm": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p]),
    "dr_bsn_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_void_p]),
    "dr_bsn_encode_to_curve_batch": (c_int, [c_void_p, c_char_p, c_size_t, c_void_p]),
    "dr_fr_sqrt": (c_int, [c_char_p, c_void_p]),
    "dr_fr_ops_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_srs_load": (c_int, [c_void_p, c_char_p, c_size_t, POINTER(c_void_p)]),
    "dr_srs_synthetic": (c_int, [c_void_p, c_char_p, c_uint, c_size_t, POINTER(c_void_p)]),
    "dr_srs_powers": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, POINTER(c_void_p)]),
    "dr_g2_mul": (c_int, [c_char_p, c_char_p, c_char_p]),
    "dr_srs_precompute": (c_int, [c_void_p, c_void_p, c_int]),
    "dr_srs_table_info": (c_int, [c_void_p, c_size_t, c_size_t, POINTER(c_int)]),
    "dr_srs_precompute_multiples": (c_int, [c_void_p, c_void_p, c_int, c_int]),
    "dr_srs_table_info_multiples": (c_int, [c_void_p, c_size_t, c_size_t, POINTER(c_int)]),
    "dr_srs_download": (c_int, [c_void_p, c_void_p, c_size_t, c_size_t, c_void_p]),
    "dr_srs_destroy": (None, [c_void_p]),
    "dr_srs_size": (c_size_t, [c_void_p]),
    "dr_g1_msm": (c_int, [c_void_p, c_void_p, c_size_t, c_char_p, c_size_t, c_void_p, POINTER(c_int)]),
    "dr_g1_msm_dev": (c_int, [c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, POINTER(c_int)]),
    "dr_g1_msm_batch": (c_int, [c_void_p, c_void_p, c_char_p, c_size_t, c_size_t, c_void_p, POINTER(c_int)]),
    "dr_g1_msm_batch_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_size_t, c_void_p, POINTER(c_int)]),
    "dr_g1_msm_points": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, POINTER(c_int)]),
    "dr_g1_sum": (c_int, [c_char_p, c_size_t, c_void_p, POINTER(c_int)]),
    "dr_pairing_check": (c_int, [c_char_p, c_char_p, c_size_t, POINTER(c_int)]),
    "dr_g1_compress": (c_int, [c_char_p, c_int, c_void_p]),
    "dr_g1_decompress": (c_int, [c_char_p, c_void_p, POINTER(c_int)]),
    "dr_g1_serialize_check": (c_int, [c_char_p]),
    "dr_ring_prover_create": (c_int, [c_void_p, c_void_p, c_uint, c_uint, c_char_p, c_char_p, c_char_p, c_char_p, POINTER(c_void_p)]),
    "dr_ring_prover_destroy": (None, [c_void_p]),
    "dr_ring_prover_root": (c_int, [c_void_p, c_void_p, POINTER(c_int)]),
    "dr_ring_prover_fixed_coeffs": (c_int, [c_void_p, c_void_p]),
    "dr_ring_prover_peek": (c_int, [c_void_p, c_int, c_void_p, c_size_t]),
    "dr_ring_prove_witness": (c_int, [c_void_p, c_size_t, c_void_p, c_char_p, c_char_p, c_void_p, c_void_p, POINTER(c_int)]),
    "dr_ring_prove_quotient": (c_int, [c_void_p, c_size_t, c_char_p, c_void_p, POINTER(c_int)]),
    "dr_ring_prove_evals": (c_int, [c_void_p, c_size_t, c_char_p, c_void_p]),
    "dr_ring_prove_openings": (c_int, [c_void_p, c_size_t, c_char_p, c_void_p, POINTER(c_int)]),
    "dr_ctx_scratch_residue": (c_int, [c_void_p, POINTER(ctypes.c_uint64)]),
    "dr_ring_prover_wipe": (c_int, [c_void_p]),
    "dr_ring_prover_residue": (c_int, [c_void_p, POINTER(ctypes.c_uint64)]),
    "dr_ntt": (c_int, [c_void_p, c_void_p, c_uint, c_size_t, c_char_p, c_char_p]),
    "dr_ntt_dev": (c_int, [c_void_p, c_void_p, c_uint, c_size_t, c_char_p, c_char_p]),
    "dr_ntt_formats_selftest": (c_int, [c_void_p, c_char_p, c_size_t, c_char_p, c_size_t, c_char_p, c_size_t, c_uint, c_size_t, c_char_p,
                                        c_char_p, c_int, c_int, c_int, ctypes.c_uint32, c_void_p]),
}


class VrfSuiteStruct(ctypes.Structure):
    """dr_vrf_suite (include/dotring_hip.h)."""
    _fields_ = [("suite_id", c_char_p), ("suite_id_len", c_size_t), ("xof", c_int),
                ("generator_xy", ctypes.c_uint8 * 64), ("blinding_base_xy", ctypes.c_uint8 * 64), ("curve", c_int)]


class RingVerifierKeyStruct(ctypes.Structure):
    """dr_ring_verifier_key (include/dotring_hip.h)."""
    _fields_ = [("log2n", ctypes.c_uint), ("omega_n", ctypes.c_uint8 * 32), ("seed_xy", ctypes.c_uint8 * 64),
                ("fixed_commitments", ctypes.c_uint8 * 288), ("g1_generator", ctypes.c_uint8 * 96), ("g2", ctypes.c_uint8 * 384),
                ("fs_prefix", c_char_p), ("fs_prefix_len", c_size_t)]


_PROTOTYPES.update({
    "dr_ringvrf_verify_batch": (c_int, [c_void_p, POINTER(VrfSuiteStruct), POINTER(RingVerifierKeyStruct), c_size_t, c_char_p, c_char_p,
                                        POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64),
                                        c_char_p, POINTER(c_int)]),
    "dr_g1_decompress_batch": (c_int, [c_void_p, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_fq_ops_selftest": (c_int, [c_void_p, c_char_p, c_size_t, c_void_p]),
    "dr_g1_ops_selftest": (c_int, [c_void_p, c_char_p, c_size_t, c_void_p]),
    "dr_bsn_decode_points": (c_int, [c_void_p, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_te_scalar_mul_batch": (c_int, [c_void_p, c_int, c_char_p, c_char_p, c_size_t, c_void_p]),
    "dr_te_msm": (c_int, [c_void_p, c_int, c_char_p, c_char_p, c_size_t, c_void_p]),
    "dr_te_msm_groups": (c_int, [c_void_p, c_int, c_char_p, c_char_p, c_size_t, c_size_t, c_void_p]),
    "dr_te_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_ed25519_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_fe25519_ops_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_p256_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_p256_field_ops_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_secp256k1_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_secp256k1_field_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_secp256k1_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_char_p, c_char_p]),
    "dr_p256_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_char_p, c_char_p]),
    "dr_ed25519_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_char_p, c_char_p]),
    "dr_bjj_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_blsg1_hash_to_field_batch": (c_int, [c_int, c_char_p, POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_blsg1_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_int, c_char_p, c_char_p]),
    "dr_blsg1_encode_to_curve_batch": (c_int, [c_void_p, c_int, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_size_t,
                                               c_char_p]),
    "dr_blsg1_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_blsg1_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p]),
    "dr_blsg1_msm": (c_int, [c_void_p, c_int, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_blsg1_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_blsg1_field_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_blsg2_hash_to_field_batch": (c_int, [c_int, c_char_p, POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_blsg2_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_int, c_char_p, c_char_p]),
    "dr_blsg2_encode_to_curve_batch": (c_int, [c_void_p, c_int, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_size_t,
                                               c_char_p]),
    "dr_blsg2_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_blsg2_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p]),
    "dr_blsg2_msm": (c_int, [c_void_p, c_int, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_blsg2_check_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p]),
    "dr_blsg2_field_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_ed448_hash_to_field_batch": (c_int, [c_int, c_char_p, POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_ed448_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_int, c_char_p, c_char_p]),
    "dr_ed448_encode_to_curve_batch": (c_int, [c_void_p, c_int, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_size_t,
                                               c_char_p]),
    "dr_ed448_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_ed448_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p]),
    "dr_ed448_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_ed448_field_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_curve448_hash_to_field_batch": (c_int, [c_int, c_char_p, POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_curve448_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_int, c_char_p, c_char_p]),
    "dr_curve448_encode_to_curve_batch": (c_int, [c_void_p, c_int, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_size_t,
                                                  c_char_p]),
    "dr_curve448_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_curve448_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p]),
    "dr_curve448_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_p521_hash_to_field_batch": (c_int, [c_int, c_char_p, POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_p521_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_int, c_char_p, c_char_p]),
    "dr_p521_encode_to_curve_batch": (c_int, [c_void_p, c_int, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_size_t,
                                      c_char_p]),
    "dr_p521_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_p521_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p]),
    "dr_p521_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_p521_field_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_p384_hash_to_field_batch": (c_int, [c_int, c_char_p, POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_p384_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_int, c_char_p, c_char_p]),
    "dr_p384_encode_to_curve_batch": (c_int, [c_void_p, c_int, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_size_t,
                                      c_char_p]),
    "dr_p384_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_p384_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p]),
    "dr_p384_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_p384_field_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_wide_msm": (c_int, [c_void_p, c_int, c_char_p, c_char_p, c_size_t, c_char_p]),
    "dr_curve25519_scalar_mul_batch": (c_int, [c_void_p, c_char_p, c_char_p, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_curve25519_msm_groups": (c_int, [c_void_p, c_char_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p, c_char_p]),
    "dr_curve25519_decode_points": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_char_p]),
    "dr_curve25519_map_to_curve": (c_int, [c_void_p, c_char_p, c_size_t, c_int, c_int, c_char_p, c_char_p]),
    "dr_bjj_field_ops_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p, c_void_p]),
    "dr_encode_to_curve_batch": (c_int, [c_void_p, POINTER(VrfSuiteStruct), c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                         POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_ring_prover_create_te": (c_int, [c_void_p, c_int, c_void_p, c_uint, c_uint, c_char_p, c_char_p, c_char_p, c_char_p, POINTER(c_void_p)]),
    "dr_pairing_selfcheck": (c_int, [c_char_p, c_char_p, c_size_t, POINTER(c_int)]),
    "dr_pedersen_prove_batch": (c_int, [c_void_p, POINTER(VrfSuiteStruct), c_size_t, c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                        POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p, c_char_p, c_char_p]),
    "dr_pedersen_verify_batch": (c_int, [c_void_p, POINTER(VrfSuiteStruct), c_size_t, c_char_p, c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                         POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), POINTER(c_int)]),
    "dr_ietf_prove_batch": (c_int, [c_void_p, POINTER(VrfSuiteStruct), c_int, c_size_t, c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                    POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p, c_char_p, c_char_p]),
    "dr_ietf_verify_batch": (c_int, [c_void_p, POINTER(VrfSuiteStruct), c_int, c_size_t, c_char_p, c_char_p, c_char_p, POINTER(ctypes.c_uint64),
                                     c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p]),
    "dr_ringvrf_prove_batch_multi": (c_int, [POINTER(c_void_p), c_size_t, POINTER(VrfSuiteStruct), c_size_t, c_char_p, POINTER(ctypes.c_uint64),
                                             c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                             POINTER(ctypes.c_uint32), c_char_p, c_size_t, c_char_p, c_char_p, c_char_p]),
    "dr_ringvrf_verify_batch_multi": (c_int, [POINTER(c_void_p), c_size_t, POINTER(VrfSuiteStruct), POINTER(RingVerifierKeyStruct), c_size_t,
                                              c_char_p, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                              POINTER(ctypes.c_uint64), c_char_p, POINTER(c_int)]),
    "dr_ringvrf_verify_each": (c_int, [c_void_p, POINTER(VrfSuiteStruct), POINTER(RingVerifierKeyStruct), c_size_t, c_char_p, c_char_p,
                                       POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64),
                                       c_char_p, c_char_p, POINTER(ctypes.c_uint32)]),
    "dr_ringvrf_verify_each_multi": (c_int, [POINTER(c_void_p), c_size_t, POINTER(VrfSuiteStruct), POINTER(RingVerifierKeyStruct), c_size_t,
                                             c_char_p, c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                             POINTER(ctypes.c_uint64), c_char_p, c_char_p, POINTER(ctypes.c_uint32)]),
    "dr_g1_claim_tree_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_size_t, c_char_p, c_char_p]),
    "dr_host_hash": (c_int, [c_int, c_char_p, c_size_t, c_char_p, c_size_t]),
    "dr_hash_to_field_batch": (c_int, [POINTER(VrfSuiteStruct), c_char_p, POINTER(ctypes.c_uint64), c_size_t, c_char_p]),
    "dr_ringvrf_prove_batch": (c_int, [c_void_p, POINTER(VrfSuiteStruct), c_size_t, c_char_p, POINTER(ctypes.c_uint64), c_char_p,
                                       POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint64), c_char_p, POINTER(ctypes.c_uint32),
                                       c_char_p, c_size_t, c_char_p, c_char_p, c_char_p]),
})
_PROTOTYPES.update({
    "dr_te_fixed_base_msm_groups": (c_int, [c_void_p, c_int, c_char_p, c_size_t, c_char_p, c_size_t, c_void_p]),
    "dr_host_random_expand": (c_int, [c_char_p, c_void_p, c_size_t]),
    "dr_ringvrf_aux_take_blindings": (c_int, [c_void_p, c_size_t, c_void_p]),
    "dr_comm_unique_id": (c_int, [c_char_p]),
    "dr_comm_create": (c_int, [c_void_p, c_char_p, c_int, c_int, POINTER(c_void_p)]),
    "dr_comm_destroy": (None, [c_void_p]),
    "dr_comm_rank": (c_int, [c_void_p]),
    "dr_comm_world": (c_int, [c_void_p]),
    "dr_comm_count": (c_int, [c_void_p, POINTER(c_int)]),
    "dr_comm_all_gather": (c_int, [c_void_p, c_char_p, c_size_t, c_char_p]),
    "dr_g1_msm_sharded_dev": (c_int, [c_void_p, c_void_p, c_void_p, c_size_t, c_void_p, c_size_t, c_void_p, POINTER(c_int)]),
})
# the group laws on raw limb images (csrc/wave_curve.hip.h, wave_law_selftest): suite -> (limbs of a coordinate, coordinates of a point)
LAW_SELFTEST_SHAPES = {"ed25519": (9, 4), "bjj": (9, 4), "p256": (9, 3), "secp256k1": (9, 3), "blsg1": (14, 3), "ed448": (16, 3),
                       "curve448": (16, 3), "p521": (19, 3), "p384": (14, 3),
                       "blsg2": (28, 3)}   # E(Fq2), a coordinate c0 then c1: a kernel of its own with the same shape and slots (csrc/kernels_g2_msm.hip.h)
LAW_SELFTEST_SLOTS = 13
_PROTOTYPES.update({f"dr_{suite}_law_selftest": (c_int, [c_void_p, c_char_p, c_char_p, c_size_t, c_void_p]) for suite in LAW_SELFTEST_SHAPES})
# fr29.hip.h and curve.hip.h's law on raw limb images (kernels_bsn.hip.h: k_fr_raw_selftest, k_te_law_selftest)
FR_RAW_IN_WORDS, FR_RAW_OUT_WORDS = 4 * 9, 13 * 9 + 4 * 8 + 1
TE_LAW_REC_WORDS, TE_LAW_SLOTS, TE_LAW_PT_WORDS = 11 * 9, 17, 4 * 9
_PROTOTYPES.update({
    "dr_fr_raw_selftest": (c_int, [c_void_p, c_char_p, c_size_t, c_void_p]),
    "dr_te_law_selftest": (c_int, [c_void_p, c_int, c_char_p, c_char_p, c_size_t, c_void_p]),
})
COMM_ID_BYTES = 128
RINGVRF_AUX_BYTES = 960
PEDERSEN_AUX_BYTES = 288
EXPORTED_SYMBOLS = tuple(_PROTOTYPES)


_buffers = threading.local()


def _thread_buffer(name: str, nbytes: int):
    """A per-thread ctypes byte buffer of at least nbytes, reused across calls (contents are overwritten by the next call)."""
    have = getattr(_buffers, name, None)
    if have is None or len(have) < nbytes:
        have = (ctypes.c_char * max(nbytes, 1))()
        setattr(_buffers, name, have)
    return have


def wipe(buf) -> None:
    """Zero a reused ctypes buffer that held secret material (the auxiliary records carry the blinding factors)."""
    ctypes.memset(buf, 0, len(buf))


def wipe_thread_buffer(name: str) -> None:
    """Zero the calling thread's reused buffer `name` if it exists (a native call that raised may have left secrets in it)."""
    have = getattr(_buffers, name, None)
    if have is not None:
        wipe(have)


def aux_take_blindings(aux_buf, batch: int):
    """The blinding factors of a dr_ringvrf_prove_batch call, moved out of its auxiliary records (zeroed there): returns the
    scratch buffer holding batch * 32 bytes; the caller slices each proof's own 32 bytes out and wipes it."""
    out = _thread_buffer("prove_blind", 32 * batch)
    _check(lib().dr_ringvrf_aux_take_blindings(aux_buf, batch, out))
    return out


def _ragged(items):
    """Concatenate byte strings -> (blob, uint64 offsets[count+1])."""
    off = array.array("Q", itertools.chain((0,), itertools.accumulate(map(len, items))))      # 0.05 ms per 1024 items (0.11 in a loop)
    return b"".join(items), (ctypes.c_uint64 * len(off)).from_buffer(off)


# element formats of dr_ntt_formats_selftest (csrc/kernels_ntt.hip.h)
NTT_FMT_STD8, NTT_FMT_FS9, NTT_FMT_STD8_SCALED, NTT_FMT_FS9_COSETS = 0, 1, 2, 3
CURVE_BANDERSNATCH, CURVE_JUBJUB, CURVE_BANDERSNATCH_SW, CURVE_ED25519, CURVE_P256, CURVE_BABYJUBJUB = 0, 1, 2, 3, 4, 5
CURVE_SECP256K1, CURVE_SECP256K1_NU = 6, 7
CURVE_P256_RO, CURVE_P256_NU, CURVE_ED25519_RO, CURVE_ED25519_NU = 8, 9, 10, 11
CURVE_CURVE25519_RO, CURVE_CURVE25519_NU = 13, 14       # (12 is not assigned)
# BLS12-381 G1 by RFC 9380: 48-byte coordinates, entry points of their own (dr_blsg1_*); every 64-byte entry point refuses these ids
CURVE_BLS12_381_G1, CURVE_BLS12_381_G1_NU = 15, 16
# BLS12-381 G2 by RFC 9380: Fq2 coordinates (96 bytes), entry points of their own (dr_blsg2_*); refused everywhere else
CURVE_BLS12_381_G2, CURVE_BLS12_381_G2_NU = 17, 18
# Ed448 by RFC 9380: 56-byte coordinates AND 56-byte scalars, entry points of their own (dr_ed448_*); refused everywhere else
CURVE_ED448_RO, CURVE_ED448_NU = 19, 20
# Curve448 by RFC 9380: Montgomery u || v over Ed448's field, entry points of their own (dr_curve448_*), the identity 112 bytes of 0xff
CURVE_CURVE448_RO, CURVE_CURVE448_NU = 21, 22
# P-521 by RFC 9380: 68-byte coordinates and scalars (below 2^521), entry points of their own (dr_p521_*), the identity 136 zero bytes
CURVE_P521_RO, CURVE_P521_NU = 23, 24
# P-384 by RFC 9380: 48-byte coordinates and scalars (every 384-bit value), entry points of their own (dr_p384_*), the identity 96 zero bytes
CURVE_P384_RO, CURVE_P384_NU = 25, 26
# bytes of an encoded point, per curve id (the suites with 33-byte encodings and Curve25519's 64-byte u || v; every other curve's are 32)
_POINT_LEN = {CURVE_BANDERSNATCH_SW: 33, CURVE_P256: 33, CURVE_SECP256K1: 33, CURVE_SECP256K1_NU: 33, CURVE_P256_RO: 33, CURVE_P256_NU: 33,
              CURVE_CURVE25519_RO: 64, CURVE_CURVE25519_NU: 64}
# the nonuniform RFC 9380 suites: one field element per message
_NU_CURVES = (CURVE_SECP256K1_NU, CURVE_P256_NU, CURVE_ED25519_NU, CURVE_CURVE25519_NU)


def curve_point_len(curve: int) -> int:
    return _POINT_LEN.get(curve, 32)
# dr_vrf_suite.xof: the transcript hash of a suite
XOF_SHA512, XOF_SHAKE128, XOF_SHA256 = 0, 1, 2
_XOF_OF_HASH = {"sha512": XOF_SHA512, "shake_128": XOF_SHAKE128, "sha256": XOF_SHA256}


def suite_point_len(suite: "VrfSuiteStruct") -> int:
    """bytes of an encoded point of the suite: 33 for the short Weierstrass suites (Bandersnatch_SW, P-256, secp256k1), 32 otherwise"""
    return curve_point_len(suite.curve)


def xof_kind(xof) -> int:
    """dr_vrf_suite.xof of a suite's hash: a hashlib constructor (sha512 -> 0, shake_128 -> 1, sha256 -> 2), the kind itself, or, as
    before, a bool (True: SHAKE128, False: SHA-512)"""
    if callable(xof):
        name = xof().name
        if name not in _XOF_OF_HASH:
            raise ValueError(f"no native transcript for hash {name}")
        return _XOF_OF_HASH[name]
    if isinstance(xof, bool) or xof is None:
        return XOF_SHAKE128 if xof else XOF_SHA512
    if xof not in (XOF_SHA512, XOF_SHAKE128, XOF_SHA256):
        raise ValueError(f"unknown transcript hash kind {xof}")
    return int(xof)


def vrf_suite(suite_id: bytes, xof, generator_xy: bytes, blinding_base_xy: bytes, curve: int = CURVE_BANDERSNATCH) -> VrfSuiteStruct:
    s = VrfSuiteStruct()
    s._keep = bytes(suite_id)
    s.suite_id, s.suite_id_len, s.xof, s.curve = s._keep, len(s._keep), xof_kind(xof), curve
    ctypes.memmove(s.generator_xy, generator_xy, 64)
    ctypes.memmove(s.blinding_base_xy, blinding_base_xy, 64)
    return s


def ring_verifier_key(log2n: int, omega_n: int, seed_xy: bytes, fixed_commitments: bytes, g1_generator: bytes, g2: bytes,
                      fs_prefix: bytes) -> RingVerifierKeyStruct:
    vk = RingVerifierKeyStruct()
    vk.log2n = log2n
    ctypes.memmove(vk.omega_n, int(omega_n).to_bytes(32, "little"), 32)
    ctypes.memmove(vk.seed_xy, seed_xy, 64)
    ctypes.memmove(vk.fixed_commitments, fixed_commitments, 288)
    ctypes.memmove(vk.g1_generator, g1_generator, 96)
    ctypes.memmove(vk.g2, g2, 384)
    vk._keep = bytes(fs_prefix)
    vk.fs_prefix, vk.fs_prefix_len = vk._keep, len(vk._keep)
    return vk


def host_hash(kind: int, data: bytes, out_len: int) -> bytes:
    """kind: 0 SHA-512, 1 SHAKE128, 2 SHAKE256, 4 SHA-256 (the library's own implementations; checked against hashlib in tests)."""
    out = ctypes.create_string_buffer(out_len)
    _check(lib().dr_host_hash(kind, data, len(data), out, out_len))
    return out.raw


def random_expand(seed32: bytes, nbytes: int) -> bytes:
    """nbytes of SHAKE256(seed || LE64(block)) output in 576-byte blocks, hashed on the library's worker threads: turns one
    32-byte secret seed from the OS into the hidden rows of a whole batch of ring proofs."""
    if len(seed32) != 32:
        raise ValueError("seed must be 32 bytes")
    out = ctypes.create_string_buffer(max(1, nbytes))
    _check(lib().dr_host_random_expand(seed32, out, nbytes))
    return out.raw[:nbytes]


def hash_to_field_batch(suite: VrfSuiteStruct, msgs) -> bytes:
    """dr_hash_to_field_batch: two elements (64 bytes) per message; one (32 bytes) for the nonuniform RFC 9380 suites"""
    blob, off = _ragged(msgs)
    out = ctypes.create_string_buffer(max(1, 64 * len(msgs)))
    _check(lib().dr_hash_to_field_batch(byref(suite), blob, off, len(msgs), out))
    return out.raw[: (32 if suite.curve in _NU_CURVES else 64) * len(msgs)]


class _Wide(NamedTuple):
    """One wide suite (csrc/capi_suite.hpp) as its dr_<suite>_* entry points see it: byte widths, selftest record count, the NU variant."""
    elem: int           # a hashed field element
    point: int          # x || y
    scalar: int
    enc: int            # one input of the flag-returning call
    limbs: int          # a raw limb image of the field selftest
    records: int        # results per operand pair of the field selftest
    nu: int             # the variant id with one element per message
    flagged: str        # the flag-returning call: "decode_points" (points and flags back) or "check_points" (flags alone)


_WIDE = {
    "blsg1": _Wide(48, 96, 32, 49, 56, 5, CURVE_BLS12_381_G1_NU, "decode_points"),
    "blsg2": _Wide(96, 192, 96, 192, 112, 5, CURVE_BLS12_381_G2_NU, "check_points"),
    "ed448": _Wide(56, 112, 56, 112, 64, 11, CURVE_ED448_NU, "decode_points"),
    "curve448": _Wide(56, 112, 56, 112, 64, 0, CURVE_CURVE448_NU, "decode_points"),       # (no field selftest: the field is Ed448's)
    "p521": _Wide(68, 136, 68, 67, 76, 11, CURVE_P521_NU, "decode_points"),               # (decodes 67-byte SEC1 strings)
    "p384": _Wide(48, 96, 48, 49, 56, 13, CURVE_P384_NU, "decode_points"),                # (decodes 49-byte SEC1 strings)
}


WIDE_PIP_FROM = 256            # csrc/msm_plan.hpp: the term count from which dr_wide_msm takes the bucket method
NARROW_PIP_FROM = 257          # csrc/msm_plan.hpp: the same for dr_te_msm on the native 256-bit curves and for dr_blsg1_msm
BLSG2_PIP_FROM = 257           # csrc/msm_plan.hpp: the same for dr_blsg2_msm on BLS12-381's E(Fq2)
# the suites dr_wide_msm serves, by the curve id it takes (either variant: RO and NU are one group)
_WIDE_MSM_CURVE = {"p384": CURVE_P384_RO, "p521": CURVE_P521_RO, "ed448": CURVE_ED448_RO, "curve448": CURVE_CURVE448_RO}


def _wide_hash_to_field_batch(suite: str, variant: int, msgs) -> bytes:
    """dr_<suite>_hash_to_field_batch (host only): two elements per message, one for the suite's NU variant"""
    w = _WIDE[suite]
    blob, off = _ragged([bytes(m) for m in msgs])
    out = ctypes.create_string_buffer(max(1, 2 * w.elem * len(msgs)))
    _check(getattr(lib(), f"dr_{suite}_hash_to_field_batch")(variant, blob, off, len(msgs), out))
    return out.raw[: (1 if variant == w.nu else 2) * w.elem * len(msgs)]


blsg1_hash_to_field_batch = functools.partial(_wide_hash_to_field_batch, "blsg1")
blsg2_hash_to_field_batch = functools.partial(_wide_hash_to_field_batch, "blsg2")
ed448_hash_to_field_batch = functools.partial(_wide_hash_to_field_batch, "ed448")
curve448_hash_to_field_batch = functools.partial(_wide_hash_to_field_batch, "curve448")
p521_hash_to_field_batch = functools.partial(_wide_hash_to_field_batch, "p521")
p384_hash_to_field_batch = functools.partial(_wide_hash_to_field_batch, "p384")


def lib() -> ctypes.CDLL:
    """Load libdotring_hip.so (built by __graft_entry__.build() / `make -C dot_ring_amd/csrc`)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `make -C dot_ring_amd/csrc` (hipcc, gfx950). "
                "dot_ring_amd has no CPU fallback."
            )
        cdll = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in _PROTOTYPES.items():
            fn = getattr(cdll, name)
            fn.restype = res
            fn.argtypes = args
        _lib = cdll
    return _lib


def last_error() -> str:
    return (lib().dr_last_error() or b"").decode("utf-8", "replace")


def _check(rc: int) -> None:
    if rc == DR_OK:
        return
    msg = (lib().dr_last_error() or b"").decode("utf-8", "replace")
    if rc in (DR_ERR_INVALID, DR_ERR_NOTSQUARE):
        raise ValueError(msg)
    if rc == DR_ERR_NOMEM:
        raise MemoryError(msg)
    raise DotRingHipError(msg)


def device_count() -> int:
    return int(lib().dr_device_count())


class DeviceBuffer:
    """A block of HBM owned by a Context."""

    def __init__(self, ctx: "Context", nbytes: int):
        self.ctx, self.nbytes = ctx, nbytes
        self.ptr = c_void_p()
        _check(lib().dr_dev_alloc(ctx.handle, nbytes, byref(self.ptr)))

    def upload(self, data: bytes) -> "DeviceBuffer":
        if len(data) > self.nbytes:
            raise ValueError("upload larger than the buffer")
        _check(lib().dr_dev_upload(self.ctx.handle, self.ptr, data, len(data)))
        return self

    def download(self, nbytes: int | None = None) -> bytes:
        nbytes = self.nbytes if nbytes is None else nbytes
        out = ctypes.create_string_buffer(nbytes)
        _check(lib().dr_dev_download(self.ctx.handle, out, self.ptr, nbytes))
        return out.raw

    def free(self) -> None:
        if self.ptr:
            lib().dr_dev_free(self.ctx.handle, self.ptr)
            self.ptr = c_void_p()


class Srs:
    """SRS bases resident in HBM (Montgomery-form affine)."""

    def __init__(self, ctx: "Context", g1_be_xy: bytes | None = None, *, synthetic_seed: bytes | None = None, first: int = 1, count: int = 0,
                 tau: int | None = None):
        self.ctx = ctx
        self.handle = c_void_p()
        if tau is not None:
            self.count = count
            _check(lib().dr_srs_powers(ctx.handle, synthetic_seed, int(tau).to_bytes(32, "little"), count, byref(self.handle)))
            return
        if synthetic_seed is not None:
            self.count = count
            _check(lib().dr_srs_synthetic(ctx.handle, synthetic_seed, first, count, byref(self.handle)))
            return
        if g1_be_xy is None or len(g1_be_xy) % 96:
            raise ValueError("SRS bytes must be a multiple of 96")
        self.count = len(g1_be_xy) // 96
        _check(lib().dr_srs_load(ctx.handle, g1_be_xy, self.count, byref(self.handle)))

    def precompute(self, window_bits: int, multiples: int = 1) -> "Srs":
        """Build (or with 0 drop) the fixed-base window table in HBM.  multiples: blocks of rows of a bit-row table, one per small odd
        multiple of the bases (2, 4, 8, 16, 32; 0 = the library's default count, 8; -1 = the count it recommends for batched proving;
        dr_srs_precompute_multiples); 1 = the plain table."""
        if multiples == 1:
            _check(lib().dr_srs_precompute(self.ctx.handle, self.handle, window_bits))
        else:
            _check(lib().dr_srs_precompute_multiples(self.ctx.handle, self.handle, window_bits, multiples))
        return self

    def table_info(self, n: int = 0, batch: int = 0) -> dict:
        """Shape of the fixed-base table and the tiling `batch` MSMs of n points over it take (dr_srs_table_info): window_bits, rows,
        digit rows per scalar, the per-call tiling (window rows or the non-adjacent form over a bit-row table) with its width, and
        the expected non-zero digits per scalar (= bucket additions per pair)."""
        info = (c_int * 8)()
        _check(lib().dr_srs_table_info_multiples(self.handle, n, batch, info))
        return {"window_bits": info[0], "rows": info[1], "batched_windows": info[2], "tiling_bits": info[3],
                "tiling": ("window rows", "-", "non-adjacent form")[info[4]], "digits_per_scalar": info[5] / 1000.0,
                "odd_buckets": bool(info[4]), "multiples": info[6], "table_multiples": info[7]}

    def download(self, offset: int, count: int) -> bytes:
        out = ctypes.create_string_buffer(max(96 * count, 1))
        _check(lib().dr_srs_download(self.ctx.handle, self.handle, offset, count, out))
        return out.raw[: 96 * count]

    def close(self) -> None:
        if self.handle:
            lib().dr_srs_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class RingProver:
    """Device-resident batched ring prover for one ring (dr_ring_prover_*)."""

    def __init__(self, ctx: "Context", srs: Srs, log2n: int, max_ring: int, omega_n: int, omega_4n: int, nm_points_xy: bytes, seed_xy: bytes,
                 curve: int = CURVE_BANDERSNATCH):
        self.ctx, self.srs = ctx, srs
        self.n = 1 << log2n
        self.handle = c_void_p()
        _check(lib().dr_ring_prover_create_te(ctx.handle, curve, srs.handle, log2n, max_ring, omega_n.to_bytes(32, "little"),
                                              omega_4n.to_bytes(32, "little"), nm_points_xy, seed_xy, byref(self.handle)))

    def close(self) -> None:
        if self.handle:
            lib().dr_ring_prover_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        # provers are cached on Ring objects: when the ring goes, its tables and per-batch state (hundreds of MB of HBM)
        # must go too
        try:
            self.close()
        except Exception:
            pass

    @staticmethod
    def _points(raw: bytes, inf, count: int) -> list:
        return [None if inf[i] else raw[96 * i : 96 * i + 96] for i in range(count)]

    def root(self) -> list:
        out, inf = ctypes.create_string_buffer(3 * 96), (c_int * 3)()
        _check(lib().dr_ring_prover_root(self.handle, out, inf))
        return self._points(out.raw, inf, 3)

    def fixed_coeffs(self) -> bytes:
        out = ctypes.create_string_buffer(3 * self.n * 32)
        _check(lib().dr_ring_prover_fixed_coeffs(self.handle, out))
        return out.raw

    PEEK_COLUMNS, PEEK_QUOTIENT, PEEK_LIN = 0, 1, 2

    def peek(self, what: int, batch: int) -> bytes:
        """Diagnostic read-back of the batch in flight: the four coefficient columns (after witness), q zero-padded to 3N + 1
        coefficients (after quotient) or the linearisation polynomial (after evals); 32-byte LE standard form, proof-major."""
        per = {self.PEEK_COLUMNS: 4 * self.n, self.PEEK_QUOTIENT: 3 * self.n + 1, self.PEEK_LIN: self.n}.get(what, 1)
        out = ctypes.create_string_buffer(max(1, 32 * per * batch))
        _check(lib().dr_ring_prover_peek(self.handle, what, out, 32 * per * batch))
        return out.raw[: 32 * per * batch]

    def witness(self, producer_index: list, blinding: bytes, zk_rows: bytes | None):
        batch = len(producer_index)
        idx = (ctypes.c_uint32 * batch)(*producer_index)
        rel, cms, inf = ctypes.create_string_buffer(64 * batch), ctypes.create_string_buffer(4 * 96 * batch), (c_int * (4 * batch))()
        _check(lib().dr_ring_prove_witness(self.handle, batch, idx, blinding, zk_rows, rel, cms, inf))
        return rel.raw, self._points(cms.raw, inf, 4 * batch)

    def quotient(self, batch: int, alphas: bytes) -> list:
        out, inf = ctypes.create_string_buffer(96 * batch), (c_int * batch)()
        _check(lib().dr_ring_prove_quotient(self.handle, batch, alphas, out, inf))
        return self._points(out.raw, inf, batch)

    def evals(self, batch: int, zetas: bytes) -> bytes:
        out = ctypes.create_string_buffer(8 * 32 * batch)
        _check(lib().dr_ring_prove_evals(self.handle, batch, zetas, out))
        return out.raw

    def openings(self, batch: int, nus: bytes) -> list:
        out, inf = ctypes.create_string_buffer(2 * 96 * batch), (c_int * (2 * batch))()
        _check(lib().dr_ring_prove_openings(self.handle, batch, nus, out, inf))
        return self._points(out.raw, inf, 2 * batch)

    def wipe(self) -> None:
        """Zero the per-batch state and the MSM scratch on the device now (every batch already ends with it)."""
        _check(lib().dr_ring_prover_wipe(self.handle))

    def residue(self) -> int:
        """Non-zero 32-bit words left in the prover's per-batch device state and its contexts' scratch (0 after a wipe)."""
        words = ctypes.c_uint64(0)
        _check(lib().dr_ring_prover_residue(self.handle, byref(words)))
        return words.value

    def ringvrf_prove_batch(self, suite: "VrfSuiteStruct", alphas, ads, salts, secret_scalars: bytes, producer_index: list,
                            fs_prefix: bytes, zk_random48: bytes | None):
        """dr_ringvrf_prove_batch: the whole batch (hashing on the library's worker threads, GPU phases in between).
        Returns (batch * 784 proof bytes, batch * 960 auxiliary bytes)."""
        batch = len(alphas)
        a_blob, a_off = _ragged(alphas)
        d_blob, d_off = _ragged(ads)
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
        idx = (ctypes.c_uint32 * batch)(*producer_index)
        # output buffers are kept per thread and reused: two fresh megabyte-sized buffers plus their `.raw` copies cost ~1 ms per
        # 1024 proofs in page faults.  The caller slices its proofs out (slicing a c_char array yields bytes) before its next call.
        out, aux = _thread_buffer("prove_out", 784 * batch), _thread_buffer("prove_aux", RINGVRF_AUX_BYTES * batch)
        _check(lib().dr_ringvrf_prove_batch(self.handle, byref(suite), batch, a_blob, a_off, d_blob, d_off, s_blob, s_off, secret_scalars, idx,
                                            fs_prefix, len(fs_prefix), zk_random48, out, aux))
        return out, aux


def ringvrf_prove_batch_multi(provers: list, suite: "VrfSuiteStruct", alphas, ads, salts, secret_scalars: bytes, producer_index: list,
                              fs_prefix: bytes, zk_random48: bytes | None):
    """dr_ringvrf_prove_batch_multi: ONE batch over the devices of `provers` (a RingProver of the same ring per device), device g
    proving proofs [g B / G, (g + 1) B / G).  Returns the same (proof bytes, auxiliary bytes) buffers as RingProver.ringvrf_prove_batch."""
    batch = len(alphas)
    a_blob, a_off = _ragged(alphas)
    d_blob, d_off = _ragged(ads)
    s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
    idx = (ctypes.c_uint32 * batch)(*producer_index)
    handles = (c_void_p * len(provers))(*[p.handle for p in provers])
    out, aux = _thread_buffer("prove_out", 784 * batch), _thread_buffer("prove_aux", RINGVRF_AUX_BYTES * batch)
    _check(lib().dr_ringvrf_prove_batch_multi(handles, len(provers), byref(suite), batch, a_blob, a_off, d_blob, d_off, s_blob, s_off,
                                              secret_scalars, idx, fs_prefix, len(fs_prefix), zk_random48, out, aux))
    return out, aux


def ringvrf_verify_batch_multi(contexts: list, suite: "VrfSuiteStruct", vk: "RingVerifierKeyStruct", proofs: bytes, inputs, ads, salts,
                               seed32: bytes) -> bool:
    """dr_ringvrf_verify_batch_multi: ONE batch of 784-byte proofs over the devices of `contexts`, the shards' verdicts AND-ed."""
    batch = len(inputs)
    if len(proofs) != 784 * batch:
        raise ValueError("proofs must be 784 bytes each")
    i_blob, i_off = _ragged(inputs)
    d_blob, d_off = _ragged(ads)
    s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
    handles = (c_void_p * len(contexts))(*[c.handle for c in contexts])
    ok = c_int(0)
    _check(lib().dr_ringvrf_verify_batch_multi(handles, len(contexts), byref(suite), byref(vk), batch, proofs, i_blob, i_off, d_blob, d_off,
                                               s_blob, s_off, seed32, byref(ok)))
    return bool(ok.value)


def ringvrf_verify_each_multi(contexts: list, suite: "VrfSuiteStruct", vk: "RingVerifierKeyStruct", proofs: bytes, inputs, ads, salts,
                              seed32: bytes):
    """dr_ringvrf_verify_each_multi: a verdict per 784-byte proof over the devices of `contexts` -> (list of bool, the four stats words)."""
    batch = len(inputs)
    if len(proofs) != 784 * batch:
        raise ValueError("proofs must be 784 bytes each")
    i_blob, i_off = _ragged(inputs)
    d_blob, d_off = _ragged(ads)
    s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
    handles = (c_void_p * len(contexts))(*[c.handle for c in contexts])
    verdicts, stats = ctypes.create_string_buffer(max(1, batch)), (ctypes.c_uint32 * 4)()
    _check(lib().dr_ringvrf_verify_each_multi(handles, len(contexts), byref(suite), byref(vk), batch, proofs, i_blob, i_off, d_blob, d_off,
                                              s_blob, s_off, seed32, verdicts, stats))
    return [b != 0 for b in verdicts.raw[:batch]], tuple(stats)


class Context:
    """One GPU + one HIP stream.  Not thread-safe; create one per thread / per rank."""

    def __init__(self, device_id: int = 0):
        self.handle = c_void_p()
        _check(lib().dr_ctx_create(device_id, byref(self.handle)))
        self.device_id = device_id

    def close(self) -> None:
        if self.handle:
            lib().dr_ctx_destroy(self.handle)
            self.handle = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self) -> None:
        _check(lib().dr_ctx_sync(self.handle))

    def alloc(self, nbytes: int) -> DeviceBuffer:
        return DeviceBuffer(self, nbytes)

    def scratch_residue(self) -> int:
        """Non-zero 32-bit words in this context's scratch buffers (0 after a batch prover has wiped them)."""
        words = ctypes.c_uint64(0)
        _check(lib().dr_ctx_scratch_residue(self.handle, byref(words)))
        return words.value

    # ---- profiling
    def prof_enable(self, on: bool = True) -> None:
        _check(lib().dr_prof_enable(self.handle, 1 if on else 0))

    def prof_reset(self) -> None:
        _check(lib().dr_prof_reset(self.handle))

    def prof_get(self, kernel: str) -> tuple[float, int]:
        ms, cnt = c_double(0), c_int(0)
        _check(lib().dr_prof_get(self.handle, kernel.encode(), byref(ms), byref(cnt)))
        return ms.value, cnt.value

    def fr_ops_selftest(self, a: bytes, b: bytes):
        """dr_fr_ops_selftest: (n x 12 x 32 result bytes, n square flags) for n pairs of canonical 32-byte elements."""
        n = len(a) // 32
        if len(a) != 32 * n or len(b) != 32 * n:
            raise ValueError("operands are 32 bytes each")
        out, flags = ctypes.create_string_buffer(max(1, 384 * n)), ctypes.create_string_buffer(max(1, n))
        _check(lib().dr_fr_ops_selftest(self.handle, a, b, n, out, flags))
        return out.raw[: 384 * n], flags.raw[:n]

    def _limb_selftest(self, fn, records: int, a_limbs: bytes, b_limbs: bytes, limb_bytes: int = 36, elem: int = 32):
        """(n x records x elem result bytes, n flag bytes) of one native suite's field selftest on n pairs of raw limb images (nine limbs
        and 32-byte results on the 256-bit suites)."""
        n = len(a_limbs) // limb_bytes
        if len(a_limbs) != limb_bytes * n or len(b_limbs) != limb_bytes * n:
            raise ValueError(f"operands are {limb_bytes // 4} int32 limbs each")
        rec = elem * records
        out, flags = ctypes.create_string_buffer(max(1, rec * n)), ctypes.create_string_buffer(max(1, n))
        _check(fn(self.handle, a_limbs, b_limbs, n, out, flags))
        return out.raw[: rec * n], flags.raw[:n]

    def fe25519_ops_selftest(self, a_limbs: bytes, b_limbs: bytes):
        """dr_fe25519_ops_selftest: (n x 11 x 32 result bytes, n flag bytes) for n pairs of raw 9-limb images (9 little-endian int32 each)."""
        return self._limb_selftest(lib().dr_fe25519_ops_selftest, 11, a_limbs, b_limbs)

    def p256_field_ops_selftest(self, a_limbs: bytes, b_limbs: bytes):
        """dr_p256_field_ops_selftest: (n x 12 x 32 result bytes, n flag bytes) for n pairs of raw 9-limb Montgomery images."""
        return self._limb_selftest(lib().dr_p256_field_ops_selftest, 12, a_limbs, b_limbs)

    def bjj_field_ops_selftest(self, a_limbs: bytes, b_limbs: bytes):
        """dr_bjj_field_ops_selftest: (n x 12 x 32 result bytes, n flag bytes) for n pairs of raw 9-limb Montgomery images."""
        return self._limb_selftest(lib().dr_bjj_field_ops_selftest, 12, a_limbs, b_limbs)

    def _decode_points(self, fn, width: int, enc: bytes, check: bool):
        """(x||y bytes, flags) of one native suite's decoder on len(enc)/width encodings."""
        if len(enc) % width:
            raise ValueError(f"compressed points are {width} bytes each")
        count = len(enc) // width
        out, ok = ctypes.create_string_buffer(max(1, 64 * count)), ctypes.create_string_buffer(max(1, count))
        _check(fn(self.handle, 1 if check else 0, enc, count, out, ok))
        return out.raw[: 64 * count], ok.raw[:count]

    def bjj_decode_points(self, enc: bytes, check: bool = True):
        """dr_bjj_decode_points: (x||y bytes, flags) for len(enc)/32 encodings, with or without the prime-order check."""
        return self._decode_points(lib().dr_bjj_decode_points, 32, enc, check)

    def p256_decode_points(self, enc: bytes, check: bool = True):
        """dr_p256_decode_points: (x||y bytes, flags) for len(enc)/33 encodings, with or without the identity check."""
        return self._decode_points(lib().dr_p256_decode_points, 33, enc, check)

    def secp256k1_decode_points(self, enc: bytes, check: bool = True):
        """dr_secp256k1_decode_points: (x||y bytes, flags) for len(enc)/33 SEC1 encodings."""
        return self._decode_points(lib().dr_secp256k1_decode_points, 33, enc, check)

    def secp256k1_field_selftest(self, a_limbs: bytes, b_limbs: bytes):
        """dr_secp256k1_field_selftest: (n x 12 x 32 result bytes, n flag bytes) for n pairs of raw 9-limb images."""
        return self._limb_selftest(lib().dr_secp256k1_field_selftest, 12, a_limbs, b_limbs)

    # ---- the wide suites (include/dotring_hip.h; widths in _WIDE): BLS12-381 G1 (points 96 bytes x || y little-endian, 96 zero bytes the
    # identity), G2 (Fq2 elements c0 || c1; 192 zero bytes the identity), Ed448 (the identity (0, 1) as itself) and Curve448 (u || v, the
    # identity 112 bytes of 0xff in and out) and P-521 (136 zero bytes the identity; scalars below 2^521) and P-384 (96 zero bytes the
    # identity); scalars as they are
    def _wide_map_to_curve(self, suite: str, us: bytes, per_item: int, clear: bool = True):
        """dr_<suite>_map_to_curve: (x||y bytes, flags) for len(us) / (elem per_item) items; clear = False: before the cofactor clearing.
        per_item other than 1 or 2 is the library's to refuse."""
        w = _WIDE[suite]
        if len(us) % w.elem or (per_item in (1, 2) and len(us) % (w.elem * per_item)):
            raise ValueError(f"field elements are {w.elem} bytes each, one or two per item")
        n = len(us) // (w.elem * per_item) if per_item in (1, 2) else len(us) // w.elem
        out, ok = ctypes.create_string_buffer(max(1, w.point * n)), ctypes.create_string_buffer(max(1, n))
        _check(getattr(lib(), f"dr_{suite}_map_to_curve")(self.handle, us, n, per_item, 1 if clear else 0, out, ok))
        return out.raw[: w.point * n], ok.raw[:n]

    def _wide_encode_to_curve_batch(self, suite: str, variant: int, msgs, salts=None) -> bytes:
        """dr_<suite>_encode_to_curve_batch: encode_to_curve(salt_i || msg_i) -> count points x||y."""
        w, count = _WIDE[suite], len(msgs)
        m_blob, m_off = _ragged([bytes(m) for m in msgs])
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged([bytes(x) for x in salts])
        out = ctypes.create_string_buffer(max(w.point * count, 1))
        _check(getattr(lib(), f"dr_{suite}_encode_to_curve_batch")(self.handle, variant, m_blob, m_off, s_blob, s_off, count, out))
        return out.raw[: w.point * count]

    def _wide_scalar_mul_batch(self, suite: str, pts_xy: bytes, scalars: bytes) -> bytes:
        """dr_<suite>_scalar_mul_batch: k_i P_i for n points and n scalars used as they are."""
        w = _WIDE[suite]
        n = len(scalars) // w.scalar
        if len(scalars) != w.scalar * n or len(pts_xy) != w.point * n:
            raise ValueError("Points and scalars must have same length")
        out = ctypes.create_string_buffer(max(1, w.point * n))
        _check(getattr(lib(), f"dr_{suite}_scalar_mul_batch")(self.handle, pts_xy, scalars, n, out))
        return out.raw[: w.point * n]

    def _wide_msm_groups(self, suite: str, pts_xy: bytes, scalars: bytes, m: int) -> bytes:
        """dr_<suite>_msm_groups: the sums of consecutive groups of m (1..64) terms k_j P_j."""
        w = _WIDE[suite]
        n = len(scalars) // w.scalar
        if m < 1 or len(scalars) != w.scalar * n or len(pts_xy) != w.point * n or n % m:
            raise ValueError("Points and scalars must have same length, a multiple of the group size")
        groups = n // m
        out = ctypes.create_string_buffer(max(1, w.point * groups))
        _check(getattr(lib(), f"dr_{suite}_msm_groups")(self.handle, pts_xy, scalars, groups, m, out))
        return out.raw[: w.point * groups]

    def wide_msm(self, suite: str, pts_xy: bytes, scalars: bytes) -> bytes:
        """dr_wide_msm: ONE sum of n terms k_i P_i on "p384", "p521", "ed448" or "curve448", in the forms of that suite's msm_groups; from
        256 terms on by the bucket method (csrc/wave_msm.hip.h).  No terms give the identity."""
        if suite not in _WIDE_MSM_CURVE:
            raise ValueError("wide_msm serves p384, p521, ed448 and curve448")
        w = _WIDE[suite]
        n = len(scalars) // w.scalar
        if len(scalars) != w.scalar * n or len(pts_xy) != w.point * n:
            raise ValueError("Points and scalars must have same length")
        out = ctypes.create_string_buffer(w.point)
        _check(lib().dr_wide_msm(self.handle, _WIDE_MSM_CURVE[suite], pts_xy, scalars, n, out))
        return out.raw[: w.point]

    def blsg1_msm(self, pts_xy: bytes, scalars: bytes) -> bytes:
        """dr_blsg1_msm: ONE sum of n terms k_i P_i on BLS12-381's E(Fq), 96-byte points and 32-byte scalars used as they are; from
        NARROW_PIP_FROM terms on by the bucket method (csrc/wave_msm.hip.h).  No terms give the identity."""
        n = len(scalars) // 32
        if len(scalars) != 32 * n or len(pts_xy) != 96 * n:
            raise ValueError("Points and scalars must have same length")
        out = ctypes.create_string_buffer(96)
        _check(lib().dr_blsg1_msm(self.handle, CURVE_BLS12_381_G1, pts_xy, scalars, n, out))
        return out.raw[:96]

    def blsg2_msm(self, pts_xy: bytes, scalars: bytes, curve: int = CURVE_BLS12_381_G2) -> bytes:
        """dr_blsg2_msm: ONE sum of n terms k_i P_i on BLS12-381's E(Fq2), 192-byte points and 32-byte scalars used as they are; from
        BLSG2_PIP_FROM terms on by the bucket method (csrc/wave_msm.hip.h over csrc/kernels_g2_msm.hip.h).  No terms give the identity."""
        n = len(scalars) // 32
        if len(scalars) != 32 * n or len(pts_xy) != 192 * n:
            raise ValueError("Points and scalars must have same length")
        out = ctypes.create_string_buffer(192)
        _check(lib().dr_blsg2_msm(self.handle, curve, pts_xy, scalars, n, out))
        return out.raw[:192]

    def _wide_flagged(self, suite: str, enc: bytes, check: bool = True):
        """dr_<suite>_decode_points: (x||y bytes, flags) for G1's 49-byte SEC1 encodings (check: also r P = O) and Ed448's 112-byte points
        (coordinates below p and on the curve; check: also not the identity and n P = O).  dr_blsg2_check_points: the flags alone, one per
        192-byte point: on the curve, and with `check` also r P = O."""
        w = _WIDE[suite]
        if len(enc) % w.enc:
            raise ValueError(f"points are {w.enc} bytes each")
        n = len(enc) // w.enc
        ok = ctypes.create_string_buffer(max(1, n))
        fn = getattr(lib(), f"dr_{suite}_{w.flagged}")
        if w.flagged == "check_points":
            _check(fn(self.handle, 1 if check else 0, enc, n, ok))
            return ok.raw[:n]
        out = ctypes.create_string_buffer(max(1, w.point * n))
        _check(fn(self.handle, 1 if check else 0, enc, n, out, ok))
        return out.raw[: w.point * n], ok.raw[:n]

    def _wide_field_selftest(self, suite: str, a_limbs: bytes, b_limbs: bytes):
        """dr_<suite>_field_selftest: (n x records x elem result bytes, n flag bytes) for n pairs of raw limb images (little-endian int32:
        14 limbs for G1, 2 x 14 for G2, 16 for Ed448, 19 for P-521, 14 for P-384)."""
        w = _WIDE[suite]
        return self._limb_selftest(getattr(lib(), f"dr_{suite}_field_selftest"), w.records, a_limbs, b_limbs, w.limbs, w.elem)

    blsg1_map_to_curve = functools.partialmethod(_wide_map_to_curve, "blsg1")
    blsg1_encode_to_curve_batch = functools.partialmethod(_wide_encode_to_curve_batch, "blsg1")
    blsg1_scalar_mul_batch = functools.partialmethod(_wide_scalar_mul_batch, "blsg1")
    blsg1_msm_groups = functools.partialmethod(_wide_msm_groups, "blsg1")
    blsg1_decode_points = functools.partialmethod(_wide_flagged, "blsg1")
    blsg1_field_selftest = functools.partialmethod(_wide_field_selftest, "blsg1")
    blsg2_map_to_curve = functools.partialmethod(_wide_map_to_curve, "blsg2")
    blsg2_encode_to_curve_batch = functools.partialmethod(_wide_encode_to_curve_batch, "blsg2")
    blsg2_scalar_mul_batch = functools.partialmethod(_wide_scalar_mul_batch, "blsg2")
    blsg2_msm_groups = functools.partialmethod(_wide_msm_groups, "blsg2")
    blsg2_field_selftest = functools.partialmethod(_wide_field_selftest, "blsg2")
    ed448_map_to_curve = functools.partialmethod(_wide_map_to_curve, "ed448")
    ed448_encode_to_curve_batch = functools.partialmethod(_wide_encode_to_curve_batch, "ed448")
    ed448_scalar_mul_batch = functools.partialmethod(_wide_scalar_mul_batch, "ed448")
    ed448_msm_groups = functools.partialmethod(_wide_msm_groups, "ed448")
    ed448_decode_points = functools.partialmethod(_wide_flagged, "ed448")
    ed448_field_selftest = functools.partialmethod(_wide_field_selftest, "ed448")
    curve448_map_to_curve = functools.partialmethod(_wide_map_to_curve, "curve448")
    curve448_encode_to_curve_batch = functools.partialmethod(_wide_encode_to_curve_batch, "curve448")
    curve448_scalar_mul_batch = functools.partialmethod(_wide_scalar_mul_batch, "curve448")
    curve448_msm_groups = functools.partialmethod(_wide_msm_groups, "curve448")
    curve448_decode_points = functools.partialmethod(_wide_flagged, "curve448")
    p521_map_to_curve = functools.partialmethod(_wide_map_to_curve, "p521")
    p521_encode_to_curve_batch = functools.partialmethod(_wide_encode_to_curve_batch, "p521")
    p521_scalar_mul_batch = functools.partialmethod(_wide_scalar_mul_batch, "p521")
    p521_msm_groups = functools.partialmethod(_wide_msm_groups, "p521")
    p521_decode_points = functools.partialmethod(_wide_flagged, "p521")
    p521_field_selftest = functools.partialmethod(_wide_field_selftest, "p521")
    p384_map_to_curve = functools.partialmethod(_wide_map_to_curve, "p384")
    p384_encode_to_curve_batch = functools.partialmethod(_wide_encode_to_curve_batch, "p384")
    p384_scalar_mul_batch = functools.partialmethod(_wide_scalar_mul_batch, "p384")
    p384_msm_groups = functools.partialmethod(_wide_msm_groups, "p384")
    p384_decode_points = functools.partialmethod(_wide_flagged, "p384")
    p384_field_selftest = functools.partialmethod(_wide_field_selftest, "p384")

    def _law_selftest(self, suite: str, points: bytes, controls: bytes) -> bytes:
        """dr_<suite>_law_selftest: n x 13 points of raw limbs (little-endian int32) for n records of P then Q in the same form and n
        little-endian control words (include/dotring_hip.h lists the slots)."""
        limbs, coords = LAW_SELFTEST_SHAPES[suite]
        rec = 2 * coords * limbs * 4
        n = len(controls) // 4
        if len(controls) != 4 * n or len(points) != rec * n:
            raise ValueError(f"{suite}: a record is {rec} bytes of limbs and one 4-byte control word")
        out = ctypes.create_string_buffer(max(1, n * LAW_SELFTEST_SLOTS * coords * limbs * 4))
        _check(getattr(lib(), f"dr_{suite}_law_selftest")(self.handle, points, controls, n, out))
        return out.raw[: n * LAW_SELFTEST_SLOTS * coords * limbs * 4]

    ed25519_law_selftest = functools.partialmethod(_law_selftest, "ed25519")
    bjj_law_selftest = functools.partialmethod(_law_selftest, "bjj")
    p256_law_selftest = functools.partialmethod(_law_selftest, "p256")
    secp256k1_law_selftest = functools.partialmethod(_law_selftest, "secp256k1")
    blsg1_law_selftest = functools.partialmethod(_law_selftest, "blsg1")
    ed448_law_selftest = functools.partialmethod(_law_selftest, "ed448")
    curve448_law_selftest = functools.partialmethod(_law_selftest, "curve448")
    p521_law_selftest = functools.partialmethod(_law_selftest, "p521")
    p384_law_selftest = functools.partialmethod(_law_selftest, "p384")
    blsg2_law_selftest = functools.partialmethod(_law_selftest, "blsg2")

    def fr_raw_selftest(self, images: bytes) -> bytes:
        """dr_fr_raw_selftest: n x 150 little-endian words for n records of four raw images of nine int32 limbs (include/dotring_hip.h
        lists the results)."""
        n = len(images) // (4 * FR_RAW_IN_WORDS)
        if len(images) != 4 * FR_RAW_IN_WORDS * n:
            raise ValueError(f"a record is {4 * FR_RAW_IN_WORDS} bytes of limbs")
        out = ctypes.create_string_buffer(max(1, n * 4 * FR_RAW_OUT_WORDS))
        _check(lib().dr_fr_raw_selftest(self.handle, images, n, out))
        return out.raw[: n * 4 * FR_RAW_OUT_WORDS]

    def te_law_selftest(self, curve: int, records: bytes, controls: bytes) -> bytes:
        """dr_te_law_selftest: n x 17 points of raw limbs for n records of P, Q and a table row (little-endian int32) and n little-endian
        control words, on Bandersnatch (0) or JubJub (1) (include/dotring_hip.h lists the slots)."""
        n = len(controls) // 4
        if len(controls) != 4 * n or len(records) != 4 * TE_LAW_REC_WORDS * n:
            raise ValueError(f"a record is {4 * TE_LAW_REC_WORDS} bytes of limbs and one 4-byte control word")
        out = ctypes.create_string_buffer(max(1, n * TE_LAW_SLOTS * TE_LAW_PT_WORDS * 4))
        _check(lib().dr_te_law_selftest(self.handle, curve, records, controls, n, out))
        return out.raw[: n * TE_LAW_SLOTS * TE_LAW_PT_WORDS * 4]

    def blsg2_check_points(self, pts_xy: bytes, subgroup: bool = True) -> bytes:
        """dr_blsg2_check_points: one flag byte per 192-byte point: on the curve, and with `subgroup` also r P = O."""
        return self._wide_flagged("blsg2", pts_xy, subgroup)

    def _map_to_curve(self, fn, us: bytes, per_item: int):
        if per_item not in (1, 2) or len(us) % (32 * per_item):
            raise ValueError("field elements are 32 bytes each, one or two per item")
        n = len(us) // (32 * per_item)
        out, ok = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n))
        _check(fn(self.handle, us, n, per_item, out, ok))
        return out.raw[: 64 * n], ok.raw[:n]

    def secp256k1_map_to_curve(self, us: bytes, per_item: int):
        """dr_secp256k1_map_to_curve: (x||y bytes, flags) for len(us) / (32 per_item) items of per_item field elements each."""
        return self._map_to_curve(lib().dr_secp256k1_map_to_curve, us, per_item)

    def p256_map_to_curve(self, us: bytes, per_item: int):
        """dr_p256_map_to_curve: as secp256k1_map_to_curve, onto P-256."""
        return self._map_to_curve(lib().dr_p256_map_to_curve, us, per_item)

    def ed25519_map_to_curve(self, us: bytes, per_item: int):
        """dr_ed25519_map_to_curve: as secp256k1_map_to_curve, onto Ed25519's prime-order subgroup (flags 0: no image)."""
        return self._map_to_curve(lib().dr_ed25519_map_to_curve, us, per_item)

    # ---- Curve25519: Montgomery points u || v with an identity flag byte per point (include/dotring_hip.h)
    def curve25519_scalar_mul_batch(self, pts_uv: bytes, id_in: bytes, scalars: bytes):
        """dr_curve25519_scalar_mul_batch: (u||v bytes, identity flags) of k_i P_i; id_in: one flag byte per point (1: the identity)."""
        n = len(scalars) // 32
        if len(scalars) != 32 * n or len(pts_uv) != 64 * n or len(id_in) != n:
            raise ValueError("Points, flags and scalars must have same length")
        out, flags = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n))
        _check(lib().dr_curve25519_scalar_mul_batch(self.handle, pts_uv, id_in, scalars, n, out, flags))
        return out.raw[: 64 * n], flags.raw[:n]

    def curve25519_msm_groups(self, pts_uv: bytes, id_in: bytes, scalars: bytes, m: int):
        """dr_curve25519_msm_groups: (u||v bytes, identity flags) of the sums of consecutive groups of m terms."""
        n = len(scalars) // 32
        if m <= 0 or n % m or len(scalars) != 32 * n or len(pts_uv) != 64 * n or len(id_in) != n:
            raise ValueError("Points, flags and scalars must have same length (a multiple of the group size)")
        groups = n // m
        out, flags = ctypes.create_string_buffer(max(1, 64 * groups)), ctypes.create_string_buffer(max(1, groups))
        _check(lib().dr_curve25519_msm_groups(self.handle, pts_uv, id_in, scalars, groups, m, out, flags))
        return out.raw[: 64 * groups], flags.raw[:groups]

    def curve25519_decode_points(self, enc: bytes, check: bool = True):
        """dr_curve25519_decode_points: (u||v bytes, flags) for len(enc)/64 encodings, with or without the prime-order check."""
        return self._decode_points(lib().dr_curve25519_decode_points, 64, enc, check)

    def curve25519_map_to_curve(self, us: bytes, per_item: int, clear_cofactor: bool = True):
        """dr_curve25519_map_to_curve: (u||v bytes, identity flags) for len(us) / (32 per_item) items; every element has an image."""
        if per_item not in (1, 2) or len(us) % (32 * per_item):
            raise ValueError("field elements are 32 bytes each, one or two per item")
        n = len(us) // (32 * per_item)
        out, flags = ctypes.create_string_buffer(max(1, 64 * n)), ctypes.create_string_buffer(max(1, n))
        _check(lib().dr_curve25519_map_to_curve(self.handle, us, n, per_item, 1 if clear_cofactor else 0, out, flags))
        return out.raw[: 64 * n], flags.raw[:n]

    def ed25519_decode_points(self, enc: bytes, check: bool = True):
        """dr_ed25519_decode_points: (x||y bytes, flags) for len(enc)/32 encodings, with or without the prime-order check."""
        return self._decode_points(lib().dr_ed25519_decode_points, 32, enc, check)

    def fq_ops_selftest(self, records: bytes) -> bytes:
        """dr_fq_ops_selftest: n records of 64 little-endian int32 (op, four 14-limb operands) -> n records of 16 int32."""
        n = len(records) // 256
        if len(records) != 256 * n:
            raise ValueError("records are 64 words each")
        out = ctypes.create_string_buffer(max(1, 64 * n))
        _check(lib().dr_fq_ops_selftest(self.handle, records, n, out))
        return out.raw[: 64 * n]

    def g1_ops_selftest(self, records: bytes) -> bytes:
        """dr_g1_ops_selftest: n records of 192 words (XYZZ images P, Q, affine A) -> n records of 32 x 60 words."""
        n = len(records) // 768
        if len(records) != 768 * n:
            raise ValueError("records are 192 words each")
        out = ctypes.create_string_buffer(max(1, 7680 * n))
        _check(lib().dr_g1_ops_selftest(self.handle, records, n, out))
        return out.raw[: 7680 * n]

    # ---- seam A
    # (curve = CURVE_BANDERSNATCH / CURVE_JUBJUB; the default goes through the dr_bsn_* names of the original seam)
    def bsn_scalar_mul_batch(self, pts_xy: bytes, scalars: bytes, curve: int = CURVE_BANDERSNATCH) -> bytes:
        n = len(scalars) // 32
        if len(scalars) != 32 * n or len(pts_xy) != 64 * n:
            raise ValueError("Points and scalars must have same length")
        out = ctypes.create_string_buffer(max(64 * n, 1))
        if curve == CURVE_BANDERSNATCH:
            _check(lib().dr_bsn_scalar_mul_batch(self.handle, pts_xy, scalars, n, out))
        else:
            _check(lib().dr_te_scalar_mul_batch(self.handle, curve, pts_xy, scalars, n, out))
        return out.raw[: 64 * n]

    def bsn_scalar_mul_batch_dev(self, d_pts: DeviceBuffer, d_scalars: DeviceBuffer, n: int, d_out: DeviceBuffer) -> None:
        _check(lib().dr_bsn_scalar_mul_batch_dev(self.handle, d_pts.ptr, d_scalars.ptr, n, d_out.ptr))

    def bsn_msm(self, pts_xy: bytes, scalars: bytes, curve: int = CURVE_BANDERSNATCH) -> bytes:
        n = len(scalars) // 32
        if len(scalars) != 32 * n or len(pts_xy) != 64 * n:
            raise ValueError("Points and scalars must have same length")
        out = ctypes.create_string_buffer(64)
        if curve == CURVE_BANDERSNATCH:
            _check(lib().dr_bsn_msm(self.handle, pts_xy, scalars, n, out))
        else:
            _check(lib().dr_te_msm(self.handle, curve, pts_xy, scalars, n, out))
        return out.raw

    def bsn_msm_groups(self, pts_xy: bytes, scalars: bytes, m: int, curve: int = CURVE_BANDERSNATCH) -> bytes:
        n = len(scalars) // 32
        if m <= 0 or n % m or len(scalars) != 32 * n or len(pts_xy) != 64 * n:
            raise ValueError("Points and scalars must have same length (a multiple of the group size)")
        groups = n // m
        out = ctypes.create_string_buffer(max(64 * groups, 1))
        if curve == CURVE_BANDERSNATCH:
            _check(lib().dr_bsn_msm_groups(self.handle, pts_xy, scalars, groups, m, out))
        else:
            _check(lib().dr_te_msm_groups(self.handle, curve, pts_xy, scalars, groups, m, out))
        return out.raw[: 64 * groups]

    def te_fixed_base_msm_groups(self, bases_xy: bytes, scalars: bytes, curve: int = CURVE_BANDERSNATCH) -> bytes:
        """out[g] = sum_j scalars[g*m+j] * bases[j] over m = len(bases_xy) / 64 constant bases (fixed-base window tables)."""
        m = len(bases_xy) // 64
        if m == 0 or len(bases_xy) != 64 * m or len(scalars) % (32 * m):
            raise ValueError("Points and scalars must have same length (a multiple of the number of bases)")
        groups = len(scalars) // (32 * m)
        out = ctypes.create_string_buffer(max(64 * groups, 1))
        _check(lib().dr_te_fixed_base_msm_groups(self.handle, curve, bases_xy, m, scalars, groups, out))
        return out.raw[: 64 * groups]

    def encode_to_curve_batch(self, suite: "VrfSuiteStruct", msgs, salts=None) -> bytes:
        """dr_encode_to_curve_batch: encode_to_curve(salt_i || msg_i) by the suite's own method -> count * 64 bytes x||y."""
        count = len(msgs)
        m_blob, m_off = _ragged([bytes(m) for m in msgs])
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged([bytes(x) for x in salts])
        out = ctypes.create_string_buffer(max(64 * count, 1))
        _check(lib().dr_encode_to_curve_batch(self.handle, byref(suite), m_blob, m_off, s_blob, s_off, count, out))
        return out.raw[: 64 * count]

    def bsn_encode_to_curve_batch(self, u_pairs: bytes) -> bytes:
        n = len(u_pairs) // 64
        if len(u_pairs) != 64 * n:
            raise ValueError("u_pairs must be n * 64 bytes")
        out = ctypes.create_string_buffer(max(64 * n, 1))
        _check(lib().dr_bsn_encode_to_curve_batch(self.handle, u_pairs, n, out))
        return out.raw[: 64 * n]

    # ---- seam B
    def srs_load(self, g1_be_xy: bytes) -> Srs:
        return Srs(self, g1_be_xy)

    def srs_synthetic(self, seed_be_xy: bytes, count: int, first: int = 1) -> Srs:
        """bases[i] = (first+i) * seed, generated on the GPU."""
        return Srs(self, synthetic_seed=seed_be_xy, first=first, count=count)

    def ringvrf_verify_batch(self, suite: "VrfSuiteStruct", vk: "RingVerifierKeyStruct", proofs: bytes, inputs, ads, salts, seed32: bytes) -> bool:
        """dr_ringvrf_verify_batch over 784-byte encoded proofs (<= 4096 per call)."""
        batch = len(inputs)
        if len(proofs) != 784 * batch:
            raise ValueError("proofs must be 784 bytes each")
        i_blob, i_off = _ragged(inputs)
        d_blob, d_off = _ragged(ads)
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
        ok = c_int(0)
        _check(lib().dr_ringvrf_verify_batch(self.handle, byref(suite), byref(vk), batch, proofs, i_blob, i_off, d_blob, d_off, s_blob, s_off,
                                             seed32, byref(ok)))
        return bool(ok.value)

    def ringvrf_verify_each(self, suite: "VrfSuiteStruct", vk: "RingVerifierKeyStruct", proofs: bytes, inputs, ads, salts, seed32: bytes):
        """dr_ringvrf_verify_each over 784-byte encoded proofs (<= 4096 per call) -> (list of bool, (pairing equations evaluated,
        proofs excluded before the fold, tree depth, 0))."""
        batch = len(inputs)
        if len(proofs) != 784 * batch:
            raise ValueError("proofs must be 784 bytes each")
        i_blob, i_off = _ragged(inputs)
        d_blob, d_off = _ragged(ads)
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
        verdicts, stats = ctypes.create_string_buffer(max(1, batch)), (ctypes.c_uint32 * 4)()
        _check(lib().dr_ringvrf_verify_each(self.handle, byref(suite), byref(vk), batch, proofs, i_blob, i_off, d_blob, d_off, s_blob, s_off,
                                            seed32, verdicts, stats))
        return [b != 0 for b in verdicts.raw[:batch]], tuple(stats)

    def g1_claim_tree_selftest(self, pts_le_xy: bytes, scalars: bytes, groups: int, m: int):
        """dr_g1_claim_tree_selftest: `groups` groups of m terms (96-byte affine LE points, 32-byte LE scalars) -> (nodes, flags): the
        2 * Bp - 1 nodes of the sum tree in heap order as 96-byte affine LE records, and one byte per node, 1 for the identity."""
        if len(pts_le_xy) != 96 * groups * m or len(scalars) != 32 * groups * m:
            raise ValueError("groups * m points of 96 bytes and scalars of 32 bytes")
        padded = 1
        while padded < groups:
            padded *= 2
        nodes = 2 * padded - 1
        out, inf = ctypes.create_string_buffer(96 * nodes), ctypes.create_string_buffer(nodes)
        _check(lib().dr_g1_claim_tree_selftest(self.handle, pts_le_xy, scalars, groups, m, out, inf))
        return out.raw[: 96 * nodes], inf.raw[:nodes]

    def g1_decompress_batch(self, enc: bytes):
        """KZG.decompress_g1 for len(enc)/48 encodings on the GPU -> (list of 96-byte records or None for infinity, flags)."""
        if len(enc) % 48:
            raise ValueError("compressed G1 points are 48 bytes each")
        count = len(enc) // 48
        out, ok = ctypes.create_string_buffer(max(1, 96 * count)), ctypes.create_string_buffer(max(1, count))
        _check(lib().dr_g1_decompress_batch(self.handle, enc, count, out, ok))
        raw = out.raw
        zero = bytes(96)
        pts = [None if raw[96 * i : 96 * i + 96] == zero else raw[96 * i : 96 * i + 96] for i in range(count)]
        return pts, ok.raw[:count]

    def bsn_decode_points(self, enc: bytes, curve: int = CURVE_BANDERSNATCH):
        """dec_point for len(enc)/32 compressed points on the GPU (33 bytes each, SW affine out, for CURVE_BANDERSNATCH_SW)
        -> (affine x||y bytes, validity flags)."""
        width = curve_point_len(curve)
        if len(enc) % width:
            raise ValueError(f"compressed points are {width} bytes each")
        count = len(enc) // width
        out, ok = ctypes.create_string_buffer(max(1, 64 * count)), ctypes.create_string_buffer(max(1, count))
        if curve == CURVE_BANDERSNATCH:
            _check(lib().dr_bsn_decode_points(self.handle, enc, count, out, ok))
        else:
            _check(lib().dr_te_decode_points(self.handle, curve, enc, count, out, ok))
        return out.raw[: 64 * count], ok.raw[:count]

    def pedersen_prove_batch(self, suite: "VrfSuiteStruct", alphas, ads, salts, secret_scalars: bytes):
        """dr_pedersen_prove_batch -> (batch * (4 points + 64) proof bytes: 192 / 196 per suite, batch * 288 auxiliary bytes)."""
        batch, plen = len(alphas), 4 * suite_point_len(suite) + 64
        a_blob, a_off = _ragged(alphas)
        d_blob, d_off = _ragged(ads)
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
        out, aux = ctypes.create_string_buffer(max(1, plen * batch)), ctypes.create_string_buffer(max(1, PEDERSEN_AUX_BYTES * batch))
        _check(lib().dr_pedersen_prove_batch(self.handle, byref(suite), batch, a_blob, a_off, d_blob, d_off, s_blob, s_off, secret_scalars, out, aux))
        return out.raw[: plen * batch], aux.raw[: PEDERSEN_AUX_BYTES * batch]

    def ietf_prove_batch(self, suite: "VrfSuiteStruct", thin: bool, alphas, ads, salts, secret_scalars: bytes):
        """dr_ietf_prove_batch -> (batch * (96 if thin else 80) proof bytes — 98 / 81 for the SW suite —, batch * 128 bytes: O and R affine)."""
        pl = suite_point_len(suite)
        batch, plen = len(alphas), 2 * pl + 32 if thin else pl + 48
        a_blob, a_off = _ragged(alphas)
        d_blob, d_off = _ragged(ads)
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
        out, aux = ctypes.create_string_buffer(max(1, plen * batch)), ctypes.create_string_buffer(max(1, 128 * batch))
        _check(lib().dr_ietf_prove_batch(self.handle, byref(suite), 1 if thin else 0, batch, a_blob, a_off, d_blob, d_off, s_blob, s_off,
                                         secret_scalars, out, aux))
        return out.raw[: plen * batch], aux.raw[: 128 * batch]

    def ietf_verify_batch(self, suite: "VrfSuiteStruct", thin: bool, proofs: bytes, public_keys: bytes, inputs, ads, salts) -> bytes:
        """dr_ietf_verify_batch over encoded Tiny (80-byte) / Thin (96-byte) proofs: one verdict byte per proof — 1 verifies, 0 does
        not, 2 invalid public key, 3 malformed proof."""
        batch, plen = len(inputs), 96 if thin else 80
        if len(proofs) != plen * batch or len(public_keys) != 32 * batch:
            raise ValueError(f"proofs must be {plen} bytes and public keys 32 bytes each")
        i_blob, i_off = _ragged(inputs)
        d_blob, d_off = _ragged(ads)
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
        verdict = ctypes.create_string_buffer(max(1, batch))
        _check(lib().dr_ietf_verify_batch(self.handle, byref(suite), 1 if thin else 0, batch, proofs, public_keys, i_blob, i_off, d_blob, d_off,
                                          s_blob, s_off, verdict))
        return verdict.raw[:batch]

    def pedersen_verify_batch(self, suite: "VrfSuiteStruct", proofs: bytes, inputs, ads, salts) -> bool:
        batch, plen = len(inputs), 4 * suite_point_len(suite) + 64
        if len(proofs) != plen * batch:
            raise ValueError(f"proofs must be {plen} bytes each")
        i_blob, i_off = _ragged(inputs)
        d_blob, d_off = _ragged(ads)
        s_blob, s_off = (None, None) if not salts or not any(salts) else _ragged(salts)
        ok = c_int(0)
        _check(lib().dr_pedersen_verify_batch(self.handle, byref(suite), batch, proofs, i_blob, i_off, d_blob, d_off, s_blob, s_off, byref(ok)))
        return bool(ok.value)

    def srs_powers(self, base_be_xy: bytes, tau: int, count: int) -> Srs:
        """bases[i] = tau^i * base (known-tau SRS for tests/benchmarks beyond the shipped file), generated on the GPU."""
        return Srs(self, synthetic_seed=base_be_xy, tau=tau, count=count)

    def g1_msm(self, srs: Srs, scalars: bytes, offset: int = 0) -> bytes | None:
        """Affine BE x||y (96 bytes) or None for the point at infinity."""
        n = len(scalars) // 32
        if len(scalars) != 32 * n:
            raise ValueError("scalars must be a multiple of 32 bytes")
        out, inf = ctypes.create_string_buffer(96), c_int(0)
        _check(lib().dr_g1_msm(self.handle, srs.handle, offset, scalars, n, out, byref(inf)))
        return None if inf.value else out.raw

    def g1_msm_dev(self, srs: Srs, d_scalars: DeviceBuffer, n: int, offset: int = 0) -> bytes | None:
        out, inf = ctypes.create_string_buffer(96), c_int(0)
        _check(lib().dr_g1_msm_dev(self.handle, srs.handle, offset, d_scalars.ptr, n, out, byref(inf)))
        return None if inf.value else out.raw

    def g1_msm_batch(self, srs: Srs, scalars: bytes, n: int) -> list[bytes | None]:
        if n <= 0 or len(scalars) % (32 * n):
            raise ValueError("scalars must be batch * n * 32 bytes")
        batch = len(scalars) // (32 * n)
        out, inf = ctypes.create_string_buffer(96 * batch), (c_int * batch)()
        _check(lib().dr_g1_msm_batch(self.handle, srs.handle, scalars, n, batch, out, inf))
        return [None if inf[b] else out.raw[96 * b : 96 * b + 96] for b in range(batch)]

    def g1_msm_batch_dev(self, srs: Srs, d_scalars: DeviceBuffer, n: int, batch: int) -> list[bytes | None]:
        out, inf = ctypes.create_string_buffer(96 * batch), (c_int * batch)()
        _check(lib().dr_g1_msm_batch_dev(self.handle, srs.handle, d_scalars.ptr, n, batch, out, inf))
        return [None if inf[b] else out.raw[96 * b : 96 * b + 96] for b in range(batch)]

    def g1_msm_points(self, pts_be_xy: bytes, scalars: bytes) -> bytes | None:
        n = len(scalars) // 32
        if len(scalars) != 32 * n or len(pts_be_xy) != 96 * n:
            raise ValueError("Points and scalars must have same length")
        out, inf = ctypes.create_string_buffer(96), c_int(0)
        _check(lib().dr_g1_msm_points(self.handle, pts_be_xy, scalars, n, out, byref(inf)))
        return None if inf.value else out.raw

    # ---- seam C
    def ntt(self, data: bytes, log2n: int, omega: int, scale: int | None = None) -> bytes:
        n = 1 << log2n
        if len(data) % (32 * n):
            raise ValueError(f"coefficient length does not match native NTT plan size {n}")
        batch = len(data) // (32 * n)
        buf = ctypes.create_string_buffer(data, len(data))
        sc = scale.to_bytes(32, "little") if scale is not None else None
        _check(lib().dr_ntt(self.handle, buf, log2n, batch, omega.to_bytes(32, "little"), sc))
        return buf.raw

    def ntt_dev(self, d_data: DeviceBuffer, log2n: int, batch: int, omega: int, scale: int | None = None) -> None:
        sc = scale.to_bytes(32, "little") if scale is not None else None
        _check(lib().dr_ntt_dev(self.handle, d_data.ptr, log2n, batch, omega.to_bytes(32, "little"), sc))

    def ntt_formats_selftest(self, src: bytes, log2n: int, batch: int, omega: int, scale: int | None = None, fmt_in: int = NTT_FMT_STD8,
                             fmt_out: int = NTT_FMT_STD8, pad: int = 0, src_div: int = 1, in_scale: bytes | None = None,
                             special: bytes | None = None) -> bytes:
        """dr_ntt_formats_selftest: `batch` transforms of raw records in the ring prover's element formats (NTT_FMT_*; words are
        little-endian 32-bit) -> batch * 2^log2n raw records of fmt_out (8 words STD8, 9 limbs FS9)."""
        if len(src) % 4 or (in_scale is not None and len(in_scale) % 4) or (special is not None and len(special) % 4):
            raise ValueError("records are whole 32-bit words")
        sc = scale.to_bytes(32, "little") if scale is not None else None
        out = ctypes.create_string_buffer(max(1, (batch << log2n) * (36 if fmt_out == NTT_FMT_FS9 else 32)))
        _check(lib().dr_ntt_formats_selftest(self.handle, src, len(src) // 4, in_scale, len(in_scale) // 4 if in_scale is not None else 0,
                                             special, len(special) // 4 if special is not None else 0, log2n, batch,
                                             omega.to_bytes(32, "little"), sc, fmt_in, fmt_out, pad, src_div, out))
        return out.raw[: (batch << log2n) * (36 if fmt_out == NTT_FMT_FS9 else 32)]


# ---- host-only helpers (no GPU needed)
def fr_sqrt(v: int) -> int:
    out = ctypes.create_string_buffer(32)
    _check(lib().dr_fr_sqrt(int(v).to_bytes(32, "little"), out))
    return int.from_bytes(out.raw, "little")


def g1_sum(points: list) -> bytes | None:
    """Host-side sum of a few affine points (96-byte BE records or None)."""
    raw = b"".join(bytes(96) if p is None else p for p in points)
    out, inf = ctypes.create_string_buffer(96), c_int(0)
    _check(lib().dr_g1_sum(raw, len(points), out, byref(inf)))
    return None if inf.value else out.raw


def g2_mul(g2_be: bytes, scalar: int) -> bytes:
    """scalar * Q for a 192-byte zcash-layout G2 point (host; setup of known-tau test SRS only)."""
    out = ctypes.create_string_buffer(192)
    _check(lib().dr_g2_mul(g2_be, int(scalar).to_bytes(32, "little"), out))
    return out.raw


def pairing_check(pairs: list) -> bool:
    """True iff prod e(P_i, Q_i) == 1; pairs = [(g1_96_bytes_or_None, g2_192_bytes), ...]. Host-side."""
    g1 = b"".join(bytes(96) if p is None else p for p, _ in pairs)
    g2 = b"".join(q for _, q in pairs)
    ok = c_int(0)
    _check(lib().dr_pairing_check(g1, g2, len(pairs), byref(ok)))
    return bool(ok.value)


def g1_neg(xy: bytes | None) -> bytes | None:
    if xy is None:
        return None
    y = int.from_bytes(xy[48:], "big")
    p = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
    return xy[:48] + ((p - y) % p).to_bytes(48, "big")


def g1_compress(xy: bytes | None) -> bytes:
    out = ctypes.create_string_buffer(48)
    _check(lib().dr_g1_compress(xy if xy is not None else bytes(96), 1 if xy is None else 0, out))
    return out.raw


def g1_decompress(data: bytes) -> bytes | None:
    if len(data) != 48:
        raise ValueError(f"invalid BLS12-381 G1 length: expected 48, got {len(data)}")
    out, inf = ctypes.create_string_buffer(96), c_int(0)
    _check(lib().dr_g1_decompress(data, out, byref(inf)))
    return None if inf.value else out.raw
