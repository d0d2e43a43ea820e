#!/usr/bin/env python3
"""Wall time of one `encode_to_curve_batch` call at 4096 messages for a suite and, in the same process, for its yardstick: the suite
DESIGN.md compares it with.  `python3 tools/encode_timing.py SUITE YARDSTICK [count]`, the names as dot_ring_amd exports them:
  BLS12_381_G1_RO Secp256k1_RO      the only other SSWU-with-isogeny suite
  BLS12_381_G2_RO BLS12_381_G1_RO   the same field, chain and law one level down
  Ed448_RO Ed25519_RO               the same map one field down
  Curve448_RO Ed448_RO              the same field and the same Elligator 2; another law and no isogeny after the map
  P521_RO Ed448_RO                  the other wide suite with VRFs: 19 limbs against 16, SSWU against Elligator 2
  P384_RO P521_RO                   the same map and law on 14 Montgomery limbs against 19 with a fold, SHA-384 against SHA-512
Each figure is ONE call after one warm-up call of the same size — unrepeated, to be quoted as such."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dot_ring_amd as d  # noqa: E402


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    count = int(sys.argv[3]) if len(sys.argv) > 3 else 4096
    msgs = [b"message %d" % i for i in range(count)]
    for cv in (getattr(d, sys.argv[1]), getattr(d, sys.argv[2])):
        cv.point_type.encode_to_curve_batch(msgs)                      # warm-up: buffers, code object
        t0 = time.perf_counter()
        out = cv.point_type.encode_to_curve_batch(msgs)
        ms = (time.perf_counter() - t0) * 1e3
        assert len(out) == count
        print(f"{cv.name}: encode_to_curve_batch({count}) {ms:.2f} ms")


if __name__ == "__main__":
    main()
