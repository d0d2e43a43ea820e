#!/usr/bin/env python3
"""Wall time of one `encode_to_curve_batch` call at 4096 messages for Ed448_RO and, in the same process, for Ed25519_RO (the same map
one field down: the yardstick DESIGN.md 8m quotes).  `python3 tools/ed448_encode_timing.py [count]`.
Each figure is ONE call after one warm-up call of the same size — unrepeated, to be quoted as such."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dot_ring_amd as d  # noqa: E402


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    msgs = [b"message %d" % i for i in range(count)]
    for cv in (d.Ed448_RO, d.Ed25519_RO):
        cv.point_type.encode_to_curve_batch(msgs)                      # warm-up: buffers, code object
        t0 = time.perf_counter()
        out = cv.point_type.encode_to_curve_batch(msgs)
        ms = (time.perf_counter() - t0) * 1e3
        assert len(out) == count
        print(f"{cv.name}: encode_to_curve_batch({count}) {ms:.2f} ms")


if __name__ == "__main__":
    main()
