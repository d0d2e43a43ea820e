#!/usr/bin/env python3
"""Wall time of one `encode_to_curve_batch` call at 4096 messages for BLS12_381_G2_RO and, in the same process, for BLS12_381_G1_RO
(the same field, chain and law one level down: the yardstick DESIGN.md 8l quotes).  `python3 tools/blsg2_encode_timing.py [count]`.
Each figure is ONE call after one warm-up call of the same size — unrepeated, to be quoted as such."""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import dot_ring_amd as d  # noqa: E402


def main():
    count = int(sys.argv[1]) if len(sys.argv) > 1 else 4096
    msgs = [b"message %d" % i for i in range(count)]
    for cv in (d.BLS12_381_G2_RO, d.BLS12_381_G1_RO):
        cv.point_type.encode_to_curve_batch(msgs)                      # warm-up: buffers, code object
        t0 = time.perf_counter()
        out = cv.point_type.encode_to_curve_batch(msgs)
        ms = (time.perf_counter() - t0) * 1e3
        assert len(out) == count
        print(f"{cv.name}: encode_to_curve_batch({count}) {ms:.2f} ms")


if __name__ == "__main__":
    main()
