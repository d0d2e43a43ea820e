#!/usr/bin/env python3
"""Time Bls12381G2Point.msm on the GPU against the only route the tree offered for the same sum before dr_blsg2_msm existed —
Context.blsg2_scalar_mul_batch over all terms, then the host's affine additions — and the two paths of dr_blsg2_msm against each other
around its threshold: the sibling of narrow_msm_sweep.py.  BLSG2_PIP_FROM (csrc/msm_plan.hpp) is read off the second table.

    python3 tools/g2_msm_sweep.py [--sizes 64,256,257,1024,4096,65536] [--threshold-sizes 257,513,1025] [--reps 5]

Per size the two sides are timed in alternating rounds, `reps` rounds each after one unmeasured call of both; a round repeats the call
until it has lasted 50 ms and reports the time per call.  Wall clock around the Python call (packing, the C call, which ends in a device
synchronise, the kernels, the host's combination), which is what a caller waits for; median and minimum over the rounds.  Points are
distinct multiples of the generator made on the device, scalars 256 bits.  The old route is this tree's own unchanged code, so both
sides are timed in one process.
  msm          point_type.msm(points, scalars)
  old_route    blsg2_scalar_mul_batch of all terms (96-byte scalars), then a left-to-right sum by Bls12381G2Point.__add__
  buckets      Context.blsg2_msm on packed bytes (from the threshold on: the bucket method)
  groups       the path dr_blsg2_msm takes BELOW its threshold, forced at this size: blsg2_msm_groups in chunks of 64 (the walk
               starts at the wave's top set bit, so 96-byte scalars below 2^256 cost what 32-byte ones do), partial sums added on the host
One JSON line per measurement."""
import argparse
import json
import os
import random
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="64,256,257,1024,4096,65536")
    ap.add_argument("--threshold-sizes", default="257,513,1025")
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import dot_ring_amd as d
    from dot_ring_amd import runtime

    pt = d.BLS12_381_G2.point_type
    ctx = runtime.context()
    sizes = [int(x) for x in args.sizes.split(",") if x]
    around = [int(x) for x in args.threshold_sizes.split(",") if x]
    rng = random.Random("g2-msm-sweep")

    def one_round(fn):
        calls, t = 0, time.perf_counter()
        while True:
            fn()
            calls += 1
            spent = time.perf_counter() - t
            if spent >= 0.05:
                return spent * 1e3 / calls

    def emit_pair(n, sides):
        """sides: (what, fn) twice, timed in alternating rounds"""
        for _, fn in sides:
            fn()
        ts = {what: [] for what, _ in sides}
        for _ in range(args.reps):
            for what, fn in sides:
                ts[what].append(one_round(fn))
        for what, _ in sides:
            print(json.dumps({"suite": "blsg2", "what": what, "n": n, "median_ms": round(statistics.median(ts[what]), 3),
                              "min_ms": round(min(ts[what]), 3), "rounds": args.reps}), flush=True)

    top = min(max(sizes + around), 8192)
    pool = pt.scalar_mul_batch([pt.generator_point()] * top, [rng.getrandbits(200) | 1 for _ in range(top)])

    def old_route(pts, ks):
        raw = ctx.blsg2_scalar_mul_batch(pt._pack(pts), b"".join(k.to_bytes(96, "little") for k in ks))
        acc = pt.identity()
        for term in pt._unpack(raw):
            acc = acc + term
        return acc

    def groups_path(raw_pts, ks):
        pad = -len(ks) % 64
        parts = ctx.blsg2_msm_groups(raw_pts + bytes(192 * pad), b"".join(k.to_bytes(96, "little") for k in ks) + bytes(96 * pad), 64)
        acc = pt.identity()
        for term in pt._unpack(parts):
            acc = acc + term
        return acc

    for n in sizes:
        pts = [pool[i % len(pool)] for i in range(n)]
        ks = [rng.getrandbits(256) for _ in range(n)]
        if pt.msm(pts, ks) != old_route(pts, ks):
            raise SystemExit(f"the two routes disagree at {n} terms")
        emit_pair(n, (("msm", lambda: pt.msm(pts, ks)), ("old_route", lambda: old_route(pts, ks))))
    for n in around:
        pts = [pool[i % len(pool)] for i in range(n)]
        ks = [rng.getrandbits(256) for _ in range(n)]
        raw_pts, raw_ks = pt._pack(pts), b"".join(k.to_bytes(32, "little") for k in ks)
        if pt._unpack(ctx.blsg2_msm(raw_pts, raw_ks))[0] != groups_path(raw_pts, ks):
            raise SystemExit(f"the two paths disagree at {n} terms")
        emit_pair(n, (("buckets", lambda: ctx.blsg2_msm(raw_pts, raw_ks)), ("groups", lambda: groups_path(raw_pts, ks))))


if __name__ == "__main__":
    main()
