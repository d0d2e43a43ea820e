#!/usr/bin/env python3
"""Time point_type.msm and the batch verifiers of the wide suites (P-384, P-521, Ed448, Curve448) on the GPU, for the A/B of the bucket
method (dr_wide_msm) against a tree without it.

    python3 tools/wide_msm_sweep.py [--tree DIR] [--suites p384,p521,ed448,curve448] [--sizes 128,256,...] [--proofs 1024] [--reps 3]

--tree: the source tree whose dot_ring_amd is measured (default: this one); for the parent commit, a worktree of it built under ab_old/
(tools/ab_commits.sh says how).  One fresh process per tree.  Per suite and size: one unmeasured call, then the median and the minimum of
`reps` calls of point_type.msm over distinct points (multiples of the generator made on the device) and full-width scalars; then
ThinVRF and PedersenVRF batch_verify over `proofs` proofs of prove_batch (5 terms per proof in one MSM).  Wall clock around the Python call,
which is what a verifier waits for: packing, the C call, the kernels, the host's window combination.  One JSON line per measurement."""
import argparse
import json
import os
import random
import statistics
import sys
import time


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tree", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    ap.add_argument("--suites", default="p384,p521,ed448,curve448")
    ap.add_argument("--sizes", default="128,256,512,1024,5120,16384,65536")
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import dot_ring_amd as d
    from dot_ring_amd.curve import scalar_mul_batch

    curves = {"p384": d.P384, "p521": d.P521, "ed448": d.Ed448, "curve448": d.Curve448}
    sizes = [int(x) for x in args.sizes.split(",") if x]
    label = args.label or os.path.basename(os.path.abspath(args.tree))

    def timed(fn):
        if fn() is False:
            raise SystemExit("the measured call returned False")
        ts = []
        for _ in range(args.reps):
            t = time.perf_counter()
            fn()
            ts.append((time.perf_counter() - t) * 1e3)
        return round(statistics.median(ts), 3), round(min(ts), 3)

    for name in args.suites.split(","):
        cv = curves[name]
        pt = cv.point_type
        rng = random.Random("wide-msm-sweep/" + name)
        bits = 521 if name == "p521" else 8 * len(pt._scalars([1]))
        top = max(sizes) if sizes else 0
        g = pt.generator_point()
        pool = scalar_mul_batch([g] * min(top, 8192), [rng.getrandbits(200) | 1 for _ in range(min(top, 8192))]) if top else []
        for n in sizes:
            pts = [pool[i % len(pool)] for i in range(n)]
            ks = [rng.getrandbits(bits) for _ in range(n)]
            med, low = timed(lambda: pt.msm(pts, ks))
            print(json.dumps({"tree": label, "suite": name, "what": "msm", "n": n, "median_ms": med, "min_ms": low}), flush=True)
        if args.proofs:
            b = args.proofs
            sks = [rng.getrandbits(250).to_bytes(32, "little") for _ in range(b)]
            alphas = [b"sweep %d" % i for i in range(b)]
            ads = [b""] * b
            pks = [cv.public_key_from_secret(sk) for sk in sks[:1]] * b
            thin = d.ThinVRF[cv].prove_batch(alphas, [sks[0]] * b, ads)
            med, low = timed(lambda: d.ThinVRF[cv].batch_verify(thin, pks, alphas, ads))
            print(json.dumps({"tree": label, "suite": name, "what": "thin_batch_verify", "n": b, "median_ms": med, "min_ms": low}), flush=True)
            ped = d.PedersenVRF[cv].prove_batch(alphas, sks, ads)
            med, low = timed(lambda: d.PedersenVRF[cv].batch_verify(ped, alphas, ads))
            print(json.dumps({"tree": label, "suite": name, "what": "pedersen_batch_verify", "n": b, "median_ms": med, "min_ms": low}), flush=True)


if __name__ == "__main__":
    main()
