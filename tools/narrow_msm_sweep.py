#!/usr/bin/env python3
"""Time point_type.msm and the batch verifiers of the 256-bit suites (Ed25519, Baby JubJub, P-256, secp256k1, Curve25519) and of
BLS12-381's E(Fq) on the GPU, for the A/B of the bucket method under dr_te_msm / dr_blsg1_msm against a tree without it: the sibling of
wide_msm_sweep.py, whose method this is.  NARROW_PIP_FROM (csrc/msm_plan.hpp) is read off its table.

    python3 tools/narrow_msm_sweep.py [--tree DIR] [--suites ed25519,...] [--sizes 257,320,...] [--proofs 1024] [--reps 3]

--tree: the source tree whose dot_ring_amd is measured (default: this one); for the parent commit, a built worktree of it.  One fresh
process per tree and suite, the parent first.  Per size: one unmeasured call, then the median and the minimum of `reps` calls of
point_type.msm over distinct points (multiples of the generator made on the device) and 256-bit scalars; then ThinVRF and PedersenVRF
batch_verify over `proofs` proofs of prove_batch.  Wall clock around the Python call, which is what a verifier waits for: packing, the
scalar reduction, the C call, the kernels, the host's window combination.  One JSON line per measurement."""
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
    ap.add_argument("--suites", default="ed25519,bjj,p256,secp256k1,curve25519,blsg1")
    ap.add_argument("--sizes", default="257,320,512,1024,4096,16384,65536")
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--label", default="")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import dot_ring_amd as d
    from dot_ring_amd.curve import scalar_mul_batch

    curves = {"ed25519": d.Ed25519, "bjj": d.BabyJubJub, "p256": d.P256, "secp256k1": d.Secp256k1, "curve25519": d.Curve25519, "blsg1": d.BLS12_381_G1}
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
        rng = random.Random("narrow-msm-sweep/" + name)
        top = max(sizes) if sizes else 0
        g = pt.generator_point()
        pool = scalar_mul_batch([g] * min(top, 8192), [rng.getrandbits(200) | 1 for _ in range(min(top, 8192))]) if top else []
        for n in sizes:
            pts = [pool[i % len(pool)] for i in range(n)]
            ks = [rng.getrandbits(256) for _ in range(n)]
            med, low = timed(lambda: pt.msm(pts, ks))
            print(json.dumps({"tree": label, "suite": name, "what": "msm", "n": n, "median_ms": med, "min_ms": low}), flush=True)
        if args.proofs and name != "blsg1":                      # (no VRF is timed over E(Fq): its verifiers' sizes are the msm rows)
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
