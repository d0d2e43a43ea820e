"""P384_RO against P521_RO and Ed448_RO (the other wide suites with VRFs and the same Python orchestration; P-384 runs 14 limbs in
Montgomery form against P-521's 19 with a fold and Ed448's 16, 97 windows against 131 and 113, the complete a = -3 law of P-521 and
SHA-384 transcripts): scalar_mul_batch, 64-term MSM groups, RO encodings, prove_batch for Tiny, Thin and Pedersen and the batch
verifiers, B items each.  One fresh process per run, a warm-up of every call first, the three suites alternating, host clock around
the (synchronous) calls, the median of `reps` calls; prints the three times and P-384's two ratios
(python tools/p384_suite_timing.py [reps] [B]).  Repeat the process and take the median of the medians."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import curve  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
B = int(sys.argv[2]) if len(sys.argv) > 2 else 256


def work(cv):
    sks = [(1000 + i).to_bytes(56, "little") for i in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    tiny, thin, ped = d.TinyVRF[cv], d.ThinVRF[cv], d.PedersenVRF[cv]
    pt = cv.point_type
    pks = [cv.public_key_from_secret(sk) for sk in sks]
    hashed = pt.encode_to_curve_batch(als)
    ks = [int.from_bytes(sk, "little") * 0x9E3779B97F4A7C15 % pt._N for sk in sks]
    proofs = {"thin": thin.prove_batch(als, sks, ads), "ped": ped.prove_batch(als, sks, ads)}
    return {
        "encode_to_curve": lambda: pt.encode_to_curve_batch(als),
        "scalar_mul_batch": lambda: curve.scalar_mul_batch(hashed, ks),
        "msm_groups m=64": lambda: curve.msm_groups(hashed, ks, 64),
        "Tiny.prove_batch": lambda: tiny.prove_batch(als, sks, ads),
        "Thin.prove_batch": lambda: thin.prove_batch(als, sks, ads),
        "Pedersen.prove_batch": lambda: ped.prove_batch(als, sks, ads),
        "Thin.batch_verify": lambda: thin.batch_verify(proofs["thin"], pks, als, ads),
        "Pedersen.batch_verify": lambda: ped.batch_verify(proofs["ped"], als, ads),
    }


def main():
    suites = [d.Ed448_RO, d.P521_RO, d.P384_RO]
    calls = {cv.name: work(cv) for cv in suites}
    for per in calls.values():                               # warm-up
        for f in per.values():
            f()
    for op in calls[suites[0].name]:
        times = {cv.name: [] for cv in suites}
        for _ in range(REPS):
            for cv in suites:                                # alternating
                t = time.perf_counter()
                out = calls[cv.name][op]()
                times[cv.name].append(time.perf_counter() - t)
                assert out is not False, (cv.name, op)
        med = {k: statistics.median(v) for k, v in times.items()}
        line = " | ".join(f"{k} {med[k] * 1e3:8.2f} ms" for k in med)
        print(f"B={B:5d} {op:22s} {line} | P384_RO/P521_RO time {med['P384_RO'] / med['P521_RO']:.3f} | P384_RO/Ed448_RO time "
              f"{med['P384_RO'] / med['Ed448_RO']:.3f}", flush=True)


if __name__ == "__main__":
    main()
