"""secp256k1 against P-256 (same protocols, 33-byte points, cofactor 1, SHA-256; secp256k1 has the cheaper field reduction, the a = 0
law and RFC 9380 hashing to the curve instead of try-and-increment): Tiny / Thin / Pedersen prove_batch, Thin / Pedersen batch_verify
at 1024 and 4096 proofs and encode_to_curve_batch of 4096 messages, one fresh process, a warm-up of every call first, the two suites
alternating, host clock around the (synchronous) calls; prints both rates and their ratio
(python tools/secp256k1_suite_timing.py [reps]).  Under rocprofv3 --kernel-trace --stats, SECP256K1_ONLY=1 times secp256k1 alone."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import dot_ring_amd as d  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
SUITES = [d.Secp256k1] if os.environ.get("SECP256K1_ONLY") else [d.P256, d.Secp256k1]


def work(cv, B):
    sks = [(1000 + i).to_bytes(32, "little") for i in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    tiny, thin, ped = d.TinyVRF[cv], d.ThinVRF[cv], d.PedersenVRF[cv]
    thin_proofs = thin.prove_batch(als, sks, ads)
    ped_proofs = ped.prove_batch(als, sks, ads)
    pks = [p.point_to_string() for p in d.curve.scalar_mul_batch([cv.point_type.generator_point()] * B,
                                                                 [int.from_bytes(s, "little") for s in sks])]
    return {
        "Tiny.prove_batch": lambda: tiny.prove_batch(als, sks, ads),
        "Thin.prove_batch": lambda: thin.prove_batch(als, sks, ads),
        "Pedersen.prove_batch": lambda: ped.prove_batch(als, sks, ads),
        "Thin.batch_verify": lambda: thin.batch_verify(thin_proofs, pks, als, ads),
        "Pedersen.batch_verify": lambda: ped.batch_verify(ped_proofs, als, ads),
        "encode_to_curve_batch": lambda: cv.point_type.encode_to_curve_batch(als),
    }


def main():
    for B in (1024, 4096):
        calls = {cv.name: work(cv, B) for cv in SUITES}
        for per in calls.values():                       # warm-up
            for f in per.values():
                f()
        for op in calls[SUITES[0].name]:
            best = {cv.name: float("inf") for cv in SUITES}
            for _ in range(REPS):
                for cv in SUITES:                        # alternating
                    t = time.perf_counter()
                    out = calls[cv.name][op]()
                    best[cv.name] = min(best[cv.name], time.perf_counter() - t)
                    assert out is not False, (cv.name, op)
            rates = {k: B / v for k, v in best.items()}
            line = " | ".join(f"{k} {rates[k]:9.0f} /s ({best[k] * 1e3:7.1f} ms)" for k in rates)
            if len(rates) == 2:
                line += f" | Secp256k1/P256 {rates['Secp256k1_RO'] / rates['P256_TAI']:.3f}"
            print(f"B={B:5d} {op:22s} {line}", flush=True)


if __name__ == "__main__":
    main()
