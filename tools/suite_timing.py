"""One suite against a yardstick suite with the same protocols: Tiny / Thin / Pedersen prove_batch, Thin / Pedersen batch_verify and
encode_to_curve_batch at 1024 and 4096 proofs, one fresh process, a warm-up of every call first, the two suites alternating, host clock
around the (synchronous) calls; prints both rates and their ratio:
    python tools/suite_timing.py SUITE [YARDSTICK] [reps]
The pairs the design notes quote: Bandersnatch_SW Bandersnatch, Ed25519 JubJub, P256 Ed25519, BabyJubJub JubJub, Secp256k1 P256.
Without a yardstick (under rocprofv3 --kernel-trace --stats, say) the suite is timed alone."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import dot_ring_amd as d  # noqa: E402

NAMES = [a for a in sys.argv[1:] if not a.isdigit()]
REPS = next((int(a) for a in sys.argv[1:] if a.isdigit()), 3)
if not 1 <= len(NAMES) <= 2:
    raise SystemExit(__doc__)
SUITES = [getattr(d, n) for n in reversed(NAMES)]           # the yardstick first, as the per-suite tools had it


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
                base, suite = (cv.name for cv in SUITES)
                line += f" | {suite}/{base} {rates[suite] / rates[base]:.3f}"
            print(f"B={B:5d} {op:22s} {line}", flush=True)


if __name__ == "__main__":
    main()
