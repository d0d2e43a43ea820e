"""Curve25519_RO against Ed25519_RO (the same group operations and transcript hash; Curve25519 adds the change of model at both ends of
each kernel — one inversion per stored point — and hashes 64-byte points where Ed25519 hashes 32): prove_batch and batch_verify of 4096
for Tiny, Thin and Pedersen, and 4096 RO encodings.  One fresh process per run, a warm-up of every call first, the two suites
alternating, host clock around the (synchronous) calls, the median of `reps` calls; prints both times and their ratio
(python tools/curve25519_suite_timing.py [reps] [suites]).  `suites` = `ed` times Ed25519_RO alone: the form that runs on a commit
without Curve25519, whose column is the yardstick.  Repeat the process and take the median of the medians."""
import os
import statistics
import sys
import time

sys.path.insert(0, os.getcwd())
import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import runtime  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
ONLY_ED = len(sys.argv) > 2 and sys.argv[2] == "ed"
B = 4096


def work(cv):
    sks = [(1000 + i).to_bytes(32, "little") for i in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    tiny, thin, ped = d.TinyVRF[cv], d.ThinVRF[cv], d.PedersenVRF[cv]
    suite, ctx = cv.point_type._suite_struct(), runtime.context()
    pks = [cv.public_key_from_secret(sk) for sk in sks]
    proofs = {"tiny": tiny.prove_batch(als, sks, ads), "thin": thin.prove_batch(als, sks, ads), "ped": ped.prove_batch(als, sks, ads)}
    return {
        "encode_to_curve": lambda: ctx.encode_to_curve_batch(suite, als, None),
        "Tiny.prove_batch": lambda: tiny.prove_batch(als, sks, ads),
        "Thin.prove_batch": lambda: thin.prove_batch(als, sks, ads),
        "Pedersen.prove_batch": lambda: ped.prove_batch(als, sks, ads),
        "Tiny.verify x64": lambda: all(p.verify(pk, al, ad) for p, pk, al, ad in zip(proofs["tiny"][:64], pks, als, ads)),
        "Thin.batch_verify": lambda: thin.batch_verify(proofs["thin"], pks, als, ads),
        "Pedersen.batch_verify": lambda: ped.batch_verify(proofs["ped"], als, ads),
    }


def main():
    suites = [d.Ed25519_RO] if ONLY_ED else [d.Ed25519_RO, d.Curve25519_RO]
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
        ratio = "" if ONLY_ED else f" | Curve25519_RO/Ed25519_RO time {med['Curve25519_RO'] / med['Ed25519_RO']:.3f}"
        print(f"B={B:5d} {op:22s} {line}{ratio}", flush=True)


if __name__ == "__main__":
    main()
