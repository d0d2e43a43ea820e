"""The RFC 9380 variants of P-256 and Ed25519 against their try-and-increment variants (same group, kernels, protocols and transcript
hash; only the way a message becomes a point differs, and for P-256 the point encoding): encode_to_curve of 1024 and 4096 messages
through the library's batch entry point (hash_to_field on the host's worker threads and ONE launch of the map kernel, against the
candidates of several counters hashed on the host and decoded in as many launches as it takes), and Tiny / Pedersen prove_batch on
both variants.  One fresh process, a warm-up of every call first, the two variants of a curve alternating, host clock around the
(synchronous) calls, best of `reps` calls; prints both times and their ratio (python tools/h2c_suite_timing.py [reps])."""
import os
import sys
import time

sys.path.insert(0, os.getcwd())
import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import runtime  # noqa: E402

REPS = int(sys.argv[1]) if len(sys.argv) > 1 else 3
PAIRS = [(d.P256_TAI, d.P256_RO), (d.Ed25519_TAI, d.Ed25519_RO)]


def work(cv, B):
    sks = [(1000 + i).to_bytes(32, "little") for i in range(B)]
    als = [b"alpha-%d" % i for i in range(B)]
    ads = [b"ad-%d" % (i % 5) for i in range(B)]
    tiny, ped = d.TinyVRF[cv], d.PedersenVRF[cv]
    suite, ctx = cv.point_type._suite_struct(), runtime.context()
    return {
        "encode_to_curve": lambda: ctx.encode_to_curve_batch(suite, als, None),
        "Tiny.prove_batch": lambda: tiny.prove_batch(als, sks, ads),
        "Pedersen.prove_batch": lambda: ped.prove_batch(als, sks, ads),
    }


def main():
    for B in (1024, 4096):
        for tai, rfc in PAIRS:
            calls = {cv.name: work(cv, B) for cv in (tai, rfc)}
            for per in calls.values():                       # warm-up
                for f in per.values():
                    f()
            for op in calls[tai.name]:
                best = {tai.name: float("inf"), rfc.name: float("inf")}
                for _ in range(REPS):
                    for cv in (tai, rfc):                    # alternating
                        t = time.perf_counter()
                        out = calls[cv.name][op]()
                        best[cv.name] = min(best[cv.name], time.perf_counter() - t)
                        assert out is not False, (cv.name, op)
                line = " | ".join(f"{k} {best[k] * 1e3:8.2f} ms" for k in best)
                print(f"B={B:5d} {op:22s} {line} | {rfc.name}/{tai.name} time {best[rfc.name] / best[tai.name]:.3f}", flush=True)


if __name__ == "__main__":
    main()
