#!/usr/bin/env python3
"""RingVRF.verify_each against batch_verify and the per-proof verify loop: ring domain 1024, 1024 proofs per call.

Every repeat is a fresh process (as tools/run_variance.sh does for the headline step): it builds the ring, proves the batch once,
then times batch_verify on the all-valid batch, verify_each on the same batch and with 1, 8 and 64 damaged proofs (an evaluation
scalar changed: the ring part fails, so the descent pays pairings), and proof.verify one at a time on 64 proofs (scaled to the batch).
Prints the per-repeat figures and their medians, with the number of pairing equations verify_each evaluated (stats[0]).

  python3 tools/verify_each_sweep.py [--repeats 3] [--calls 5] [--proofs 1024] [--root DIR]

--root DIR measures the checkout at DIR instead of this one (a built checkout of the parent commit gives the parent's batch_verify on
the same box in the same call; verify_each figures are skipped where the method does not exist).  DOTRING_TRACE=1 in the
environment adds the phase lines of the native calls on stderr."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001


def child(proofs_n: int, calls: int) -> None:
    import dot_ring_amd as d
    from dot_ring_amd.curve import scalar_mul_batch

    cv = d.Bandersnatch
    vrf = d.RingVRF[cv]
    members = 300                                            # -> domain 1024
    sks = [(31000 + i).to_bytes(32, "little") for i in range(members)]
    keys = [p.point_to_string() for p in scalar_mul_batch([cv.point_type.generator_point()] * members, [int.from_bytes(s, "little") for s in sks])]
    params = d.RingProofParams.from_ring_size(members)
    assert params.domain_size == 1024
    ring = d.Ring(keys, params)
    root = d.RingRoot.from_ring(ring, params)
    als = [b"sweep-%d" % i for i in range(proofs_n)]
    ads = [b"ad"] * proofs_n
    who = [i % members for i in range(proofs_n)]
    proofs = vrf.prove_batch(als, ads, [sks[w] for w in who], [keys[w] for w in who], ring, root)
    raw = [p.encode() for p in proofs]

    class Blob:
        def __init__(self, b):
            self._b = b

        def encode(self):
            return self._b

    def damaged(k):
        out = list(raw)
        for j in range(k):
            i = (j * proofs_n) // k + (proofs_n // (2 * k))
            b = out[i]
            out[i] = b[:384] + ((int.from_bytes(b[384:416], "little") + 1) % FR).to_bytes(32, "little") + b[416:]
        return [Blob(b) for b in out]

    def timed(f, n=calls):
        f()                                                  # warm-up: buffers, tables, the worker pool
        ts = []
        for _ in range(n):
            t0 = time.perf_counter()
            r = f()
            ts.append((time.perf_counter() - t0) * 1e3)
        return statistics.median(ts), r

    res = {}
    ms, ok = timed(lambda: vrf.batch_verify(proofs, als, ads, ring, root))
    assert ok
    res["batch_verify_ms"] = ms
    if hasattr(vrf, "verify_each"):
        for k in (0, 1, 8, 64):
            objs = proofs if k == 0 else damaged(k)
            stats = {}
            ms, verdicts = timed(lambda: vrf.verify_each(objs, als, ads, ring, root, stats=stats))
            assert verdicts.count(False) == k
            res["verify_each_%d_bad_ms" % k] = ms
            res["verify_each_%d_bad_pairings" % k] = stats["pairings"]
    loop_n = min(64, proofs_n)
    ms, oks = timed(lambda: [p.verify(a, x, ring, root) for p, a, x in zip(proofs[:loop_n], als, ads)], max(1, calls // 2))
    assert all(oks)
    res["verify_loop_%d_ms" % loop_n] = ms
    res["verify_loop_scaled_ms"] = ms * proofs_n / loop_n
    print("SWEEP " + json.dumps(res))


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--proofs", type=int, default=1024)
    ap.add_argument("--root", default=HERE)
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        child(a.proofs, a.calls)
        return 0
    rows = []
    for r in range(a.repeats):
        env = dict(os.environ)
        env["PYTHONPATH"] = a.root + os.pathsep + env.get("PYTHONPATH", "")
        out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--proofs", str(a.proofs), "--calls", str(a.calls)],
                             cwd=a.root, env=env, capture_output=True, text=True, timeout=900)
        sys.stderr.write(out.stderr[-4000:])
        if out.returncode != 0:
            print("repeat %d failed" % r)
            return 1
        row = [json.loads(ln[6:]) for ln in out.stdout.splitlines() if ln.startswith("SWEEP ")][0]
        rows.append(row)
        print("repeat %d %s" % (r, " ".join("%s=%.2f" % kv for kv in row.items())), flush=True)
    print("median   %s" % " ".join("%s=%.2f" % (k, statistics.median(row[k] for row in rows)) for k in rows[0]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
