"""CPU: the ring proof's Fiat-Shamir schedule in groups of four proofs (dot_ring_amd/csrc/hostring.hpp, shared by the batch prover and the
batch verifier) and the verifier arithmetic beside RingClaimScalars (hostproto.hpp), compiled with plain g++ behind a line-oriented
harness (tests/native/ring_fs_check.cpp).  The schedule is compared with the oracle's derive_challenges for every proof of batches of
1, 3, 4, 5 and 9 proofs — a full group, partial groups whose spare slots repeat the last proof, more than two groups — and the
arithmetic with Python integers.  Every check runs on two builds of the harness: the plain one and one with the address and
undefined-behaviour sanitizers."""
import hashlib
import os
import random
import struct
import subprocess

import pytest

from oracle.pyref import ring as oring

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = oring.P
BUILDS = {"plain": ["-O2"], "sanitized": ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]}


class Harness:
    def __init__(self, exe):
        self.proc = subprocess.Popen([exe], stdin=subprocess.PIPE, stdout=subprocess.PIPE, text=True)

    def ask(self, *fields) -> list:
        self.proc.stdin.write(" ".join((f.hex() or "-") if isinstance(f, (bytes, bytearray)) else str(f) for f in fields) + "\n")
        self.proc.stdin.flush()
        return self.proc.stdout.readline().split()

    def close(self) -> int:
        self.proc.stdin.close()
        return self.proc.wait(timeout=30)


@pytest.fixture(scope="module", params=list(BUILDS))
def harness(request, tmp_path_factory):
    exe = tmp_path_factory.mktemp("ring_fs_" + request.param) / "ring_fs_check"
    subprocess.run(["g++", *BUILDS[request.param], "-std=c++17", "-pthread", "-Wno-psabi", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "ring_fs_check.cpp"), "-o", str(exe)], check=True)
    h = Harness(str(exe))
    yield h
    assert h.close() == 0, "the harness did not end cleanly (a sanitizer report ends it with a non-zero status)"


def _le32(v):
    return int(v).to_bytes(32, "little")


def _ints(blob):
    return [int.from_bytes(blob[i : i + 32], "little") for i in range(0, len(blob), 32)]


@pytest.mark.parametrize("batch", [1, 3, 4, 5, 9])
def test_grouped_schedule_equals_the_oracle_for_every_proof(harness, batch):
    """alphas, zeta and nus of every proof from the grouped schedule == derive_challenges on that proof's bytes alone: the spare slots
    of a partial group leave no trace, and prover-style (round by round) and verifier-style (group by group) runs agree"""
    rng = random.Random(1000 + batch)
    initial = bytes(rng.randrange(256) for _ in range(40 + batch))
    body = bytes(rng.randrange(256) for _ in range(100))
    prefix = oring.FsTranscript(initial)                      # what both sides have absorbed before "instance": a label and a key
    prefix.absorb(b"vk", body)
    prefix_bytes = initial + struct.pack(">I", len(initial)) + b"vk" + struct.pack(">I", 2) + body + struct.pack(">I", len(body))
    rel = [(rng.randrange(1 << 256), rng.randrange(1 << 256)) for _ in range(batch)]
    cols = [bytes(rng.randrange(256) for _ in range(384)) for _ in range(batch)]
    cq = [bytes(rng.randrange(256) for _ in range(96)) for _ in range(batch)]
    evals = [[rng.randrange(1 << 256) for _ in range(7)] for _ in range(batch)]
    lzw = [rng.randrange(1 << 256) for _ in range(batch)]
    out = harness.ask("schedule", prefix_bytes, batch, b"".join(_le32(x) + _le32(y) for x, y in rel), b"".join(cols), b"".join(cq),
                      b"".join(_le32(e) for ev in evals for e in ev), b"".join(_le32(v) for v in lzw))
    assert out[0] == "challenges", out
    alphas, zetas, nus = (_ints(bytes.fromhex(h)) for h in out[1:4])
    assert len(alphas) == 7 * batch and len(zetas) == batch and len(nus) == 8 * batch
    for i in range(batch):
        want_alphas, want_zeta, want_nus = oring.derive_challenges(prefix, rel[i], cols[i], cq[i], evals[i], lzw[i])
        assert alphas[7 * i : 7 * i + 7] == want_alphas, (batch, i)
        assert zetas[i] == want_zeta, (batch, i)
        assert nus[8 * i : 8 * i + 8] == want_nus, (batch, i)


def test_verifier_randomness_is_shake256_of_seed_and_counter(harness):
    """coefficient k of proof i = SHAKE256(seed || LE64(2 i + k)), 48 bytes big-endian mod p, zero -> 1 (never hit by a hash output)"""
    rng = random.Random(77)
    for seed in (bytes(32), bytes(rng.randrange(256) for _ in range(32))):
        for i, k in ((0, 0), (0, 1), (1, 0), (7, 1), (4095, 1), (1 << 40, 0)):
            want = int.from_bytes(hashlib.shake_256(seed + struct.pack("<Q", 2 * i + k)).digest(48), "big") % P or 1
            out = harness.ask("random", seed, i, k)
            assert out[0] == "scalar" and int.from_bytes(bytes.fromhex(out[1]), "little") == want, (i, k)


def test_claim_fold_against_python_integers(harness):
    """the seven lhs scalars in the verifier's gather order and the four summands on the fixed points, for random claim scalars and
    randomness, with zero, one and p - 1 among them"""
    rng = random.Random(78)
    cases = [[rng.randrange(P) for _ in range(17)] for _ in range(6)]
    cases.append([0] * 17)
    cases.append([P - 1] * 17)
    cases.append([1] * 15 + [0, P - 1])
    for vals in cases:
        nus, (k_ip, k_x, k_y, zeta, zeta_omega, agg, l_zw), (r1, r2) = vals[:8], vals[8:15], vals[15:]
        out = harness.ask("fold", b"".join(_le32(v) for v in vals[:15]), _le32(r1), _le32(r2))
        assert out[0] == "fold", out
        lhs, fixed = _ints(bytes.fromhex(out[1])), _ints(bytes.fromhex(out[2]))
        assert lhs == [r1 * nus[3] % P, (r1 * nus[4] + r2 * k_ip) % P, (r1 * nus[5] + r2 * k_x) % P, (r1 * nus[6] + r2 * k_y) % P,
                       r1 * nus[7] % P, r1 * zeta % P, r2 * zeta_omega % P]
        assert fixed == [r1 * nus[0] % P, r1 * nus[1] % P, r1 * nus[2] % P, (r1 * agg + r2 * l_zw) % P]
