"""RFC 9380 section 5 on the host, without a GPU.  dot_ring_amd/csrc/hosth2c.hpp (one expand_message_xmd, one expand_message_xof, the
reductions of the wide fields) and hostproto.hpp's hash_to_field_xmd over it are built stand-alone with g++ under the address and
undefined-behaviour sanitizers (tests/native/h2c_hash_check.cpp) and compared with the RFC's `u` values and with the Python restatements
at every message length from 0 to 300 bytes — across every padding boundary of SHA-256 (64-byte blocks), SHA-512 (128) and SHAKE256
(136-byte rate) — under three salts; the reductions also at the edges of their range.  Then the Python side of all fourteen RFC 9380
variants: elements per message, the packed length, the salt as a prefix, and for the six wide variants the point type, the module-level
binding and the restatement against each other."""
import json
import os
import random
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bls12_381_g1_ref as g1  # noqa: E402
import bls12_381_g2_ref as g2  # noqa: E402
import ed448_ref as e448  # noqa: E402
import h2c_ref as h  # noqa: E402
import secp256k1_ref as k1  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dot_ring_amd", "csrc")
FQ_P, FE_P = g1.P, e448.P


def _g2_flat(msg, count, dst):
    return [c for pair in g2.hash_to_field(msg, count, dst) for c in pair]


# (suite, variant) of the program -> (restatement giving the integers of one output line, DST, elements per message)
RESTATED = {
    ("blsg1", "ro"): (g1.hash_to_field, g1.DST_RO, 2), ("blsg1", "nu"): (g1.hash_to_field, g1.DST_NU, 1),
    ("blsg2", "ro"): (_g2_flat, g2.DST_RO, 2), ("blsg2", "nu"): (_g2_flat, g2.DST_NU, 1),
    ("ed448", "ro"): (e448.hash_to_field, e448.DST_RO, 2), ("ed448", "nu"): (e448.hash_to_field, e448.DST_NU, 1),
    ("secp256k1", "ro"): (k1.hash_to_field, k1.DST_RO, 2), ("ed25519", "ro"): (h.ed_hash_to_field, h.ED_DST_RO, 2),
}
GOLDEN_FILES = {("blsg1", "ro"): "bls12_381_G1_ro", ("blsg1", "nu"): "bls12_381_G1_nu", ("blsg2", "ro"): "bls12_381_G2_ro",
                ("blsg2", "nu"): "bls12_381_G2_nu", ("ed448", "ro"): "ed448_ro", ("ed448", "nu"): "ed448_nu"}


@pytest.fixture(scope="module")
def checker(tmp_path_factory):
    exe = tmp_path_factory.mktemp("h2c") / "h2c_hash_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-pthread", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "native", "h2c_hash_check.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        proc = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr[-2000:]
        out = [[int(tok, 16) for tok in row.split()] for row in proc.stdout.splitlines()]
        assert len(out) == len(lines)
        return out

    return run


def _hex(b):
    return b.hex() or "-"


def test_wide_suites_reproduce_the_rfc_vectors(checker, golden_dir):
    lines, want = [], []
    for (suite, variant), name in sorted(GOLDEN_FILES.items()):
        with open(os.path.join(golden_dir, "h2c", name + ".json")) as f:
            doc = json.load(f)
        assert doc["dst"].encode() == RESTATED[suite, variant][1] and len(doc["vectors"]) == 5
        for v in doc["vectors"]:
            lines.append(f"{suite} {variant} - {_hex(v['msg'].encode())}")
            if suite == "blsg2":
                want.append([int(c, 16) for u in v["u"] for c in (u["re"], u["im"])])
            else:
                want.append([int(u, 16) for u in v["u"]])
            assert len(want[-1]) == RESTATED[suite, variant][2] * (2 if suite == "blsg2" else 1)
    assert checker(lines) == want


@pytest.mark.parametrize("suite,variant", sorted(RESTATED))
def test_every_length_against_the_restatement(checker, suite, variant):
    hash_to_field, dst, count = RESTATED[suite, variant]
    rng = random.Random(f"{suite}-{variant}")
    cases = [(salt, rng.randbytes(n)) for salt in (b"", rng.randbytes(1), rng.randbytes(40)) for n in range(301)]
    got = checker([f"{suite} {variant} {_hex(salt)} {_hex(msg)}" for salt, msg in cases])
    for (salt, msg), row in zip(cases, got):
        assert row == hash_to_field(salt + msg, count, dst), (len(salt), len(msg))


@pytest.mark.parametrize("op,size,p", [("reduce64", 64, FQ_P), ("reduce84", 84, FE_P)])
def test_reductions_at_the_edges(checker, op, size, p):
    rng = random.Random(op)
    values = [0, 2 ** (8 * size) - 1, p, p - 1, p + 1]                       # all zero, all 0xff, p and p +- 1 in the low bytes
    values += [(hi << (8 * ((p.bit_length() + 7) // 8))) | lo for hi in (1, 2 ** (8 * (size - (p.bit_length() + 7) // 8)) - 1) for lo in (0, p - 1, p, p + 1)]
    values += [rng.getrandbits(8 * size) for _ in range(64)]
    got = checker([f"{op} {v.to_bytes(size, 'big').hex()}" for v in values])
    assert [row[0] for row in got] == [v % p for v in values]
    assert all(len(row) == 1 for row in got)


# ---------------------------------------------------------------- the Python side
VARIANTS = ["Secp256k1_RO", "Secp256k1_NU", "P256_RO", "P256_NU", "Ed25519_RO", "Ed25519_NU", "Curve25519_RO", "Curve25519_NU",
            "BLS12_381_G1_RO", "BLS12_381_G1_NU", "BLS12_381_G2_RO", "BLS12_381_G2_NU", "Ed448_RO", "Ed448_NU"]
ELEM_BYTES = {"BLS12_381_G1": 48, "BLS12_381_G2": 96, "Ed448": 56}
# variant -> (the module-level binding, the restatement's packing of one message's elements)
WIDE = {
    "BLS12_381_G1_RO": (_native.blsg1_hash_to_field_batch, lambda m: b"".join(u.to_bytes(48, "little") for u in g1.hash_to_field(m, 2, g1.DST_RO))),
    "BLS12_381_G1_NU": (_native.blsg1_hash_to_field_batch, lambda m: b"".join(u.to_bytes(48, "little") for u in g1.hash_to_field(m, 1, g1.DST_NU))),
    "BLS12_381_G2_RO": (_native.blsg2_hash_to_field_batch, lambda m: b"".join(c.to_bytes(48, "little") for c in _g2_flat(m, 2, g2.DST_RO))),
    "BLS12_381_G2_NU": (_native.blsg2_hash_to_field_batch, lambda m: b"".join(c.to_bytes(48, "little") for c in _g2_flat(m, 1, g2.DST_NU))),
    "Ed448_RO": (_native.ed448_hash_to_field_batch, lambda m: b"".join(u.to_bytes(56, "little") for u in e448.hash_to_field(m, 2, e448.DST_RO))),
    "Ed448_NU": (_native.ed448_hash_to_field_batch, lambda m: b"".join(u.to_bytes(56, "little") for u in e448.hash_to_field(m, 1, e448.DST_NU))),
}
MSGS = [b"", b"a", bytes(range(63)), bytes(64), bytes(range(136)), b"x" * 300]
SALTS = [b"", b"s", b"", bytes(range(40)), b"\x00", b"salt"]


@pytest.mark.parametrize("name", VARIANTS)
def test_hash_to_field_pairs_of_every_variant(name):
    pt = getattr(d, name).point_type
    per_item = 1 if name.endswith("_NU") else 2
    assert pt._per_item() == per_item
    elem = ELEM_BYTES.get(name[:-3], 32)
    salted = pt.hash_to_field_pairs(MSGS, SALTS)
    assert len(salted) == per_item * elem * len(MSGS)
    assert salted == pt.hash_to_field_pairs([s + m for m, s in zip(MSGS, SALTS)])
    assert len(pt.hash_to_field_pairs(MSGS)) == per_item * elem * len(MSGS) and pt.hash_to_field_pairs([]) == b""


@pytest.mark.parametrize("name", sorted(WIDE))
def test_wide_variants_agree_with_binding_and_restatement(name):
    binding, restated = WIDE[name]
    cv = getattr(d, name)
    joined = [s + m for m, s in zip(MSGS, SALTS)]
    want = b"".join(restated(m) for m in joined)
    assert cv.point_type.hash_to_field_pairs(MSGS, SALTS) == want
    assert binding(cv.curve.params.curve_id, joined) == want
