"""CPU: the descent that turns tests of subset sums into a verdict per proof (dot_ring_amd/csrc/verify_tree.hpp, behind
dr_ringvrf_verify_each), driven with stub predicates by tests/native/verify_tree_check.cpp (host compiler, -fsanitize=undefined
-fno-sanitize-recover), and RingVRF.verify_each's fallback route, the same descent in Python over a stub batch_verify.

B in {1, 2, 3, 5, 64, 65, 130, 4096}; for B <= 5 every subset of bad leaves, for the larger B none, one at each end, one at 63 and
at 64, an adjacent pair, every other leaf, and all.  The verdicts equal the bad set; one test when nothing is bad; at most
1 + 2 k ceil(log2 B') tests for k bad leaves (B' the padded size: a failed parent costs at most two tests on the level below and
there are at most k failed parents per level); a node is asked only under a failed parent; padding is never tested."""
import itertools
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

SIZES = [1, 2, 3, 5, 64, 65, 130, 4096]


def _cases():
    out = []
    for b in SIZES:
        if b <= 5:
            for k in range(b + 1):
                out += [(b, list(c)) for c in itertools.combinations(range(b), k)]
            continue
        sets = [[], [0], [b - 1], [63], [64], [b // 2 - 1, b // 2], [63, 64], list(range(0, b, 2)), list(range(1, b, 2)), list(range(b))]
        out += [(b, [i for i in s if i < b]) for s in sets]
    return out


CASES = _cases()


def _padded(b):
    p = 1
    while p < b:
        p *= 2
    return p


def _bound(b, k):
    return 1 if k == 0 else 1 + 2 * k * (_padded(b).bit_length() - 1)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = tmp_path_factory.mktemp("verify_tree") / "verify_tree_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "verify_tree_check.cpp"), "-o", str(path)], check=True)
    return str(path)


def test_native_descent_finds_exactly_the_bad_leaves(exe):
    text = "".join(f"{b} {len(bad)} {' '.join(map(str, bad))}\n" for b, bad in CASES)
    proc = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    rows = proc.stdout.splitlines()
    assert len(rows) == len(CASES)
    for (b, bad), row in zip(CASES, rows):
        tested, padding_tested, orphan, widest, padded, depth, bits = row.split()
        want = "".join("0" if i in set(bad) else "1" for i in range(b))
        assert bits == want, (b, bad)
        assert int(padded) == _padded(b) and int(depth) == _padded(b).bit_length() - 1
        assert int(tested) <= _bound(b, len(bad)), (b, bad, tested)
        if not bad:
            assert int(tested) == 1
        assert int(padding_tested) == 0 and int(orphan) == 0, (b, bad, row)
        if b == 4096 and len(bad) == 2048:
            assert int(widest) >= 1024          # the tests of one level are handed over together


def test_python_descent_over_a_stub_batch_verify():
    from dot_ring_amd.vrf.ring_vrf import verify_tree_descent

    for b, bad in CASES:
        bad_set, calls = set(bad), []

        def batch_verify(lo, hi):
            assert 0 <= lo < hi <= b            # never a span of padding alone
            calls.append((lo, hi))
            return not any(lo <= i < hi for i in bad_set)

        verdicts, tests = verify_tree_descent(b, batch_verify)
        assert verdicts == [i not in bad_set for i in range(b)], (b, bad)
        assert tests == len(calls) <= _bound(b, len(bad)), (b, bad, tests)
        if not bad:
            assert tests == 1
        assert len(set(calls)) == len(calls)    # no span is asked twice
    assert verify_tree_descent(0, lambda lo, hi: True) == ([], 0)


def test_verify_each_is_declared_everywhere():
    from dot_ring_amd import _native

    with open(os.path.join(ROOT, "include", "dotring_hip.h")) as f:
        header = f.read()
    for name in ("dr_ringvrf_verify_each", "dr_ringvrf_verify_each_multi", "dr_g1_claim_tree_selftest"):
        assert name + "(" in header and name in _native.EXPORTED_SYMBOLS and hasattr(_native.lib(), name)
    import dot_ring_amd as d

    assert callable(d.RingVRF[d.Bandersnatch].verify_each)
    with pytest.raises(ValueError):
        d.RingVRF[d.Bandersnatch].verify_each([], [b""], [], None, None)
