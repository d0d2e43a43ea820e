"""GPU: RingVRF.verify_each (dr_ringvrf_verify_each) — a verdict per proof from one batch pass — against the existing verifiers.

Ring domain 512 on Bandersnatch, one JubJub case at 512 and one Bandersnatch case at 1024; proofs from prove_batch.
  (a) all valid at B in {1, 3, 8, 9, 64, 65, 130}: all True, ONE pairing equation, batch_verify agrees;
  (b) one kind of damage at a time at chosen positions, B = 65 and B = 9 (the kernel route and the host route): the verdicts equal
      [p.verify(...)] of the existing single verifier, the false set is exactly the damaged set, batch_verify on the list is False
      and on the list without the false ones True;
  (c) one bad proof among 64 costs at most 13 pairing equations;
  (d) the Python bisection route (DOTRING_NATIVE_HOST=0, a child process) gives the same lists at B = 9;
  (e) a device set (DOTRING_DEVICES=0,0) at B = 37 with three bad proofs gives the same list;
  (f) unequal lengths raise, a mismatched root gives all False, an object with a bad field is False for itself alone."""
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FR = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001        # BLS12-381 scalar field = Bandersnatch base field
MAX_B = 130
KINDS = ["input", "ad", "eval", "s_b", "swap_openings", "noncanonical", "g1_undecodable", "te_off_curve", "te_off_subgroup", "g1_infinity",
         "other_ring"]


class Blob:                          # anything with encode(): the native verifiers only read the bytes
    def __init__(self, b):
        self._b = b

    def encode(self):
        return self._b


def _setup(cv_name="Bandersnatch", ring_size=9, count=MAX_B, tag=b""):
    import dot_ring_amd as d

    cv = getattr(d, cv_name)
    vrf = d.RingVRF[cv]
    sks = [(9000 + i).to_bytes(32, "little") for i in range(min(ring_size, 16))]
    keys = [cv.public_key_from_secret(sk) for sk in sks]
    from dot_ring_amd.curve import scalar_mul_batch
    if ring_size > len(sks):        # fill a large ring with further members nobody proves for
        more = [(20000 + i) for i in range(ring_size - len(sks))]
        keys += [p.point_to_string() for p in scalar_mul_batch([cv.point_type.generator_point()] * len(more), more)]
    params = d.RingProofParams.from_ring_size(ring_size, test_vectors=True, cv=cv)
    ring = d.Ring(keys, params)
    root = d.RingRoot.from_ring(ring, params)
    als = [tag + b"in%d" % i for i in range(count)]
    ads = [b"ad%d" % (i % 3) for i in range(count)]
    who = [i % len(sks) for i in range(count)]
    proofs = vrf.prove_batch(als, ads, [sks[w] for w in who], [keys[w] for w in who], ring, root)
    return d, cv, vrf, keys, params, ring, root, als, ads, [p.encode() for p in proofs]


@pytest.fixture(scope="module")
def world(ctx):
    d, cv, vrf, keys, params, ring, root, als, ads, raw = _setup()
    assert params.domain_size == 512
    # the same members in another order: another root; its proofs do not hold under `root`
    other = d.Ring(keys[::-1], params)
    other_root = d.RingRoot.from_ring(other, params)
    sks = [(9000 + i).to_bytes(32, "little") for i in range(9)]
    who = [i % 9 for i in range(MAX_B)]
    foreign = [p.encode() for p in vrf.prove_batch(als, ads, [sks[w] for w in who], [keys[w] for w in who], other, other_root)]
    # Bandersnatch strings: a y with no x on the curve, and a curve point outside the prime-order subgroup
    from oracle.pyref import bandersnatch as obsn
    off_curve = off_subgroup = None
    y = 2
    while off_curve is None or off_subgroup is None:
        enc = y.to_bytes(32, "little")
        try:
            if not obsn.in_prime_subgroup(obsn.decompress(enc)) and off_subgroup is None:
                off_subgroup = enc
        except ValueError:
            if off_curve is None:
                off_curve = enc
        y += 1
    memo = {}

    def single(blob, inp, ad):
        """the existing single verifier: decode, then RingVRF.verify"""
        key = (blob, inp, ad)
        if key not in memo:
            try:
                obj = vrf.decode(blob)
            except ValueError:
                memo[key] = False
            else:
                memo[key] = bool(obj.verify(inp, ad, ring, root))
        return memo[key]

    return dict(d=d, vrf=vrf, ring=ring, root=root, als=als, ads=ads, raw=raw, foreign=foreign, off_curve=off_curve,
                off_subgroup=off_subgroup, single=single, other=other, other_root=other_root, order=cv.curve.params.subgroup_order)


def _each(w, blobs, als, ads, ring=None, root=None):
    stats = {}
    got = w["vrf"].verify_each([Blob(b) for b in blobs], als, ads, ring or w["ring"], root or w["root"], stats=stats)
    return got, stats


def _batch(w, blobs, als, ads):
    return w["vrf"].batch_verify([Blob(b) for b in blobs], als, ads, w["ring"], w["root"])


@pytest.mark.parametrize("count", [1, 3, 8, 9, 64, 65, 130])
def test_all_valid_costs_one_equation(world, count):
    w = world
    blobs, als, ads = w["raw"][:count], w["als"][:count], w["ads"][:count]
    got, stats = _each(w, blobs, als, ads)
    assert got == [True] * count
    assert stats["pairings"] == 1 and stats["excluded"] == 0 and stats["depth"] == (count - 1).bit_length()
    assert _batch(w, blobs, als, ads)


def _damage(w, kind, blobs, als, ads, where):
    """apply `kind` at the positions `where`; returns the damaged set (the openings swap needs a partner)"""
    count = len(blobs)
    le = lambda v: v.to_bytes(32, "little")
    put = lambda b, off, new: b[:off] + new + b[off + len(new):]
    if kind == "swap_openings":
        where = sorted(set(where) | ({(where[0] + 1) % count} if len(where) == 1 else set()))
        opens = [blobs[i][688:784] for i in where]
        for k, i in enumerate(where):                       # each takes the next one's two opening proofs: valid points, wrong claims
            blobs[i] = put(blobs[i], 688, opens[(k + 1) % len(where)])
        return set(where)
    for i in where:
        b = blobs[i]
        if kind == "input":
            als[i] = als[i] + b"!"
        elif kind == "ad":
            ads[i] = ads[i] + b"!"
        elif kind == "eval":                                # px(zeta) -> another canonical value: the ring part fails alone
            blobs[i] = put(b, 384, le((int.from_bytes(b[384:416], "little") + 1) % FR))
        elif kind == "s_b":                                 # the Pedersen part fails alone
            blobs[i] = put(b, 160, le((int.from_bytes(b[160:192], "little") + 1) % w["order"]))
        elif kind == "noncanonical":                        # s + n, or an evaluation + p: the same residue, not canonical
            if i % 2 == 0:
                blobs[i] = put(b, 128, le(int.from_bytes(b[128:160], "little") + w["order"]))
            else:
                blobs[i] = put(b, 416, le(int.from_bytes(b[416:448], "little") + FR))
        elif kind == "g1_undecodable":
            blobs[i] = put(b, 192, bytes([0x9F]) + b"\xff" * 47)
        elif kind == "te_off_curve":
            blobs[i] = put(b, 64, w["off_curve"])
        elif kind == "te_off_subgroup":
            blobs[i] = put(b, 32, w["off_subgroup"])
        elif kind == "g1_infinity":
            blobs[i] = put(b, 288, bytes([0xC0]) + bytes(47))
        elif kind == "other_ring":
            blobs[i] = w["foreign"][i]
        else:
            raise AssertionError(kind)
    return set(where)


def _position_sets(count):
    sets = [[0], [count - 1], [63], [64], [count // 2 - 1, count // 2] if count < 64 else [63, 64], list(range(0, count, 2)), list(range(count))]
    out = []
    for s in sets:
        s = [i for i in s if i < count]
        if s and s not in out:
            out.append(s)
    return out


@pytest.mark.parametrize("count", [65, 9])
@pytest.mark.parametrize("kind", KINDS)
def test_damaged_proofs_are_the_false_ones(world, kind, count):
    w = world
    for where in _position_sets(count):
        blobs, als, ads = list(w["raw"][:count]), list(w["als"][:count]), list(w["ads"][:count])
        damaged = _damage(w, kind, blobs, als, ads, where)
        got, stats = _each(w, blobs, als, ads)
        want = [w["single"](b, a, x) for b, a, x in zip(blobs, als, ads)]
        assert got == want, (kind, where, [i for i in range(count) if got[i] != want[i]])
        assert {i for i in range(count) if not got[i]} == damaged, (kind, where)
        assert not _batch(w, blobs, als, ads), (kind, where)
        keep = [i for i in range(count) if got[i]]
        assert _batch(w, [blobs[i] for i in keep], [als[i] for i in keep], [ads[i] for i in keep]), (kind, where)
        assert stats["pairings"] <= 1 + 2 * len(damaged) * stats["depth"], (kind, where, stats)
        if kind in ("noncanonical", "g1_undecodable", "te_off_curve", "te_off_subgroup"):
            assert stats["excluded"] == len(damaged) and stats["pairings"] == 1, (kind, where, stats)


def test_one_bad_proof_among_64_costs_at_most_13_equations(world):
    w = world
    for pos in (0, 37, 63):
        blobs, als, ads = list(w["raw"][:64]), list(w["als"][:64]), list(w["ads"][:64])
        _damage(w, "eval", blobs, als, ads, [pos])
        got, stats = _each(w, blobs, als, ads)
        assert got == [i != pos for i in range(64)]
        assert stats["pairings"] <= 13 and stats["depth"] == 6, stats


def test_identical_neighbours_and_repeated_proofs(world):
    """two identical proofs side by side (equal leaves: the doubling inside the tree), once valid and once both damaged alike"""
    w = world
    blobs, als, ads = list(w["raw"][:12]), list(w["als"][:12]), list(w["ads"][:12])
    for lst in (blobs, als, ads):
        lst[5] = lst[4]
    assert _each(w, blobs, als, ads)[0] == [True] * 12
    _damage(w, "eval", blobs, als, ads, [4])
    blobs[5] = blobs[4]
    assert _each(w, blobs, als, ads)[0] == [i not in (4, 5) for i in range(12)]


@pytest.mark.parametrize("cv_name,ring_size,domain", [("JubJub", 9, 512), ("Bandersnatch", 300, 1024)])
def test_other_curve_and_domain(ctx, cv_name, ring_size, domain):
    d, cv, vrf, keys, params, ring, root, als, ads, raw = _setup(cv_name, ring_size, 11, b"o")
    assert params.domain_size == domain
    got = vrf.verify_each([Blob(b) for b in raw], als, ads, ring, root)
    assert got == [True] * 11 and vrf.batch_verify([Blob(b) for b in raw], als, ads, ring, root)
    als[7] += b"?"
    b = raw[2]
    raw[2] = b[:384] + ((int.from_bytes(b[384:416], "little") + 1) % FR).to_bytes(32, "little") + b[416:]
    stats = {}
    got = vrf.verify_each([Blob(b) for b in raw], als, ads, ring, root, stats=stats)
    assert got == [i not in (2, 7) for i in range(11)]
    assert got == [vrf.decode(b).verify(a, x, ring, root) for b, a, x in zip(raw, als, ads)]
    assert stats["pairings"] > 1 and not vrf.batch_verify([Blob(b) for b in raw], als, ads, ring, root)


_CHILD = r"""
import sys
sys.path.insert(0, {tests!r})
import test_gpu_ring_verify_each as t
d, cv, vrf, keys, params, ring, root, als, ads, raw = t._setup(count={count})
w = dict(order=cv.curve.params.subgroup_order)
from dot_ring_amd import runtime
print("ROUTE", int(vrf._native_verifier_serves(ring, root)), len(runtime.device_contexts()))
out, seen = [], []
for kind, where in {cases!r}:
    blobs, a, x = list(raw), list(als), list(ads)
    t._damage(w, kind, blobs, a, x, where)
    objs = []
    for blob in blobs:                  # the Python route reads the proofs' fields: objects where the bytes decode at all
        try:
            objs.append(vrf.decode(blob))
        except ValueError:
            objs.append(t.Blob(blob))
    stats = {{}}
    out.append("".join("1" if v else "0" for v in vrf.verify_each(objs, a, x, ring, root, stats=stats)))
    seen.append("%d,%d,%d" % (stats["pairings"], stats["excluded"], stats["depth"]))
print("VERDICTS", " ".join(out))
print("STATS", " ".join(seen))
"""


def _child(count, cases, extra_env):
    env = {k: v for k, v in os.environ.items() if not k.startswith("DOTRING_")}
    env.update(extra_env)
    env["PYTHONPATH"] = ROOT + os.pathsep + env.get("PYTHONPATH", "")
    script = _CHILD.format(tests=os.path.join(ROOT, "tests"), count=count, cases=cases)
    out = subprocess.run([sys.executable, "-c", script], cwd=ROOT, env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    line = lambda tag: [ln.split()[1:] for ln in out.stdout.splitlines() if ln.startswith(tag)][0]
    native, contexts = (int(v) for v in line("ROUTE"))
    return line("VERDICTS"), bool(native), contexts, [tuple(int(v) for v in s.split(",")) for s in line("STATS")]


def _here(world, count, cases):
    out = []
    for kind, where in cases:
        blobs, als, ads = list(world["raw"][:count]), list(world["als"][:count]), list(world["ads"][:count])
        _damage(world, kind, blobs, als, ads, where)
        out.append("".join("1" if v else "0" for v in _each(world, blobs, als, ads)[0]))
    return out


def test_python_bisection_route_gives_the_same_lists(world):
    cases = [("input", []), ("input", [0]), ("eval", [8]), ("s_b", [3, 4]), ("swap_openings", [2]), ("noncanonical", [1, 6]),
             ("g1_infinity", [0, 2, 4, 6, 8]), ("ad", list(range(9)))]
    here = _here(world, 9, cases)
    assert here[0] == "1" * 9 and here[2] == "1" * 8 + "0" and here[4] == "1100" + "1" * 5 and here[7] == "0" * 9
    got, native, contexts, stats = _child(9, cases, {"DOTRING_NATIVE_HOST": "0"})
    assert got == here
    # ... and it was the bisection that ran: the native verifier does not serve, nothing is excluded before a fold (the native route
    # excludes the two non-canonical proofs and then needs one equation), and the count is the descent's over batch_verify
    from dot_ring_amd.vrf.ring_vrf import verify_tree_descent

    assert not native
    for verdicts, (tests, excluded, depth) in zip(here, stats):
        assert excluded == 0 and depth == 4
        assert tests == verify_tree_descent(9, lambda lo, hi: "0" not in verdicts[lo:hi])[1]
    assert stats[0][0] == 1 and stats[5][0] > 1


def test_device_set_gives_the_same_list(world):
    cases = [("eval", [1, 18, 36])]
    here = _here(world, 37, cases)
    assert here == ["".join("0" if i in (1, 18, 36) else "1" for i in range(37))]
    got, native, contexts, stats = _child(37, cases, {"DOTRING_DEVICES": "0,0"})
    assert got == here
    # ... and two shards judged it: two contexts, and the deepest tree is a shard's (19 proofs: depth 5), not the batch's (37: 6)
    assert native and contexts == 2 and stats[0][1] == 0 and stats[0][2] == 5
    assert _each(world, *[world[k][:37] for k in ("raw", "als", "ads")])[1]["depth"] == 6


def test_argument_handling(world):
    w = world
    vrf, ring, root = w["vrf"], w["ring"], w["root"]
    blobs, als, ads = w["raw"][:5], w["als"][:5], w["ads"][:5]
    with pytest.raises(ValueError):
        vrf.verify_each([Blob(b) for b in blobs], als[:4], ads, ring, root)
    with pytest.raises(ValueError):
        vrf.verify_each([Blob(b) for b in blobs], als, ads[:4], ring, root)
    assert vrf.verify_each([], [], [], ring, root) == []
    assert vrf.verify_each([Blob(b) for b in blobs], als, ads, w["other"], root) == [False] * 5
    assert vrf.verify_each([Blob(b) for b in blobs], als, ads, ring, w["other_root"]) == [False] * 5

    class Broken:
        def encode(self):
            raise ValueError("a field that does not encode")

    objs = [Blob(b) for b in blobs]
    objs[1] = Broken()
    objs[3] = Blob(blobs[3][:-1])
    stats = {}
    assert vrf.verify_each(objs, als, ads, ring, root, stats=stats) == [True, False, True, False, True]
    assert stats["excluded"] == 2 and stats["pairings"] == 1
    # the C entry points refuse what dr_ringvrf_verify_batch refuses
    import ctypes

    from dot_ring_amd import _native, runtime

    vk, suite = root.__dict__["_native_vk"], vrf._suite_struct()
    with pytest.raises(ValueError):
        runtime.context().ringvrf_verify_each(suite, vk, b"".join(w["raw"][:1]) * 4097, [b""] * 4097, [b""] * 4097, None, bytes(32))
    with pytest.raises(ValueError):
        _native.ringvrf_verify_each_multi([runtime.context(), runtime.context()], suite, vk, b"".join(blobs), als, ads, None, bytes(32))
    off = (ctypes.c_uint64 * 2)(0, 0)
    assert _native.lib().dr_ringvrf_verify_each(runtime.context().handle, ctypes.byref(suite), ctypes.byref(vk), 1, bytes(784), b"", off, b"", off,
                                                None, None, bytes(32), None, None) != 0
