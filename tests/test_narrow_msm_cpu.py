"""CPU: the host side of the bucket method under dr_te_msm (Ed25519, Baby JubJub, P-256, secp256k1, Curve25519) and dr_blsg1_msm
(E(Fq)) from the library's own headers, compiled for the host under the undefined-behaviour sanitizer
(tests/native/narrow_msm_host_check.cpp): the plan over 252 / 254 / 257 tiled bits, the digits of scalars reduced as native_msm reduces
them, the two host laws over drh::Mod256 and the E(Fq) law (csrc/narrow_law.hpp) against the big-integer restatements, Curve25519's
conversion of the result, dr::wide_combine over these laws, and the bucket histograms of every family of narrow_msm_cases.py — so what
test_gpu_narrow_msm.py runs on the GPU is proved here to sit on both sides of the hand-over between the two accumulate kernels, to make
one heavy list per non-zero digit and index group, and (the ladder inputs) to make no list of 64 or more."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import curve25519_ref  # noqa: E402
import ed25519_ref  # noqa: E402
import narrow_msm_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BITS = (252, 254, 257)


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("narrow_msm") / "narrow_msm_host_check"
    subprocess.run(["g++", "-O2", "-std=c++20", "-fsanitize=undefined", "-fno-sanitize-recover", "-Wno-psabi", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "narrow_msm_host_check.cpp"), "-o", str(out)], check=True)
    return str(out)


def _histograms(exe, path, rows):
    """rows: (name, suite, n of the plan, scalars), possibly an iterator -> {name: dict}; the cases go through the program's standard input
    and path takes what it prints"""
    names = []
    with open(path, "w") as printed:
        proc = subprocess.Popen([exe, "hist", "-"], stdin=subprocess.PIPE, stdout=printed, stderr=printed, text=True)
        for name, suite, n, ks in rows:
            names.append(name)
            proc.stdin.write(f"case {name} {suite} {n} {len(ks)}\n")
            proc.stdin.write(f"{ks[0]:x}*{len(ks)}\n" if len(set(ks)) == 1 else "\n".join(map("%x".__mod__, ks)) + "\n")
        proc.stdin.close()
        code = proc.wait()
    with open(path) as printed:
        stdout = printed.read()
    assert code == 0, stdout[-2000:]
    out, cur = {}, None
    for line in stdout.splitlines():
        word = line.split()
        if word[0] == "case":
            cur = {k: int(v) for k, v in (item.split("=") for item in word[2:])}
            cur["lists"] = []
            out[word[1]] = cur
        elif word[0] == "list":
            cur["lists"].append(tuple(int(x) for x in word[1:]))                # (window, group, bucket, length, negative entries)
    assert list(out) == names
    return out


def test_plan_invariants_and_pinned_sizes(exe):
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert "narrow msm plan ok" in proc.stdout and f"from {cases.FROM}," in proc.stdout and f"heavy from {cases.HEAVY + 1}" in proc.stdout
    from dot_ring_amd import _native

    assert _native.NARROW_PIP_FROM == cases.FROM >= 257             # where Bls12381G1Point.msm hands over to dr_blsg1_msm
    assert {s.bits for s in cases.SUITES.values()} == set(BITS)
    # one bit more than a scalar can have: reduced below the order, or (E(Fq)) any 256-bit value
    assert all(s.bits == (s.order.bit_length() if s.reduce else 256) + 1 for s in cases.SUITES.values())
    for n, (c, widths, H, groups, _) in cases.PLANS.items():
        for bits, W in zip(BITS, widths):
            t = cases.Tiling(n, bits)
            assert (t.c, t.W, t.H, t.groups, t.cmax) == (c, W, H, groups, c)
        assert n == cases.FROM or n % groups


@pytest.mark.parametrize("name", cases.NAMES)
def test_digits_sum_back_to_the_reduced_scalar(exe, tmp_path, name):
    """0, 1, the order and its neighbours, 2^256 - 1, all-7 and all-8 nibbles and 200 seeded values under the tilings of every window
    width 7 - 10: the program's digits sum back to what the host path uploads (k mod n; on E(Fq) k itself), and so do the restatement's"""
    s = cases.SUITES[name]
    rng = cases._rng(name, "digits")
    ks = cases.edge_scalars(s) + [rng.getrandbits(256) for _ in range(200)]
    assert {0, 1, s.order - 1, s.order, s.order + 1, (1 << 256) - 1, int("7" * 64, 16), int("8" * 64, 16)} <= set(ks)
    sizes = (cases.FROM, 4103, 16387, 65539)
    h = _histograms(exe, tmp_path / "digits.txt", [(f"digits-{n}", name, n, ks) for n in sizes])
    for n, c in zip(sizes, (7, 8, 9, 10)):
        t = cases.Tiling(n, s.bits)
        got = h[f"digits-{n}"]
        assert (got["c"], got["W"], got["H"], got["groups"], got["cmax"]) == (c, t.W, t.H, t.groups, c) and got["reconstruct_bad"] == 0
        for k in ks:
            ds = cases.digits(s.red(k), t)
            assert sum(d << st for d, st in zip(ds, t.starts)) == s.red(k) and all(abs(d) <= 1 << (w - 1) for d, w in zip(ds, t.widths))
    assert s.reduce == (name != "blsg1") and s.red(s.order + 1) == (1 if s.reduce else s.order + 1)


def test_malformed_input_is_refused(exe, tmp_path):
    """the checker itself: a scalar of more than 256 bits and a suite it does not know end the program with status 2"""
    path = tmp_path / "bad.txt"
    path.write_text("case wide blsg1 300 1\n1%s\n" % ("0" * 64))
    assert subprocess.run([exe, "hist", str(path)], capture_output=True, text=True).returncode == 2
    path.write_text("case nosuite p384 300 1\n1\n")
    assert subprocess.run([exe, "hist", str(path)], capture_output=True, text=True).returncode == 2


# ---------------------------------------------------------------- the host laws
def _law_points(name):
    """(points of the law's input form, the restatement they live in, its identity)"""
    s = cases.SUITES[name]
    ref = ed25519_ref if name == "curve25519" else s.ref
    o = (0, 1) if name == "curve25519" else s.o
    lad = [curve25519_ref.to_edwards(p) for p in cases.ladder(name)[:12]] if name == "curve25519" else cases.ladder(name)[:12]
    extra = []
    if name in ("ed25519", "bjj", "curve25519"):
        extra = ref.torsion_points()                                     # the 8-torsion: (0, 1), (0, -1) among them (x = 0)
        assert (0, 1) in extra and (0, ref.P - 1) in extra and len(set(extra)) == 8
    elif name == "blsg1":
        extra = [(0, 2), (0, ref.P - 2), s.special]                         # the x = 0 points (order 3) and a point outside G1
        assert ref.on_curve((0, 2)) and ref.mul(3, (0, 2)) is None and ref.mul(ref.R_ORDER, s.special) is not None
    elif name == "p256":
        y = ref.sqrt(ref.B)
        assert y is not None and y * y % ref.P == ref.B                  # P-256 has the points (0, +-sqrt(b))
        extra = [(0, y), (0, ref.P - y)]
    else:
        assert pow(7, (s.ref.P - 1) // 2, s.ref.P) != 1                  # secp256k1 has no point with x = 0: 7 is no square
    return lad, extra, ref, o


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_law_equals_the_restatement(exe, tmp_path, name):
    """random pairs, P + P, P + (-P), the identity on either side, the 8-torsion of Ed25519 and Baby JubJub, the x = 0 points where the
    curve has any, a point of E(Fq) outside G1 — and for Curve25519 the conversion of every result, (0, 0) and the identity among them"""
    s = cases.SUITES[name]
    lad, extra, ref, o = _law_points(name)
    if name == "curve25519":
        raw_in = lambda pt: ed25519_ref.raw(pt)
        raw_out = lambda pt: s.raw(curve25519_ref.from_edwards(pt))
    else:
        raw_in = raw_out = s.raw
    rng = cases._rng(name, "law")
    pairs = [(rng.choice(lad), rng.choice(lad)) for _ in range(20)]
    pairs += [(p, p) for p in lad[:3]] + [(p, ref.neg(p)) for p in lad[:3]] + [(o, lad[0]), (lad[0], o), (o, o)]
    pairs += [(a, b) for a in extra for b in extra] + [(a, lad[1]) for a in extra] + [(lad[2], a) for a in extra]
    path = tmp_path / "law.txt"
    path.write_text("".join(f"{name} {raw_in(a).hex()} {raw_in(b).hex()}\n" for a, b in pairs))
    proc = subprocess.run([exe, "law", str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    got = [line.split() for line in proc.stdout.splitlines()]
    want = []
    for a, b in pairs:
        sm, db = ref.add(a, b), ref.add(a, a)
        want.append([raw_out(sm).hex(), raw_out(db).hex(), raw_out(ref.add(sm, db)).hex()])
    assert got == want
    seen = {w for row in want for w in row}
    assert s.identity.hex() in seen
    if name == "curve25519":
        assert bytes(64).hex() in seen and (b"\xff" * 64).hex() in seen      # (0, -1) -> (0, 0), the identity -> 64 bytes of 0xff


@pytest.mark.parametrize("name", cases.NAMES)
def test_host_combine_equals_the_restatement(exe, tmp_path, name):
    """set sums m G (ladder points, some negated, some the identity) for the plans of the threshold size, 16387 and 65539 terms: the
    program's combination is (sum_w 2^start_w sum_g m_wg mod n) G"""
    s = cases.SUITES[name]
    ref, lad = s.ref, cases.ladder(name)
    if name == "curve25519":
        raw_in = lambda pt: ed25519_ref.raw(curve25519_ref.to_edwards(pt))
    else:
        raw_in = s.raw
    rng = cases._rng(name, "combine")
    blocks, want = [], []
    for n in (cases.FROM, 16387, 65539, "identity"):
        t = cases.Tiling(cases.FROM if n == "identity" else n, s.bits)
        total, lines = 0, []
        for w in range(t.W):
            for g in range(t.groups):
                kind = "id" if n == "identity" else rng.choice(["m", "m", "m", "neg", "id"])
                i = rng.randrange(len(lad))
                pt = None if kind == "id" else lad[i] if kind == "m" else ref.neg(lad[i])
                total += (0 if kind == "id" else (cases.LADDER_A + i) * (1 if kind == "m" else -1)) << t.starts[w]
                lines.append(raw_in(pt).hex())
        blocks.append(f"sums {name} {cases.FROM if n == 'identity' else n}\n" + "\n".join(lines) + "\n")
        want.append(s.raw(ref.mul(total % s.order, ref.G) if total % s.order else None).hex())
    path = tmp_path / "sums.txt"
    path.write_text("".join(blocks))
    proc = subprocess.run([exe, "combine", str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert proc.stdout.split() == want and want[-1] == s.identity.hex()


# ---------------------------------------------------------------- the families' bucket lists
@pytest.fixture(scope="module")
def hist(exe, tmp_path_factory):
    """name -> the histograms of every case on that suite, made at the first call for all six suites, one program each at the same time;
    the cases are built one at a time and dropped"""
    done = {}
    printed = tmp_path_factory.mktemp("narrow_msm_hist")

    def one(name):
        built = (cases.build(name, family, n) for n in cases.PLANS for family in cases.plan_families(n))
        return _histograms(exe, printed / f"{name}.txt", ((c.name, name, c.n, c.scalars) for c in built))

    def of(name):
        if not done:
            with ThreadPoolExecutor(len(cases.NAMES)) as pool:
                done.update(zip(cases.NAMES, pool.map(one, cases.NAMES)))
        return done[name]

    return of


@pytest.mark.parametrize("n", tuple(cases.PLANS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_plans_and_ladder_lists(hist, name, n):
    """the pinned plan; every family's digits sum back; the ladder scalars make NO list of 64 or more — a condition on the seeded inputs,
    so that their GPU runs are the per-lane walk alone"""
    s = cases.SUITES[name]
    c, widths, H, groups, _ = cases.PLANS[n]
    W = widths[BITS.index(s.bits)]
    for family in cases.plan_families(n):
        h = hist(name)[f"{name}-{family}-{n}"]
        assert (h["n"], h["c"], h["W"], h["H"], h["groups"], h["cmax"]) == (n, c, W, H, groups, c) and h["reconstruct_bad"] == 0
        assert h["heavy"] == sum(1 for x in h["lists"] if x[3] > cases.HEAVY)
    lad = hist(name)[f"{name}-ladder-{n}"]
    assert lad["heavy"] == 0 and lad["longest"] < cases.HEAVY and lad["lists"] == []


EQUAL_LENGTHS = {cases.FROM: [cases.FROM], 1031: [515, 516], 4103: [1025, 1026], 16387: [2048, 2049], 65539: [4096, 4097]}


@pytest.mark.parametrize("n", tuple(cases.PLANS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_equal_has_one_heavy_list_per_digit_and_group(hist, name, n):
    case, h = cases.build(name, "equal", n), hist(name)[f"{name}-equal-{n}"]
    t = cases.Tiling(n, cases.SUITES[name].bits)
    ds = cases.digits(case.scalars[0], t)
    nonzero = sum(1 for d in ds if d)
    assert len(set(case.scalars)) == 1 and case.scalars[0] < cases.SUITES[name].order
    assert h["heavy"] == nonzero * t.groups == len(h["lists"]) and nonzero >= t.W - 8
    assert sorted((x[0], x[1]) for x in h["lists"]) == [(w, g) for w in range(t.W) if ds[w] for g in range(t.groups)]
    assert all(x[2] == abs(ds[x[0]]) - 1 and x[4] == (x[3] if ds[x[0]] < 0 else 0) for x in h["lists"])
    assert sorted({x[3] for x in h["lists"]}) == case.claims["lengths"] == EQUAL_LENGTHS[n] and min(EQUAL_LENGTHS[n]) > cases.HEAVY


@pytest.mark.parametrize("n", tuple(n for n in cases.PLANS if "lengths" in cases.plan_families(n)))
@pytest.mark.parametrize("name", cases.NAMES)
def test_lengths_and_cancelling_pairs(hist, name, n):
    """lists of exactly 64 and 65 in window 0 of index group 0; an odd number of terms that still sum to the identity, in the curve's
    own spelling; the edges' special terms"""
    s = cases.SUITES[name]
    h = hist(name)[f"{name}-lengths-{n}"]
    assert [x for x in h["lists"] if x[0] == 0 and x[2] < 2] == [(0, 0, 0, 64, 0), (0, 0, 1, 65, 0)]
    assert h["heavy"] >= h["W"] - 1
    ident = cases.build(name, "cancel-identity", n)
    assert n % 2 == 1 and ident.terms[-1][:2] == ("id", 0)
    assert all(a[0] == "m" and b[0] == "neg" and a[1:] == b[1:] for a, b in zip(ident.terms[:-1:2], ident.terms[1:-1:2]))
    assert ident.expected() == s.identity and any(x[3] >= 80 for x in hist(name)[ident.name]["lists"])
    assert s.identity == {"ed25519": bytes(32) + b"\x01" + bytes(31), "bjj": bytes(32) + b"\x01" + bytes(31), "p256": bytes(64),
                          "secp256k1": bytes(64), "curve25519": b"\xff" * 64, "blsg1": bytes(96)}[name]
    mixed = hist(name)[f"{name}-cancel-mixed-{n}"]
    assert any(x[3] >= 130 for x in mixed["lists"]) and any(100 <= x[3] < 130 for x in mixed["lists"])
    edges = cases.build(name, "edges", n)
    assert edges.scalars[:8] == [0, 1, s.order - 1, s.order, s.order + 1, (1 << 256) - 1, int("7" * 64, 16), int("8" * 64, 16)]
    assert sum(1 for t in edges.terms if t[0] == "id") == 5 and edges.terms[-1][2] == (1 << 256) - 1
    special = [t[2] for t in edges.terms if t[0] == "special"]
    if name in ("ed25519", "bjj", "curve25519"):
        q = s.special if name != "curve25519" else curve25519_ref.to_edwards(s.special)
        ref = ed25519_ref if name == "curve25519" else s.ref
        assert ref.mul(8, q) == (0, 1) != ref.mul(4, q) and len(special) == 5 and all(k >= s.order for k in special)
        assert sum(k % s.order for k in special) % 8 not in (0, sum(special) % 8)
    elif name == "blsg1":
        assert len(special) == 5 and all(k >= s.order for k in special) and s.ref.mul(s.order, s.special) is not None
    else:
        assert not special
