"""CPU: the plan of the wide suites' bucket method (dr::plan_wide_msm, dot_ring_amd/csrc/msm_plan.hpp), its digits (dr::wide_digit,
wide_recode.hip.h) and the host's window combination (dr::wide_combine, wide_combine.hpp, over the laws of P-384, P-521, Ed448 and
Curve448), from the library's own headers compiled for the host under the undefined-behaviour sanitizer
(tests/native/wide_msm_plan_check.cpp).

The program checks the plan's invariants over a sweep of sizes and pins (c, W, H, groups) of every size the GPU tests use.  Then it runs
wide_digit per (window, index group) over the scalars of every family of wide_msm_cases.py, as wave_msm_sort walks them, and prints the
bucket histograms; the tests below assert on them what the families claim — so what test_gpu_wide_msm.py runs on the GPU is proved here
to enter the wave walk, to sit on both sides of the hand-over between the two accumulate kernels, to reach the last bucket of a
full-width window, and to have two index groups at 1030 terms.  The same for the upper half of the plan (wide_msm_cases.PLANS, run by
test_gpu_wide_msm_plans.py): widths 9 and 10, 8 to 64 index groups, group bounds with a remainder, a tiling of full-width windows only;
those cases go to the program through a pipe, one at a time.  Last, the program combines set sums with each of the four laws and the
result is checked against the big-integer restatements."""
import os
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import wide_msm_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("wide_msm_plan") / "wide_msm_plan_check"
    subprocess.run(["g++", "-O2", "-std=c++20", "-fsanitize=undefined", "-fno-sanitize-recover", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "wide_msm_plan_check.cpp"), "-o", str(out)], check=True)
    return str(out)


def _histograms(exe, path, rows, piped=False):
    """rows: (name, bits, scalar words, n of the plan, scalars) -> {name: dict}.  piped: rows may be an iterator and go through the
    program's standard input, a case of one scalar as one line (the large cases would make a file of hundreds of megabytes), and path
    takes what the program prints"""
    if piped:
        names = []
        with open(path, "w") as printed:
            proc = subprocess.Popen([exe, "hist", "-"], stdin=subprocess.PIPE, stdout=printed, stderr=printed, text=True)
            for name, bits, words, n, ks in rows:
                names.append(name)
                proc.stdin.write(f"case {name} {bits} {words} {n} {len(ks)}\n")
                proc.stdin.write(f"{ks[0]:x}*{len(ks)}\n" if len(set(ks)) == 1 else "\n".join(map("%x".__mod__, ks)) + "\n")
            proc.stdin.close()
            code = proc.wait()
        with open(path) as printed:
            stdout = printed.read()
        assert code == 0, stdout[-2000:]
    else:
        rows = list(rows)
        names = [row[0] for row in rows]
        with open(path, "w") as f:
            for name, bits, words, n, ks in rows:
                f.write(f"case {name} {bits} {words} {n} {len(ks)}\n")
                f.write("\n".join("%x" % k for k in ks) + "\n")
        proc = subprocess.run([exe, "hist", str(path)], capture_output=True, text=True)
        assert proc.returncode == 0, proc.stderr
        stdout = proc.stdout
    out, cur = {}, None
    for line in stdout.splitlines():
        word = line.split()
        if word[0] == "case":
            cur = {k: int(v) for k, v in (item.split("=") for item in word[2:])}
            cur["lists"] = []
            out[word[1]] = cur
        elif word[0] == "top":
            cur["top"] = [int(x) for x in word[1:]]
        elif word[0] == "list":
            cur["lists"].append(tuple(int(x) for x in word[1:]))                # (window, group, bucket, length, negative entries)
    assert list(out) == names
    return out


@pytest.fixture(scope="module")
def hist(exe, tmp_path_factory):
    rows = [(c.name, cases.SUITES[c.suite].bits, cases.SUITES[c.suite].words, c.n, c.scalars) for c in cases.all_cases()]
    return _histograms(exe, tmp_path_factory.mktemp("wide_msm_hist") / "families.txt", rows)


def test_plan_invariants_and_pinned_sizes(exe):
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert "wide msm plan ok" in proc.stdout and f"heavy from {cases.HEAVY + 1}" in proc.stdout
    assert cases.FROM == 256 and cases.HEAVY == 64
    from dot_ring_amd import _native

    assert _native.WIDE_PIP_FROM == cases.FROM              # where Ed448Point.msm hands over to dr_wide_msm


@pytest.mark.parametrize("name", cases.NAMES)
def test_digits_sum_back_to_the_scalar(exe, tmp_path, name):
    """0, 1, the largest value, all-7 and all-8 nibbles, the order and its neighbours and seeded random values, under the tilings of
    every window width (n = 256, 4100, 20000, 70000: c = 7, 8, 9, 10); the Python restatement of the digits agrees"""
    s = cases.SUITES[name]
    rng = cases._rng(name, "digits")
    ks = cases.edge_scalars(s) + [s.order - 2, s.top >> 1, (s.top >> 1) - 1] + [rng.getrandbits(s.bits - 1) for _ in range(200)]
    assert {0, 1, s.top - 1, s.order - 1, s.order, s.order + 1} <= set(ks) and s.top - 1 == (1 << 521 if name == "p521" else 1 << 8 * s.nbytes) - 1
    sizes = (256, 4100, 20000, 70000)
    h = _histograms(exe, tmp_path / "digits.txt", [(f"digits-{n}", s.bits, s.words, n, ks) for n in sizes])
    for n in sizes:
        t = cases.Tiling(n, s.bits)
        got = h[f"digits-{n}"]
        assert (got["c"], got["W"], got["H"], got["groups"], got["cmax"]) == (t.c, t.W, t.H, t.groups, t.cmax)
        assert got["reconstruct_bad"] == 0
        assert sum(t.widths) == s.bits and t.c == {256: 7, 4100: 8, 20000: 9, 70000: 10}[n]
        for k in ks:
            ds = cases.digits(k, t)
            assert sum(d << st for d, st in zip(ds, t.starts)) == k and all(abs(d) <= 1 << (w - 1) for d, w in zip(ds, t.widths))


def test_a_lost_carry_would_be_seen(exe, tmp_path):
    """the checker itself: a scalar with the bit above the tiling set does not reconstruct (2^384 has no place in 385 tiled bits' top
    digit when it is read as 12 words — the program refuses it — and 2^521 under P-521's 522 bits fills the sign position)"""
    path = tmp_path / "bad.txt"
    path.write_text("case over 522 17 256 1\n%x\n" % (1 << 521))
    proc = subprocess.run([exe, "hist", str(path)], capture_output=True, text=True)
    assert proc.returncode == 0 and "reconstruct_bad=1" in proc.stdout
    path.write_text("case wide 385 12 256 1\n%x\n" % (1 << 384))
    assert subprocess.run([exe, "hist", str(path)], capture_output=True, text=True).returncode == 2


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_family_plans_and_digits(hist, name, n):
    s = cases.SUITES[name]
    t = cases.Tiling(n, s.bits)
    assert t.groups == {cases.FROM: 1, 1030: 2, 4100: 4}[n] and t.c == (8 if n == 4100 else 7)
    for family in cases.FAMILIES:
        h = hist[f"{name}-{family}-{n}"]
        assert (h["n"], h["c"], h["W"], h["H"], h["groups"]) == (n, t.c, t.W, t.H, t.groups) and h["reconstruct_bad"] == 0
        assert h["heavy"] == sum(1 for x in h["lists"] if x[3] > cases.HEAVY)
    # random full-width scalars: nothing for the wave walk, and the last bucket of full-width windows is reached
    lad = hist[f"{name}-ladder-{n}"]
    assert lad["heavy"] == 0 and lad["longest"] < cases.HEAVY
    full = [w for w in range(t.W) if t.widths[w] == t.cmax]
    assert full and sum(lad["top"][w] for w in full) >= 1 and sum(lad["top"][w] for w in range(t.W) if w not in full) == 0


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_equal_has_one_long_list_per_window_and_group(hist, name, n):
    case, h = cases.case(name, "equal", n), hist[f"{name}-equal-{n}"]
    t = cases.Tiling(n, cases.SUITES[name].bits)
    nonzero = sum(1 for d in cases.digits(case.scalars[0], t) if d)
    assert h["heavy"] == nonzero * t.groups and nonzero >= t.W - 8
    assert sorted({x[3] for x in h["lists"]}) == case.claims["lengths"] and min(case.claims["lengths"]) > cases.HEAVY
    assert case.claims["lengths"] == {cases.FROM: [256], 1030: [515], 4100: [1025]}[n]


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_lengths_sit_on_both_sides_of_the_hand_over(hist, name, n):
    """a list of exactly 64 entries for the per-lane kernel and one of exactly 65 for the wave kernel, in window 0 of index group 0"""
    h = hist[f"{name}-lengths-{n}"]
    assert (0, 0, 0, 64, 0) in h["lists"] and (0, 0, 1, 65, 0) in h["lists"]
    assert [x for x in h["lists"] if x[0] == 0 and x[2] < 2] == [(0, 0, 0, 64, 0), (0, 0, 1, 65, 0)]
    # (in the other windows the distinct scalars' digits fall into the shared scalars' buckets too: lists of 64 and 65 and a few more)
    assert h["heavy"] >= h["W"]


@pytest.mark.parametrize("n", cases.SIZES)
@pytest.mark.parametrize("name", cases.NAMES)
def test_cancel_and_edges_claims(hist, name, n):
    s = cases.SUITES[name]
    mixed, ident, edges = (cases.case(name, f, n) for f in ("cancel-mixed", "cancel-identity", "edges"))
    hm, hi = hist[mixed.name], hist[ident.name]
    # 130 terms of one scalar, half of them negated points (the signs in the lists are the digits': all alike), and 100 repeats
    assert [t[0] for t in mixed.terms[:130]] == ["m", "neg"] * 65 and len({t[2] for t in mixed.terms[:130]}) == 1
    assert mixed.terms[130:230] == [("m", 7, mixed.terms[130][2])] * 100
    assert any(x[3] >= 130 for x in hm["lists"]) and any(100 <= x[3] < 130 for x in hm["lists"]) and hm["heavy"] >= 2
    # nothing but pairs: the total is the identity in the suite's spelling, and 80 terms share a scalar
    assert all(a[0] == "m" and b[0] == "neg" and a[1:] == b[1:] for a, b in zip(ident.terms[::2], ident.terms[1::2]))
    assert ident.expected() == s.identity and any(x[3] >= 80 for x in hi["lists"])
    assert s.identity == {"p384": bytes(96), "p521": bytes(136), "ed448": bytes(56) + b"\x01" + bytes(55), "curve448": b"\xff" * 112}[name]
    # edges: the scalars, identity points, and the small-order point under scalars a reduction mod n would change
    ks = edges.scalars
    assert ks[:8] == [0, 1, s.order - 1, s.order, s.order + 1, s.top - 1, cases.nibbles(s, 7), cases.nibbles(s, 8)]
    assert "%x" % cases.nibbles(s, 7) in ("7" * (2 * s.nbytes), "1" + "7" * 130) and "%x" % cases.nibbles(s, 8) in ("8" * (2 * s.nbytes), "8" * 130)
    assert sum(1 for t in edges.terms if t[0] == "id") == 5 and edges.terms[-1][2] == s.top - 1
    small = [t[2] for t in edges.terms if t[0] == "small"]
    if name in ("ed448", "curve448"):
        q, order = {"ed448": ((1, 0), 4), "curve448": ((0, 0), 2)}[name]
        assert s.small == q and s.small_order == order and s.ref.mul(order, q) == getattr(s.ref, "O", None) != s.ref.mul(order // 2, q)
        assert len(small) == 5 and all(k >= s.order for k in small)
        assert sum(small) % order != sum(k % s.order for k in small) % order
    else:
        assert not small


# ---------------------------------------------------------------- the upper half of the plan (test_gpu_wide_msm_plans.py)
EQUAL_LENGTHS = {1031: [515, 516], 4103: [1025, 1026], 16383: [2047, 2048], 16387: [2048, 2049], 65535: [4095, 4096], 65539: [4096, 4097],
                 131075: [4096, 4097], 262147: [4096, 4097]}


@pytest.fixture(scope="module")
def plan_hist(exe, tmp_path_factory):
    """name -> the histograms of every case of cases.PLANS on that suite, made at the first call for all four suites, one program each at
    the same time; the cases are built one at a time and dropped (all of a suite's together are 1.4 million scalars)"""
    done = {}
    printed = tmp_path_factory.mktemp("wide_msm_plans")

    def one(name):
        s = cases.SUITES[name]
        built = (cases.build(name, family, n) for n in cases.PLANS for family in cases.plan_families(n))
        rows = ((c.name, s.bits, s.words, c.n, c.scalars) for c in built)
        return _histograms(exe, printed / f"{name}.txt", rows, piped=True)

    def of(name):
        if not done:
            with ThreadPoolExecutor(len(cases.NAMES)) as pool:
                done.update(zip(cases.NAMES, pool.map(one, cases.NAMES)))
        return done[name]

    return of


@pytest.mark.parametrize("n", tuple(cases.PLANS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_upper_plans_and_their_ladder_lists(plan_hist, name, n):
    """the pinned plan, in which no group bound is a whole multiple; every family's digits sum back; the ladder scalars make no list of 64
    (a condition on the inputs: their GPU runs then are the per-lane walk alone) and reach the last bucket of full-width windows"""
    s = cases.SUITES[name]
    t = cases.Tiling(n, s.bits)
    c, widths, H, groups, _ = cases.PLANS[n]
    W = widths[(385, 449, 522).index(s.bits)]
    assert (t.c, t.W, t.H, t.groups, t.cmax) == (c, W, H, groups, c) and n % groups != 0 and groups <= 64
    assert [-(-g * n // groups) for g in range(groups + 1)] != [g * n // groups for g in range(groups + 1)]
    for family in cases.plan_families(n):
        h = plan_hist(name)[f"{name}-{family}-{n}"]
        assert (h["n"], h["c"], h["W"], h["H"], h["groups"], h["cmax"]) == (n, c, W, H, groups, c) and h["reconstruct_bad"] == 0
        assert h["heavy"] == sum(1 for x in h["lists"] if x[3] > cases.HEAVY)
        assert (h["rem"] == 0) == (len(set(t.widths)) == 1)
    if (n, s.bits) in ((16387, 522), (65535, 522)):
        assert h["rem"] == 0 and set(t.widths) == {9}                       # 522 = 58 x 9: no window of width 8
    lad = plan_hist(name)[f"{name}-ladder-{n}"]
    assert lad["heavy"] == 0 and lad["longest"] < cases.HEAVY
    full = [w for w in range(t.W) if t.widths[w] == t.cmax]
    assert full and sum(lad["top"][w] for w in full) >= 1 and sum(lad["top"][w] for w in range(t.W) if w not in full) == 0


@pytest.mark.parametrize("n", tuple(cases.PLANS))
@pytest.mark.parametrize("name", cases.NAMES)
def test_upper_equal_has_one_long_list_per_window_and_group(plan_hist, name, n):
    """one heavy list per non-zero digit and index group, of all the group's terms: two lengths, since n is no multiple of the groups"""
    case, h = cases.build(name, "equal", n), plan_hist(name)[f"{name}-equal-{n}"]
    t = cases.Tiling(n, cases.SUITES[name].bits)
    ds = cases.digits(case.scalars[0], t)
    nonzero = sum(1 for d in ds if d)
    assert len(set(case.scalars)) == 1 and h["heavy"] == nonzero * t.groups == len(h["lists"]) and nonzero >= t.W - 8
    assert sorted((x[0], x[1]) for x in h["lists"]) == [(w, g) for w in range(t.W) if ds[w] for g in range(t.groups)]
    assert all(x[2] == abs(ds[x[0]]) - 1 and x[4] == (x[3] if ds[x[0]] < 0 else 0) for x in h["lists"])
    assert sorted({x[3] for x in h["lists"]}) == case.claims["lengths"] == EQUAL_LENGTHS[n] and min(EQUAL_LENGTHS[n]) > cases.HEAVY
    assert h["longest"] == EQUAL_LENGTHS[n][1]


@pytest.mark.parametrize("n", tuple(n for n in cases.PLANS if "lengths" in cases.plan_families(n)))
@pytest.mark.parametrize("name", cases.NAMES)
def test_upper_lengths_and_cancelling_pairs(plan_hist, name, n):
    """lists of exactly 64 and 65 in window 0 of index group 0, and an odd number of terms that still sum to the identity"""
    h = plan_hist(name)[f"{name}-lengths-{n}"]
    assert [x for x in h["lists"] if x[0] == 0 and x[2] < 2] == [(0, 0, 0, 64, 0), (0, 0, 1, 65, 0)]
    assert h["heavy"] >= h["W"]
    s = cases.SUITES[name]
    ident = cases.build(name, "cancel-identity", n)
    assert n % 2 == 1 and ident.terms[-1][:2] == ("id", 0) and ident.terms[-1][2] >> (s.bits // 2)        # a long scalar on the identity
    assert all(a[0] == "m" and b[0] == "neg" and a[1:] == b[1:] for a, b in zip(ident.terms[:-1:2], ident.terms[1:-1:2]))
    assert ident.expected() == s.identity and any(x[3] >= 80 for x in plan_hist(name)[ident.name]["lists"])
    mixed = plan_hist(name)[f"{name}-cancel-mixed-{n}"]
    assert any(x[3] >= 130 for x in mixed["lists"]) and any(100 <= x[3] < 130 for x in mixed["lists"])


# ---------------------------------------------------------------- the host's window combination
@pytest.mark.parametrize("name", cases.NAMES)
def test_host_combine_equals_the_restatement(exe, tmp_path, name):
    """set sums m G (ladder points, some negated, some the identity) for the plans of 256, 1030 and 4100 terms, and of 16387, 65539 and
    262147 (widths 9 and 10; 8, 16 and 64 index groups: up to 3392 set sums): the program's combination is
    (sum_w 2^start_w sum_g m_wg mod n) G"""
    s = cases.SUITES[name]
    ref, lad = s.ref, cases.ladder(name)
    rng = cases._rng(name, "combine")
    blocks, want = [], []
    assert [cases.PLANS[n][3] for n in (16387, 65539, 262147)] == [8, 16, 64]
    for n in cases.SIZES + (16387, 65539, 262147, "identity"):
        t = cases.Tiling(256 if n == "identity" else n, s.bits)
        total, lines = 0, []
        for w in range(t.W):
            for g in range(t.groups):
                kind = "id" if n == "identity" else rng.choice(["m", "m", "m", "neg", "id"])
                i = rng.randrange(len(lad))
                pt = None if kind == "id" else lad[i] if kind == "m" else ref.neg(lad[i])
                total += (0 if kind == "id" else (cases.LADDER_A + i) * (1 if kind == "m" else -1)) << t.starts[w]
                lines.append(s.raw(pt).hex())
        blocks.append(f"sums {name} {256 if n == 'identity' else n}\n" + "\n".join(lines) + "\n")
        want.append(s.raw(ref.mul(total % s.order, ref.G) if total % s.order else None).hex())
    path = tmp_path / "sums.txt"
    path.write_text("".join(blocks))
    proc = subprocess.run([exe, "combine", str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert proc.stdout.split() == want and want[-1] == s.identity.hex()
