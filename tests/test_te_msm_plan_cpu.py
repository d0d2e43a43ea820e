"""CPU: the plan of the twisted Edwards Pippenger (dr::plan_te_msm, dot_ring_amd/csrc/msm_plan.hpp) and the bucket lists that the
input families of te_msm_cases.py make, from the library's own headers compiled for the host (tests/native/te_msm_plan_check.cpp).

The program checks the plan's invariants over a sweep of sizes for both orders and pins (c, W, H, groups) of every size the GPU tests and
pedersen_verify_core use.  Then it runs dr::for_each_digit per (window, index group) over the reduced scalars of every family, as
k_g1_sort_sets walks them, and prints the bucket histograms; the tests below assert on them what the families claim — so what
test_gpu_te_msm.py runs on the GPU is proved here to enter k_te_msm_accumulate_heavy, to sit on both sides of the hand-over between the
two accumulate kernels, and to reach the last bucket of k_te_msm_reduce."""
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import te_msm_cases as cases  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    out = tmp_path_factory.mktemp("te_msm_plan") / "te_msm_plan_check"
    subprocess.run(["g++", "-O1", "-std=c++17", "-I", os.path.join(ROOT, "dot_ring_amd", "csrc"),
                    os.path.join(ROOT, "tests", "native", "te_msm_plan_check.cpp"), "-o", str(out)], check=True)
    return str(out)


def _histograms(exe, path, rows):
    """rows: (name, scalar_bits, reduced scalars) -> {name: dict}"""
    with open(path, "w") as f:
        for name, bits, ks in rows:
            f.write(f"case {name} {bits} {len(ks)}\n")
            f.write("\n".join("%064x" % k for k in ks) + "\n")
    proc = subprocess.run([exe, "hist", str(path)], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    out, cur = {}, None
    for line in proc.stdout.splitlines():
        word = line.split()
        if word[0] == "case":
            cur = {k: v for k, v in (item.split("=") for item in word[2:])}
            cur = {k: [int(x) for x in v.split(",")] if k == "widths" else int(v) for k, v in cur.items()}
            cur["heavy_lists"] = []
            out[word[1]] = cur
        elif word[0] == "top":
            cur["top"] = [int(x) for x in word[1:]]
        elif word[0] == "heavy":
            cur["heavy_lists"].append(tuple(int(x) for x in word[1:]))          # (window, group, bucket, length, negative entries)
    assert list(out) == [name for name, _, _ in rows]
    return out


@pytest.fixture(scope="module")
def hist(exe, tmp_path_factory):
    rows = [(c.name, cases.SCALAR_BITS[c.curve], c.reduced) for c in cases.all_cases()]
    return _histograms(exe, tmp_path_factory.mktemp("te_msm_hist") / "families.txt", rows)


def test_te_msm_plan_invariants_and_pinned_sizes(exe):
    proc = subprocess.run([exe], capture_output=True, text=True)
    assert proc.returncode == 0, proc.stderr
    assert "te msm plan ok" in proc.stdout and f"heavy from {cases.HEAVY + 1}" in proc.stdout


@pytest.mark.parametrize("name", cases.NAMES)
def test_family_plan_and_digits(hist, name):
    """the Python restatement the families are aimed with (tiling, signed_digits) is the C++ plan, and the digits of for_each_digit sum
    back to every scalar"""
    case, h = cases.case(name), hist[name]
    t = cases.tiling(case.n, case.curve)
    assert (h["n"], h["c"], h["W"], h["H"], h["groups"], h["widths"]) == (case.n, t.c, t.W, t.H, t.groups, t.widths)
    assert h["heavy_from"] == cases.HEAVY + 1
    assert h["reconstruct_bad"] == 0
    assert all(k < case.order for k in case.reduced) and len(set(j for j in case.idx if j >= 0)) <= cases.POOL[case.curve]
    for k in case.reduced[:: max(1, case.n // 64)]:
        assert sum(d << s for d, s in zip(cases.signed_digits(k, t), t.starts)) == k
    assert h["longest"] == (max(x[3] for x in h["heavy_lists"]) if h["heavy_lists"] else h["longest"]) and len(h["heavy_lists"]) == h["heavy"]


@pytest.mark.parametrize("name", [n for n in cases.NAMES if "-equal-" in n])
def test_equal_has_one_long_list_per_window_and_group(hist, name):
    case, h = cases.case(name), hist[name]
    assert h["groups"] == case.claims["groups"] and h["heavy"] == case.claims["heavy"] > 0
    assert sorted({x[3] for x in h["heavy_lists"]}) == case.claims["heavy_lengths"]
    want = {"bsn-equal-256": (1, [256]), "bsn-equal-1030": (2, [515]), "bsn-equal-65536": (16, [4096]), "jub-equal-300": (1, [300]),
            "jub-equal-1030": (2, [515]), "sw-equal-300": (1, [300])}[name]
    assert (h["groups"], case.claims["heavy_lengths"]) == want


@pytest.mark.parametrize("name", [n for n in cases.NAMES if "-lengths-" in n])
def test_lengths_sit_on_both_sides_of_the_hand_over(hist, name):
    """lists of exactly 64, 65, 127, 128, 129 and 193 entries in the aimed window and nothing else: five for the wave kernel (one entry
    over, one under and one over two rounds, three rounds and one), the 64-entry list for the per-lane kernel"""
    case, h = cases.case(name), hist[name]
    t = cases.tiling(case.n, case.curve)
    w = case.claims["window"]
    assert w == {"low": 0, "middle": t.W // 2, "top": t.W - 1}[name.rsplit("-", 1)[1]]
    assert h["heavy_lists"] == [(w, 0, 0, 65, 0), (w, 0, 2, 127, 0), (w, 0, 3, 128, 0), (w, 0, 4, 129, 0), (w, 0, 5, 193, 0)]
    assert h["exact"] == 1 and h["longest"] == 193 and h["heavy"] == 5
    digits = [cases.signed_digits(k, t) for k in case.reduced]
    assert all(sum(1 for d in ds if d) == 1 and 1 <= ds[w] <= 6 for ds in digits)
    assert [sum(1 for ds in digits if ds[w] == v) for v in range(1, 7)] == [65, 64, 127, 128, 129, 193]


@pytest.mark.parametrize("name", [n for n in cases.NAMES if "-cancel-" in n or "-verifier-" in n])
def test_cancel_and_verifier_have_heavy_lists(hist, name):
    case, h = cases.case(name), hist[name]
    assert h["heavy"] >= case.claims["min_heavy"] >= 1
    assert case.n >= 256
    if name.endswith("cancel-opposite"):
        t = cases.tiling(case.n, case.curve)
        assert t.groups == 1 and case.idx[:130] == [0] * 130 and case.idx[130:260] == [0, cases.negated(0)] * 65
        assert all((case.reduced[i] + case.reduced[i + 1]) % case.order == 0 for i in range(0, 130, 2))
        digits = [cases.signed_digits(k, t) for k in case.reduced]
        # (P, s) and (P, order - s) meet in a bucket only in the few windows where the order has a run of equal bits: everywhere else
        # two lists of 65 per window, for the wave kernel
        assert sum(1 for a, b in zip(digits[0], digits[1]) if abs(a) == abs(b) != 0) <= 3
        assert sum(1 for x in h["heavy_lists"] if x[3] >= 65) >= 3
        # (P, u) and (-P, u): some window has a list of exactly these 130 terms — 65 x +P, 65 x -P, the identity in sum
        assert len(set(case.reduced[130:260])) == 1
        alone = [w for w in range(t.W) if digits[130][w] and [i for i in range(case.n) if abs(digits[i][w]) == abs(digits[130][w])] == list(range(130, 260))]
        assert alone and all((w, 0, abs(digits[130][w]) - 1, 130, 130 if digits[130][w] < 0 else 0) in h["heavy_lists"] for w in alone)
    if name.endswith("cancel-same"):
        assert case.idx[:200] == [0] * 200 and len(set(case.reduced[:200])) == 1 and max(x[3] for x in h["heavy_lists"]) >= 200
    if name.endswith("cancel-identity"):
        assert case.idx[:164].count(cases.IDENTITY) == 100 and len(set(case.reduced[:164])) == 1
        assert max(x[3] for x in h["heavy_lists"]) >= 164
    if "-verifier-" in name:
        batch = int(name.rsplit("-", 1)[1])
        assert case.n == 5 * batch + 2
        short = [i for i, k in enumerate(case.reduced) if k < 1 << 128]
        assert short == [i for i in range(5 * batch) if i % 5 in (0, 3)]


@pytest.mark.parametrize("name", [n for n in cases.NAMES if "-top-bucket-" in n])
def test_top_bucket_reaches_the_last_bucket_of_every_full_width_window(hist, name):
    """the planted scalars: digit +2^(width-1) in every window below the top one (the top window's digits stay below order >> start,
    which is less than half its range on both curves), i.e. bucket H - 1 of every full-width window below the top; and digit
    -(2^(width-1) - 1) with a carry in every window below the top, whose digit is the last carry"""
    case, h = cases.case(name), hist[name]
    t = cases.tiling(case.n, case.curve)
    assert t.c == case.claims["c"] == {256: 7, 4096: 8, 16384: 9, 65536: 10}[case.n]
    i_plus, i_minus = case.claims["planted"]
    plus, minus = cases.signed_digits(case.reduced[i_plus], t), cases.signed_digits(case.reduced[i_minus], t)
    assert plus == [1 << (w - 1) for w in t.widths[:-1]] + [0]
    assert minus == [-((1 << (w - 1)) - 1) for w in t.widths[:-1]] + [1]
    assert (case.order >> t.starts[-1]) < 1 << (t.widths[-1] - 1)          # why the top window cannot hold either pattern
    full = [w for w in range(t.W - 1) if t.full(w)]
    assert len(full) >= 19 and all(h["top"][w] >= 1 for w in full)          # (c = 10: 20 of the 26 windows are 10 bits wide)
    # H - L, the last chunk of k_te_msm_reduce, holds bucket H - 1: the planted term alone puts an entry there in its own group
    assert all(plus[w] == t.H for w in full)


def test_existing_pippenger_inputs_have_no_heavy_list(exe, tmp_path):
    """regression guard for the statement in DESIGN.md: the six inputs of test_bsn_msm_pippenger_matches_oracle stay with the per-lane kernel"""
    rows = [(f"existing-{n}", 253, cases.existing_pippenger_scalars(n)) for n in cases.EXISTING_SIZES]
    h = _histograms(exe, tmp_path / "existing.txt", rows)
    got = [(n, h[f"existing-{n}"]["c"], h[f"existing-{n}"]["W"], h[f"existing-{n}"]["H"], h[f"existing-{n}"]["groups"]) for n in cases.EXISTING_SIZES]
    assert got == [(256, 7, 37, 64, 1), (257, 7, 37, 64, 1), (1024, 7, 37, 64, 2), (5122, 8, 32, 128, 4), (20482, 9, 29, 256, 8), (65536, 10, 26, 512, 16)]
    for n in cases.EXISTING_SIZES:
        assert h[f"existing-{n}"]["heavy"] == 0 and h[f"existing-{n}"]["longest"] < cases.HEAVY and h[f"existing-{n}"]["reconstruct_bad"] == 0
