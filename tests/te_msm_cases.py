"""The input families of the twisted Edwards Pippenger tests (te_msm_pippenger, capi_msm.hip), written once: the CPU test
(test_te_msm_plan_cpu.py) proves from the scalars alone which bucket lists each family makes, the GPU test (test_gpu_te_msm.py) runs
exactly these terms.  Plain Python over SHA-256 seeds; nothing here touches a GPU.

A case is (name, curve, points, scalars): `scalars` are Python ints, `points` affine pairs of the curve's own form (twisted Edwards
for curves 0 and 1, short Weierstrass with None for the identity on curve 2), built on first use from a small pool of seeded subgroup
points that the terms reuse cyclically (`idx[i]` = pool index of term i, -1 = the identity point, negated(j) = minus pool point j).

`tiling` restates dr::plan_te_msm (msm_plan.hpp) and `signed_digits` dr::for_each_digit (msm_recode.hip.h); the families use them to
aim at windows and buckets, and the CPU test checks both against the C++ they restate."""
import hashlib
from functools import cached_property

BANDERSNATCH, JUBJUB, BANDERSNATCH_SW = 0, 1, 2
ORDER = {
    BANDERSNATCH: 0x1CFB69D4CA675F520CCE760202687600FF8F87007419047174FD06B52876E7E1,
    JUBJUB: 0x0E7DB4EA6533AFA906673B0101343B00A6682093CCC81082D0970E5ED6F72CB7,
    BANDERSNATCH_SW: 0x1CFB69D4CA675F520CCE760202687600FF8F87007419047174FD06B52876E7E1,
}
SCALAR_BITS = {cv: order.bit_length() for cv, order in ORDER.items()}          # 253, 252, 253
POOL = {BANDERSNATCH: 64, JUBJUB: 16, BANDERSNATCH_SW: 16}                      # distinct points (the last two have Python references)
HEAVY = 64                                                                      # dr::TE_HEAVY_BUCKET (the CPU test compares)
IDENTITY = -1
FIELD = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001      # the base field of all three curves


def negated(j):
    """idx value for -pool[j] (j >= 0), and back: an involution on everything but IDENTITY"""
    return -2 - j


# ------------------------------------------------------------------ the plan and the recoding, restated
class Tiling:
    def __init__(self, n, scalar_bits):
        self.c = 7 if n < 4096 else 8 if n < 16384 else 9 if n < 65536 else 10
        bits = scalar_bits + 1
        self.W = -(-bits // self.c)
        base, rem = divmod(bits, self.W)
        self.widths = [base + (1 if w >= self.W - rem else 0) for w in range(self.W)]
        self.starts = [sum(self.widths[:w]) for w in range(self.W)]
        self.cmax = max(self.widths)
        self.H = 1 << (self.cmax - 1)
        self.groups = 1
        while self.groups < 64 and n // (self.groups * 2 * self.H) >= 8:
            self.groups *= 2

    def full(self, w):
        return self.widths[w] == self.cmax

    def bounds(self, g, n):
        return -(-g * n // self.groups), -(-(g + 1) * n // self.groups)


def tiling(n, curve=BANDERSNATCH):
    return Tiling(n, SCALAR_BITS[curve])


def signed_digits(k, t):
    """the digits of for_each_digit, zeros included: raw = bits + carry; raw > half becomes raw - 2^width with a carry"""
    out, carry = [], 0
    for start, width in zip(t.starts, t.widths):
        raw = ((k >> start) & ((1 << width) - 1)) + carry
        carry = 1 if raw > (1 << (width - 1)) else 0
        out.append(raw - (carry << width))
    assert carry == 0 and k >> (t.starts[-1] + t.widths[-1]) == 0
    return out


# ------------------------------------------------------------------ seeds
def _h(tag, i):
    return int.from_bytes(hashlib.sha256(tag.encode() + b"/" + i.to_bytes(8, "little")).digest(), "little")


def seeded(tag, count, mod):
    return [_h(tag, i) % mod for i in range(count)]


class Case:
    def __init__(self, name, curve, idx, scalars, claims=None):
        assert len(idx) == len(scalars)
        self.name, self.curve, self.idx, self.scalars = name, curve, list(idx), list(scalars)
        self.claims = claims or {}                   # what the CPU test proves about the bucket lists of this case

    @property
    def n(self):
        return len(self.scalars)

    @property
    def order(self):
        return ORDER[self.curve]

    @cached_property
    def reduced(self):
        return [k % self.order for k in self.scalars]

    @cached_property
    def points(self):
        pool = point_pool(self.curve)
        ident = None if self.curve == BANDERSNATCH_SW else (0, 1)
        minus = (lambda p: (p[0], -p[1] % FIELD)) if self.curve == BANDERSNATCH_SW else (lambda p: (-p[0] % FIELD, p[1]))
        return [ident if j == IDENTITY else pool[j] if j >= 0 else minus(pool[negated(j)]) for j in self.idx]

    def __iter__(self):
        return iter((self.name, self.curve, self.points, self.scalars))

    def __repr__(self):
        return self.name


_POOLS = {}


def point_pool(curve):
    """the curve's seeded subgroup points: k_j G for k_j = sha256("te-msm-pool/<curve>/" j) mod the order (never 0)"""
    if curve not in _POOLS:
        ks = [_h(f"te-msm-pool/{curve}", j) % (ORDER[curve] - 1) + 1 for j in range(POOL[curve])]
        if curve == BANDERSNATCH:
            from oracle import coracle
            from oracle.pyref import bandersnatch as bsn

            _POOLS[curve] = [coracle.te_mul(bsn.G, k) for k in ks]
        elif curve == JUBJUB:
            from oracle.pyref import bandersnatch as bsn

            with bsn.using(bsn.JUBJUB):
                _POOLS[curve] = [bsn.mul_py(bsn.G, k) for k in ks]
        else:
            import sw_ref

            _POOLS[curve] = [sw_ref.mul(k, sw_ref.G) for k in ks]
    return _POOLS[curve]


def _cyclic(n, curve):
    return [i % POOL[curve] for i in range(n)]


def _tag(curve):
    return {BANDERSNATCH: "bsn", JUBJUB: "jub", BANDERSNATCH_SW: "sw"}[curve]


# ------------------------------------------------------------------ families
def equal(curve, n):
    """all scalars one seeded value: every window has ONE list per index group, n / groups long.  Closed form: k * sum P_i"""
    k = _h(f"te-msm-equal/{curve}/{n}", 0) % ORDER[curve]
    t = tiling(n, curve)
    lists = sum(1 for d in signed_digits(k, t) if d) * t.groups
    lens = sorted({hi - lo for lo, hi in (t.bounds(g, n) for g in range(t.groups))})
    return Case(f"{_tag(curve)}-equal-{n}", curve, _cyclic(n, curve), [k] * n, {"heavy": lists, "heavy_lengths": lens, "groups": t.groups})


LENGTHS = ((1, 65), (2, 64), (3, 127), (4, 128), (5, 129), (6, 193))          # (digit, terms): 706 terms, no filler


def lengths(curve, where):
    """lists of exactly 64, 65, 127, 128, 129 and 193 entries in one window (digits 2, 1, 3, 4, 5, 6): five for the wave kernel, the
    64-entry list for the per-lane kernel.  where = "low": window 0; "middle": the scalars shifted to the start bit of window W / 2;
    "top": of window W - 1 (its digits must stay below order >> start: 57 on both curves, these reach 6)"""
    n = sum(count for _, count in LENGTHS)
    t = tiling(n, curve)
    w = {"low": 0, "middle": t.W // 2, "top": t.W - 1}[where]
    assert 6 < ORDER[curve] >> t.starts[w] and 6 <= 1 << (t.widths[w] - 1) and t.groups == 1
    ks = [digit << t.starts[w] for digit, count in LENGTHS for _ in range(count)]
    # interleave the six values (a stride coprime to 706) so that no list is a contiguous run of terms
    ks = [ks[i * 271 % n] for i in range(n)]
    return Case(f"{_tag(curve)}-lengths-{where}", curve, _cyclic(n, curve), ks,
                {"window": w, "window_lengths": [65, 64, 127, 128, 129, 193], "heavy": 5, "exactly_heavy": 1})


def _filler(tag, curve, count, avoid=None):
    """seeded random terms below the order; `avoid(k)`: candidates to skip (the next seed is taken)"""
    out, i = [], 0
    while len(out) < count:
        k = _h(tag, i) % ORDER[curve]
        i += 1
        if avoid is None or not avoid(k):
            out.append(k)
    return out


def cancel_opposite(curve):
    """Terms 0..129: 65 x (P, s) and 65 x (P, order - s), interleaved.  Their 130 terms cancel in the MSM, but hardly ever inside a
    bucket: the digits of order - s are not the negatives of those of s (digit_w(s) + digit_w(order - s) is the order's own window w
    give or take a carry: zero only where the order has a run of equal bits — for these s no window on Bandersnatch, one on JubJub), so
    these make two lists of 65 in nearly every window, which the wave kernel walks.  Terms 130..259: 65 x (P, u) and 65 x (-P, u), interleaved — equal digits, opposite points: in every window of u ONE list
    of 130 entries, 65 of them +P and 65 -P, whose sum is the identity and whose lanes hold P - P, 2 P - 2 P or the like.  Terms
    260..299: seeded random terms over the other pool points."""
    order = ORDER[curve]
    s, u = _h(f"te-msm-cancel/{curve}", 0) % order, _h(f"te-msm-cancel/{curve}", 1) % order
    fill = _filler(f"te-msm-cancel-fill/{curve}", curve, 40)
    ks = [s, order - s] * 65 + [u] * 130 + fill
    idx = [0] * 130 + [0, negated(0)] * 65 + [1 + i % (POOL[curve] - 2) for i in range(40)]
    return Case(f"{_tag(curve)}-cancel-opposite", curve, idx, ks, {"min_heavy": 3})


def cancel_same(curve):
    """200 x the same (P, s), padded to 256: in every window of s the lanes of the wave hold 4 P (lanes 0..7) or 3 P, so the shuffle
    tree adds equal points, i.e. doubles through the unified addition"""
    s = _h(f"te-msm-same/{curve}", 0) % ORDER[curve]
    fill = _filler(f"te-msm-same-fill/{curve}", curve, 56)
    return Case(f"{_tag(curve)}-cancel-same", curve, [0] * 200 + [1 + i % (POOL[curve] - 1) for i in range(56)], [s] * 200 + fill, {"min_heavy": 1})


def cancel_identity(curve):
    """the identity point (0, 1) 100 times inside heavy lists: 100 x ((0, 1), s) interleaved with 64 x (P_i, s), padded to 256"""
    s = _h(f"te-msm-ident/{curve}", 0) % ORDER[curve]
    idx = [IDENTITY] * 100 + _cyclic(64, curve)
    idx = [idx[i * 37 % 164] for i in range(164)]                  # 37 is coprime to 164: a permutation
    fill = _filler(f"te-msm-ident-fill/{curve}", curve, 92)
    return Case(f"{_tag(curve)}-cancel-identity", curve, idx + _cyclic(92, curve), [s] * 164 + fill, {"min_heavy": 1})


def verifier(batch):
    """the scalar shape of pedersen_verify_core (capi_batch.hip): 5 B + 2 terms, terms 0 and 3 of every five below 2^128 (the batch
    weights), the rest below the order.  The window that starts at bit 128 sees only the carry of the short ones: one bucket."""
    n, order = 5 * batch + 2, ORDER[BANDERSNATCH]
    ks = [_h(f"te-msm-verifier/{batch}", i) % (1 << 128 if i < 5 * batch and i % 5 in (0, 3) else order) for i in range(n)]
    return Case(f"bsn-verifier-{batch}", BANDERSNATCH, _cyclic(n, BANDERSNATCH), ks, {"min_heavy": 1})


def top_patterns(t, order):
    """(all digits +2^(width-1), all raw digits 2^(width-1) + 1): the largest such patterns below the order.
    First: bit start + width - 1 of every window, taken from the top down while the value stays below the order (the top window's
    would be bit scalar_bits: it stays empty) — bucket H - 1 of every full-width window but the top one.
    Second: raw = bits + carry = half + 1 in every window, i.e. bits half + 1 in window 0 and half above it: digit -(half - 1) and a
    carry; the first window that cannot take its bits (the top one) receives the last carry as digit +1."""
    plus = 0
    for w in reversed(range(t.W)):
        bit = 1 << (t.starts[w] + t.widths[w] - 1)
        if plus + bit < order:
            plus += bit
    minus = 1
    for w in range(t.W):
        bit = 1 << (t.starts[w] + t.widths[w] - 1)
        if minus + bit >= order:
            break
        minus += bit
    return plus, minus


def top_bucket(curve, n):
    t, order = tiling(n, curve), ORDER[curve]
    plus, minus = top_patterns(t, order)
    ks = seeded(f"te-msm-top/{curve}/{n}", n, order)
    ks[n // 3], ks[2 * n // 3 + 1] = plus, minus
    return Case(f"{_tag(curve)}-top-bucket-{n}", curve, _cyclic(n, curve), ks,
                {"c": t.c, "top_bucket": True, "planted": (n // 3, 2 * n // 3 + 1)})


def plan_edge(curve, n):
    """random scalars (on JubJub unreduced, below 2^256) at a size where the plan changes"""
    mod = 1 << 256 if curve == JUBJUB else ORDER[curve]
    return Case(f"{_tag(curve)}-plan-edge-{n}", curve, _cyclic(n, curve), seeded(f"te-msm-edge/{curve}/{n}", n, mod))


def random_case(curve, n, tag="before"):
    """the checked random MSM that runs before a family on the same context, so that the scratch holds foreign points"""
    return Case(f"{_tag(curve)}-{tag}-{n}", curve, _cyclic(n, curve), seeded(f"te-msm-{tag}/{curve}/{n}", n, ORDER[curve]))


PLAN_EDGES = (1023, 1024, 2047, 2048, 4095, 4096, 16383, 16384, 65535)
TOP_SIZES = (256, 4096, 16384, 65536)                                         # c = 7, 8, 9, 10

_BUILDERS = (
    [("bsn-equal-%d" % n, lambda n=n: equal(BANDERSNATCH, n)) for n in (256, 1030, 65536)]
    + [("bsn-lengths-%s" % w, lambda w=w: lengths(BANDERSNATCH, w)) for w in ("low", "middle", "top")]
    + [("bsn-cancel-opposite", lambda: cancel_opposite(BANDERSNATCH)), ("bsn-cancel-same", lambda: cancel_same(BANDERSNATCH)),
       ("bsn-cancel-identity", lambda: cancel_identity(BANDERSNATCH))]
    + [("bsn-verifier-%d" % b, lambda b=b: verifier(b)) for b in (100, 205)]
    + [("bsn-top-bucket-%d" % n, lambda n=n: top_bucket(BANDERSNATCH, n)) for n in TOP_SIZES]
    + [("bsn-plan-edge-%d" % n, lambda n=n: plan_edge(BANDERSNATCH, n)) for n in PLAN_EDGES]
    + [("jub-equal-%d" % n, lambda n=n: equal(JUBJUB, n)) for n in (300, 1030)]
    + [("jub-lengths-%s" % w, lambda w=w: lengths(JUBJUB, w)) for w in ("low", "middle", "top")]
    + [("jub-cancel-opposite", lambda: cancel_opposite(JUBJUB)), ("jub-cancel-same", lambda: cancel_same(JUBJUB)),
       ("jub-cancel-identity", lambda: cancel_identity(JUBJUB))]
    + [("jub-top-bucket-%d" % n, lambda n=n: top_bucket(JUBJUB, n)) for n in (256, 4096)]
    + [("jub-plan-edge-4096", lambda: plan_edge(JUBJUB, 4096))]
    + [("sw-equal-300", lambda: equal(BANDERSNATCH_SW, 300))]
)
NAMES = [name for name, _ in _BUILDERS]
_CASES = {}


def case(name):
    if name not in _CASES:
        _CASES[name] = dict(_BUILDERS)[name]()
        assert _CASES[name].name == name
    return _CASES[name]


def all_cases():
    return [case(name) for name in NAMES]


def existing_pippenger_scalars(n):
    """the scalars of test_bsn_msm_pippenger_matches_oracle (test_gpu_kernels.py) at its size n, restated: the regression guard that
    those inputs make no heavy list"""
    order = ORDER[BANDERSNATCH]
    ks = [int.from_bytes(hashlib.sha256(b"pipk" + i.to_bytes(8, "little")).digest(), "little") % order for i in range(n)]
    ks[0], ks[1], ks[2] = 0, order - 1, 1
    ks[5] = (order - ks[4]) % order
    return ks


EXISTING_SIZES = (256, 257, 1024, 5122, 20482, 65536)
