"""GPU: the claim-point and sum-tree kernels behind RingVRF.verify_each (csrc/kernels_g1_claims.hip.h) through
dr_g1_claim_tree_selftest, against the affine big-integer G1 reference of tests/test_fq28_forms_cpu.py (oracle/fq28_forms.py).

groups in {1, 2, 3, 63, 64, 65, 130} (one lane, below / at / above one 64-leaf workgroup, the second launch over the subtree roots)
and m in {2, 11}; scalars random, 0, 1, r - 1 and 2^255 - 1; points at infinity among the inputs; a group that sums to the identity;
two sibling leaves equal (the doubling inside the tree) and two opposite (the identity inside it); a whole 64-leaf subtree of
identities beside a live one; all identities.  Every node of every tree must come back bit-exact.

The reference multiplies each (point, scalar) pair of a small pool once; the groups draw their terms from the pool, so a case costs
additions only."""
import random

import pytest

import test_fq28_forms_cpu as forms

F = forms.F
coracle = forms.coracle
pytestmark = pytest.mark.gpu

R_ORDER = coracle.FR_P
SCALARS = [None, None, 0, 1, R_ORDER - 1, 2**255 - 1, None]          # None: random (the last one 128 bits)


@pytest.fixture(scope="module")
def pool():
    """[(point or None, scalar, scalar * point)]: six points and their negatives times seven scalars, and infinity times two"""
    rng = random.Random(0xC1A1)
    pts = [F.mul(F.G1_GEN, rng.randrange(2, 1 << 20)) for _ in range(6)]
    out = []
    for pt in pts:
        for j, s in enumerate(SCALARS):
            k = s if s is not None else rng.randrange(1 << 128) if j == 6 else rng.randrange(R_ORDER)
            prod = F.mul(pt, k)
            assert prod == F.mul(pt, k % R_ORDER)
            out.append((pt, k, prod))
            out.append((F.neg(pt), k, F.neg(prod)))
    out += [(None, rng.randrange(R_ORDER), None), (None, 0, None)]
    return out


def _enc_point(pt):
    return bytes(96) if pt is None else pt[0].to_bytes(48, "little") + pt[1].to_bytes(48, "little")


def _groups(pool, rng, groups, m, layout):
    zero = next(t for t in pool if t[0] is not None and t[1] == 0)
    if layout == "all_identity":
        return [[rng.choice([zero, pool[-1], pool[-2]]) for _ in range(m)] for _ in range(groups)]
    gs = [[rng.choice(pool) for _ in range(m)] for _ in range(groups)]
    if groups >= 2:
        gs[1] = list(gs[0])                                            # siblings equal: their parent is a doubling
    if groups >= 4:
        gs[3] = [(F.neg(p), k, F.neg(q)) for p, k, q in gs[2]]         # siblings opposite: their parent is the identity
    if groups >= 5:
        p, k, q = next(t for t in pool if t[2] is not None)
        gs[4] = [(p, k, q), (F.neg(p), k, F.neg(q))] + [zero] * (m - 2)      # a group that sums to the identity
    if layout == "dead_subtree":
        for g in range(64, min(groups, 128)):
            gs[g] = [rng.choice([zero, pool[-1]]) for _ in range(m)]
    return gs


def _reference_nodes(gs):
    padded = 1
    while padded < len(gs):
        padded *= 2
    nodes = [None] * (2 * padded - 1)
    for g, terms in enumerate(gs):
        acc = None
        for _, _, prod in terms:
            acc = F.add(acc, prod)
        nodes[padded - 1 + g] = acc
    for k in reversed(range(padded - 1)):
        nodes[k] = F.add(nodes[2 * k + 1], nodes[2 * k + 2])
    return nodes


CASES = [(g, m, "mixed") for g in (1, 2, 3, 63, 64, 65, 130) for m in (2, 11)]
CASES += [(130, 2, "dead_subtree"), (130, 11, "dead_subtree"), (3, 2, "all_identity"), (65, 11, "all_identity")]


@pytest.mark.parametrize("groups,m,layout", CASES)
def test_every_node_of_the_claim_tree_is_exact(ctx, pool, groups, m, layout):
    rng = random.Random(groups * 100 + m)
    gs = _groups(pool, rng, groups, m, layout)
    pts = b"".join(_enc_point(p) for terms in gs for p, _, _ in terms)
    scalars = b"".join(k.to_bytes(32, "little") for terms in gs for _, k, _ in terms)
    nodes, inf = ctx.g1_claim_tree_selftest(pts, scalars, groups, m)
    want = _reference_nodes(gs)
    assert len(nodes) == 96 * len(want) and len(inf) == len(want)
    bad = [k for k, w in enumerate(want) if nodes[96 * k : 96 * k + 96] != _enc_point(w) or inf[k] != (1 if w is None else 0)]
    assert not bad, f"nodes {bad[:8]} of {len(want)} differ"
    if layout == "mixed" and groups >= 5:
        padded = (len(want) + 1) // 2
        assert want[(padded - 1 + 2 - 1) // 2] is None and want[padded - 1 + 4] is None           # opposite siblings; the cancelling group
        assert want[padded - 1] is None or want[(padded - 1 - 1) // 2] == F.dbl(want[padded - 1])     # equal siblings
    if layout == "dead_subtree":
        assert want[4] is None and want[3] is not None                                   # leaves 64..127 beside leaves 0..63
    if layout == "all_identity":
        assert all(w is None for w in want)


def test_refusals(ctx):
    with pytest.raises(ValueError):
        ctx.g1_claim_tree_selftest(bytes(96), bytes(32), 2, 1)
    with pytest.raises(ValueError):
        ctx.g1_claim_tree_selftest(b"\xff" * 96, bytes(32), 1, 1)          # a coordinate >= p
