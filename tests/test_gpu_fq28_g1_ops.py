"""GPU: the base field (csrc/fq28.hip.h) and the XYZZ group law (csrc/g1.hip.h) under the G1 kernels, one operation at a time,
on raw register images (dr_fq_ops_selftest, dr_g1_ops_selftest), against plain Python integers (oracle/fq28_forms.py).

An MSM on random scalars almost never meets the operands where this code can be wrong: values at k p +- 1 for canon28, zero
products in every lazy form for maybe_zero_normal, the exceptional cases of the group law under non-unit Z.  Here each lane puts
its operands on the edge of its own op's preconditions, and every output is checked twice: its congruence, and the register
form the code documents (limb bounds, value range) — the form is what the next consumer relies on."""
import random

import pytest

from oracle import coracle
from oracle import fq28_forms as F

pytestmark = pytest.mark.gpu

P = F.P
R = F.R
(MUL, SQR, MUL2, ADD, SUB, CARRY, CANON, IS_ZERO, MAYBE_ZERO, INV, TO_MONT, FROM_MONT, UNPACK, CNEG) = range(14)
OP_NAMES = "mul sqr mul2 add sub carry canon28 is_zero_mod_p maybe_zero_normal inv to_mont28 from_mont28 unpack28 cneg".split()
RANDOM_LANES = 2000


def _rec(op, a=(), b=(), c=(), d=()):
    """one 64-word record: the op, four operands of 14 limbs (shorter ones — 12 words — padded with zeros)"""
    rec = [op]
    for x in (a, b, c, d):
        assert len(x) <= F.NL
        rec += list(x) + [0] * (F.NL - len(x))
    return rec + [0] * 7


def _images(v, rng):
    """v in the lazy forms canon28 / is_zero_mod_p / inv meet: carry-normal, carries moved (|limb| < 2^29 + 1, < 3 2^28 + 2),
    a difference of two N images"""
    n = F.normal(v)
    return [n, F.scramble(n, rng, 1), F.scramble(n, rng, 2), F.d_image(v, rng.randrange(P))]


def _zero_forms(rng):
    """values = 0 (mod p) in every lazy form the group law produces: 0, +-p .. +-4p as N / scrambled / d images, and sums of a
    value and its negation made limb-wise, without a carry"""
    out = []
    for k in range(-4, 5):
        out += _images(k * P, rng)
    for _ in range(8):
        v = rng.randrange(P)
        out.append([x + y for x, y in zip(F.normal(v), F.normal(P - v))])            # value p, limbs < 2^29
        out.append([x + y for x, y in zip(F.normal(v), F.d_image(-v, rng.randrange(P)))])      # value 0
        out.append([x - y for x, y in zip(F.normal(v + P), F.normal(v))])              # value p, limbs (-2^28, 2^28)
    return out


def _fq_lanes(rng):
    lanes = []                                           # (record, tag)
    # products: the operand shapes the kernels use, random and every limb at +-(bound - 1)
    for la, lb, va, vb in F.MUL_SHAPES:
        for _ in range(RANDOM_LANES // 4):
            lanes.append((_rec(MUL, F.lazy(rng, la, va), F.lazy(rng, lb, vb)), "mul shape"))
    ea, eb = F.MUL_EXTREME
    for sa in (1, -1):
        for sb in (1, -1):
            lanes.append((_rec(MUL, F.extreme(ea, sa), F.extreme(eb, sb)), "mul extreme"))
            lanes.append((_rec(MUL, F.extreme(eb, sa), F.extreme(ea, sb)), "mul extreme"))
    sl, sv = F.SQR_SHAPE
    for _ in range(RANDOM_LANES):
        lanes.append((_rec(SQR, F.lazy(rng, sl, sv)), "sqr shape"))
    for s in (1, -1):
        lanes.append((_rec(SQR, F.extreme(sl, s)), "sqr extreme"))
    shape2 = F.MUL2_SHAPE
    for _ in range(RANDOM_LANES):
        lanes.append((_rec(MUL2, *[F.lazy(rng, lb_, vb_) for lb_, vb_ in shape2]), "mul2 shape"))
    for signs in ((1, 1, 1, 1), (-1, 1, -1, 1), (1, -1, -1, -1), (-1, -1, 1, 1)):
        lanes.append((_rec(MUL2, *[F.extreme(lb_, s) for (lb_, _), s in zip(shape2, signs)]), "mul2 extreme"))
    # limb-wise ops
    for _ in range(RANDOM_LANES):
        lanes.append((_rec(ADD, F.lazy(rng, 1 << 29, 16), F.lazy(rng, 1 << 29, 16)), "add"))
        lanes.append((_rec(SUB, F.lazy(rng, 1 << 29, 16), F.lazy(rng, 1 << 29, 16)), "sub"))
        lanes.append((_rec(CARRY, F.lazy(rng, 1 << 30, 31)), "carry"))
        lanes.append((_rec(CNEG, F.lazy(rng, 1 << 30, 31), [rng.randrange(2)] + [0] * 13), "cneg"))
    for s in (1, -1):
        lanes.append((_rec(CARRY, F.extreme(1 << 30, s)), "carry extreme"))
    # canon28 / is_zero_mod_p: k p + delta for k in -7..7, delta in {-1, 0, 1}, +-(8p - 1), every zero form
    edge_vals = [k * P + dl for k in range(-7, 8) for dl in (-1, 0, 1)] + [8 * P - 1, -(8 * P - 1), 8 * P - 2, 1 - 8 * P]
    for v in edge_vals:
        for img in _images(v, rng):
            lanes.append((_rec(CANON, img), "canon edge"))
            lanes.append((_rec(IS_ZERO, img), "is_zero edge"))
    for img in _zero_forms(rng):
        lanes.append((_rec(CANON, img), "canon zero form"))
        lanes.append((_rec(IS_ZERO, img), "is_zero zero form"))
        b = F.lazy(rng, 1 << 28, 2)
        lanes.append((_rec(MAYBE_ZERO, img, b), "maybe_zero zero operand"))
        lanes.append((_rec(MAYBE_ZERO, b, img), "maybe_zero zero operand"))
    for _ in range(RANDOM_LANES):
        img = F.lazy(rng, 1 << 30, 7.99)
        lanes.append((_rec(CANON, img), "canon random"))
        lanes.append((_rec(IS_ZERO, img), "is_zero random"))
        lanes.append((_rec(MAYBE_ZERO, F.lazy(rng, 1 << 29, 8), F.lazy(rng, 1 << 28, 8)), "maybe_zero random"))
    # the group law's zero test of P = U2 - x with U2 = x (mod p): U2 anywhere in a product's range, x in its whole range
    for _ in range(200):
        v = rng.randrange(P)
        u2 = v + rng.choice([0, P]) if v < P // 2 else v - rng.choice([0, P])       # a normal product's value for v
        for x in (v - P, v, v + P, v + 2 * P, v - 4 * P):                            # x in (-5p, 3p)
            lanes.append((_rec(IS_ZERO, [a - b for a, b in zip(F.normal(u2), F.normal(x))]), "is_zero U2 - x"))
    # inversion and the conversions: small values, halves, powers of two, the R-related constants, then random lanes
    consts = [0, 1, 2, 3, P - 1, P - 2, (P - 1) // 2, (P + 1) // 2, R % P, R * R % P, R**3 % P, pow(R, -1, P), pow(2, 384, P),
              pow(2, 400, P), 4 * R % P]
    consts += [1 << k for k in (1, 27, 28, 29, 55, 56, 191, 363, 364, 379, 380)]
    for x in consts:
        for img in _images(x, rng) + _images(x + P, rng) + _images(x - P, rng):
            lanes.append((_rec(INV, img), "inv edge"))
            lanes.append((_rec(FROM_MONT, img), "from_mont edge"))
        lanes.append((_rec(TO_MONT, F.words12(x)), "to_mont edge"))
        lanes.append((_rec(UNPACK, F.words12(x)), "unpack edge"))
    for x in (P, 2 * P, (1 << 381) - 1, (1 << 384) - 1):           # non-canonical words: unpack28 is exact, to_mont28's mul still holds
        lanes.append((_rec(TO_MONT, F.words12(x)), "to_mont wide"))
        lanes.append((_rec(UNPACK, F.words12(x)), "unpack wide"))
    for img in _zero_forms(rng):
        lanes.append((_rec(INV, img), "inv zero form"))
    for _ in range(RANDOM_LANES):
        lanes.append((_rec(INV, F.lazy(rng, 1 << 30, 7.99)), "inv random"))
        lanes.append((_rec(FROM_MONT, F.lazy(rng, 1 << 30, 31)), "from_mont random"))
        x = rng.randrange(P)
        lanes.append((_rec(TO_MONT, F.words12(x)), "to_mont random"))
        lanes.append((_rec(UNPACK, F.words12(rng.randrange(1 << 384))), "unpack random"))
    return lanes


def _normal_product(limbs, want_times_r, tag):
    """a mul / sqr / mul2 output: limbs 0..12 in [0, 2^28), value in (-p/2, 1.5 p), value R = the product (mod p)"""
    v = F.value(limbs)
    assert (v * R - want_times_r) % P == 0, ("congruence", tag)
    assert F.is_n(limbs), ("limbs 0..12 outside [0, 2^28)", tag, limbs)
    assert -P // 2 < v < P + P // 2, (f"value {v / P:.3f} p outside (-p/2, 1.5 p)", tag)


def test_fq28_ops_against_big_integers(ctx):
    """dr_fq_ops_selftest: every operation of fq28.hip.h on the edges of its documented preconditions and on random lanes"""
    rng = random.Random(28)
    lanes = _fq_lanes(rng)
    raw = ctx.fq_ops_selftest(b"".join(F.pack_i32(r) for r, _ in lanes))
    out = F.unpack_i32(raw)
    seen = {}
    for i, (rec, tag) in enumerate(lanes):
        op, a, b, c, d = rec[0], rec[1:15], rec[15:29], rec[29:43], rec[43:57]
        o = out[16 * i : 16 * i + 16]
        limbs, flag = o[:14], o[14]
        va, vb, vc, vd = F.value(a), F.value(b), F.value(c), F.value(d)
        tag = (OP_NAMES[op], tag, i)
        seen[OP_NAMES[op]] = seen.get(OP_NAMES[op], 0) + 1
        if op in (MUL, SQR, MUL2):
            want = va * vb if op == MUL else va * va if op == SQR else va * vb + vc * vd
            if "extreme" in tag[1]:              # operands far outside the value range: the congruence and the limb form only
                assert (F.value(limbs) * R - want) % P == 0 and F.is_n(limbs), tag
            else:
                _normal_product(limbs, want, tag)
        elif op == ADD:
            assert limbs == [x + y for x, y in zip(a, b)], tag
        elif op == SUB:
            assert limbs == [x - y for x, y in zip(a, b)], tag
        elif op == CNEG:
            assert limbs == ([-x for x in a] if b[0] & 1 else a), tag
        elif op == CARRY:
            assert limbs == F.normal(va), tag                # value unchanged, limbs 0..12 in [0, 2^28)
        elif op == CANON:
            assert abs(va) < 8 * P, tag
            assert F.from_words(limbs[:12]) == va % P, (tag, hex(va))     # canonical: exactly the residue, < p
        elif op == IS_ZERO:
            assert flag == (1 if va % P == 0 else 0), (tag, hex(va))
        elif op == MAYBE_ZERO:
            _normal_product(limbs, va * vb, tag)
            zero = (va * vb) % P == 0
            assert flag == (1 if limbs[0] in (0, F.P_LIMBS[0]) else 0), tag
            if zero:
                assert flag == 1, ("maybe_zero_normal missed a zero", tag, F.value(limbs) // P)
        elif op == INV:
            x = va % P
            if x == 0:
                assert limbs == [0] * 14, ("inv(0) must be 0", tag)
            else:
                _normal_product(limbs, R * R * R * pow(x, -1, P), tag)      # (x / R)^-1 R = R^2 / x; times R for the congruence
        elif op == TO_MONT:
            _normal_product(limbs, F.from_words(a[:12]) * R * R, tag)
        elif op == FROM_MONT:
            assert F.from_words(limbs[:12]) == F.from_mont(va), tag
        elif op == UNPACK:
            assert limbs == F.normal(F.from_words(a[:12])), tag
    assert all(seen.get(name, 0) >= RANDOM_LANES for name in OP_NAMES), seen


# ---------------------------------------------------------------- group law
SLOT = 60
CHAIN = 24
SLOTS_OUT = 32
N_REF = {"x": (-5, 3), "y": (-2, 2), "zz": (-0.5, 1.5), "zzz": (-0.5, 1.5)}       # value / p of each coordinate of an XYZZ output


class _Ranges:
    """value / p and limb extremes reached per (output, coordinate), for the assertion messages and the printed summary"""

    def __init__(self):
        self.r = {}

    def add(self, key, limbs):
        v = F.value(limbs) / P
        lo, hi, lm = self.r.get(key, (v, v, 0))
        self.r[key] = (min(lo, v), max(hi, v), max(lm, F.max_limb(limbs)))

    def __str__(self):
        return "; ".join(f"{k[0]}.{k[1]}: [{lo:.3f}, {hi:.3f}] p, max|limb| 2^{lm.bit_length()}" for k, (lo, hi, lm) in sorted(self.r.items()))


def _check_xyzz(words, want, name, tag, ranges):
    got, consistent = F.decode_xyzz(words)
    x, y, zz, zzz, inf = F.split_xyzz(words)
    assert inf in (0, 1), (name, tag, inf)
    assert (inf == 1) == (want is None), (name, tag, "infinity flag", inf)
    if want is None:
        return
    assert consistent, (name, tag, "ZZ^3 != ZZZ^2 (mod p)")
    assert got == want, (name, tag, "wrong point")
    for cname, limbs in (("x", x), ("y", y), ("zz", zz), ("zzz", zzz)):
        ranges.add((name, cname), limbs)
        lo, hi = N_REF[cname]
        v = F.value(limbs)
        ok_limbs = F.is_d(limbs) if cname == "y" else F.is_n(limbs)
        assert ok_limbs, (name, tag, cname, "limb form", limbs, str(ranges))
        assert lo * P < v < hi * P, (name, tag, cname, f"value {v / P:.3f} p outside ({lo}, {hi}) p", str(ranges))


def _g1_lanes(rng):
    gen = F.G1_GEN
    rand_pt = lambda: coracle.g1_mul(gen, rng.randrange(1, coracle.FR_P))          # noqa: E731
    rz = lambda: rng.choice([1, 2, P - 1, rng.randrange(1, P), rng.randrange(1, P)])  # noqa: E731

    def xi(pt):
        return F.xyzz_image(pt, rz(), rng, rng.choice([-1, 0, 1]), rng.choice([0, -1]), rng.choice(["d", "d", "n"]))

    def ai(pt, y_form=None):
        return F.affine_image(pt, rng, rng.choice([-1, 0, 1]), y_form or rng.choice(["n", "d", "cneg"]))

    lanes = []                                         # (P, Q, A points; P, Q, A images; tag)

    def lane(p, q, a, tag, pi=None, qi=None, aimg=None):
        lanes.append((p, q, a, pi or xi(p), qi or xi(q), aimg or ai(a), tag))

    for _ in range(300):
        lane(rand_pt(), rand_pt(), rand_pt(), "random")
    for _ in range(40):
        p = rand_pt()
        lane(p, p, rand_pt(), "Q = P, another Z")
        lane(p, F.neg(p), rand_pt(), "Q = -P")
        lane(p, rand_pt(), p, "A = affine(P)")
        lane(p, rand_pt(), F.neg(p), "A = -affine(P) through cneg", aimg=ai(F.neg(p), "cneg"))
        lane(p, F.dbl(p), rand_pt(), "Q = 2P")
        lane(p, F.neg(p), p, "Q = -P, A = P")
        lane(p, p, F.neg(p), "Q = P, A = -P")
        a = rand_pt()
        lane(rand_pt(), rand_pt(), a, "A.y through cneg", aimg=ai(a, "cneg"))
        img = xi(p)
        lane(p, p, rand_pt(), "Q = P, same image", pi=img, qi=list(img))
        lane(p, rand_pt(), rand_pt(), "P with Z = 1", pi=F.xyzz_image(p, 1, rng, 0, 0, "n"))
    for _ in range(10):
        lane(None, rand_pt(), rand_pt(), "P at infinity")
        lane(rand_pt(), None, rand_pt(), "Q at infinity")
        lane(rand_pt(), rand_pt(), None, "A at infinity")
        lane(None, None, rand_pt(), "P, Q at infinity")
        lane(None, rand_pt(), None, "P, A at infinity")
        lane(None, None, None, "all at infinity")
    return lanes


def test_g1_group_law_on_register_images(ctx):
    """dr_g1_ops_selftest: g1_add, g1_madd, g1_dbl, g1_dbl_affine, g1_to_affine_dev, the store / load round trip and a 24-step
    chain (madd A, add Q, dbl) per lane, on random points under random Z with x in each allowed representative and y with
    negative limbs, and on the exceptional cases: Q = P under another Z, Q = -P, A = +-affine(P), Q = 2P, infinities"""
    rng = random.Random(381)
    lanes = _g1_lanes(rng)
    recs = []
    for _, _, _, pi, qi, aimg, _ in lanes:
        recs += list(pi) + [0] * (64 - len(pi)) + list(qi) + [0] * (64 - len(qi)) + list(aimg) + [0] * (64 - len(aimg))
    out = F.unpack_i32(ctx.g1_ops_selftest(F.pack_i32(recs)))
    per = SLOTS_OUT * SLOT
    ranges = _Ranges()
    for i, (p, q, a, pi, qi, aimg, tag) in enumerate(lanes):
        o = out[per * i : per * (i + 1)]
        slot = lambda k: o[SLOT * k : SLOT * k + F.XYZZ_RAW_WORDS]      # noqa: E731
        tag = (tag, i)
        _check_xyzz(slot(0), F.add(p, q), "add", tag, ranges)
        _check_xyzz(slot(1), F.add(p, a), "madd", tag, ranges)
        _check_xyzz(slot(2), F.dbl(p), "dbl", tag, ranges)
        if a is not None:                              # g1_dbl_affine is only reached for a finite point (g1_madd tests q.inf first)
            _check_xyzz(slot(3), F.dbl(a), "dbl_affine", tag, ranges)
        # to_affine: x, y are products (normal), the flag follows P
        s4 = slot(4)
        x4, y4, _, _, inf4 = F.split_xyzz(s4)
        assert (inf4 == 1) == (p is None), ("to_affine", tag)
        if p is not None:
            for cname, limbs in (("x", x4), ("y", y4)):
                ranges.add(("to_affine", cname), limbs)
                _normal_product(limbs, F.to_mont(p[0] if cname == "x" else p[1]) * R, ("to_affine", cname, tag))
        # store_xyzz -> memory words (canonical) -> load_xyzz
        mem = [w & 0xFFFFFFFF for w in o[6 * SLOT : 6 * SLOT + 48]]
        if p is None:
            assert mem == [0] * 48, ("store_xyzz of infinity", tag)
        else:
            for k, limbs in enumerate(F.split_xyzz(pi)[:4]):
                assert F.from_words(mem[12 * k : 12 * k + 12]) == F.value(limbs) % P, ("store_xyzz", k, tag)
        _check_xyzz(slot(5), p, "load(store)", tag, ranges)
        acc = p
        for k in range(CHAIN):
            acc = F.add(acc, a) if k % 3 == 0 else F.add(acc, q) if k % 3 == 1 else F.dbl(acc)
            _check_xyzz(slot(7 + k), acc, f"chain[{k}]" if k < 3 else f"chain[{k % 3}+3j]", tag, ranges)
    print("\nG1 register ranges reached:", ranges)
