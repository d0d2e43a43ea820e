"""The case table of the single-launch C entry points, written once: tools/record_entry_surface.py ran it on the GPU at the commit
before the host round trips were merged and wrote tests/golden/entry_surface_gpu.json; tests/test_gpu_entry_surface.py replays it and
compares entry by entry.  A case is one call of one entry point of libdotring_hip.so through ctypes (so that null pointers, bad sizes
and unknown ids reach the library as they are) and records the return code, dr_last_error() on refusal, every output buffer (hex, or a
digest of its SHA-256 beyond 64 bytes; buffers start as 0xa5 bytes, so an untouched one shows) and the launch count of every name in
LAUNCH_NAMES that is not zero.  `expect` holds what the independent restatements (tests/*_ref.py, oracle/pyref, the RFC 9380 vector
files) say about an output: the recorder asserts it before it writes, so the file is not merely what the library did.

Every refused case is refused on the host before any launch (but for the four of REFUSED_AFTER_SW_TO_TE); every accepted one passes valid inputs, or strings that a decoder kernel
judges.  An oversize `n` comes with small buffers: only on entry points that compare n with their limit before they read a buffer."""
import ctypes
import hashlib
import json
import os
import random
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (HERE, ROOT):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import babyjubjub_ref  # noqa: E402
import bls12_381_g1_ref  # noqa: E402
import bls12_381_g2_ref  # noqa: E402
import curve25519_ref  # noqa: E402
import ed25519_ref  # noqa: E402
import ed448_ref  # noqa: E402
import p256_ref  # noqa: E402
import secp256k1_ref  # noqa: E402
import sw_ref  # noqa: E402
from oracle import coracle  # noqa: E402
from oracle.pyref import bandersnatch as bsn  # noqa: E402

GOLDEN = os.path.join(HERE, "golden", "entry_surface_gpu.json")
H2C = os.path.join(HERE, "golden", "h2c")
LAUNCH_NAMES = [    # every name the library launches under (csrc: launch(ctx, "...") and the NTT's run("...")), the other units' included
    "k_bsn_scalar_mul", "k_bsn_msm_groups", "k_bsn_fixed_base", "k_bsn_decode_points", "k_sw_decode_points", "k_sw_to_te", "k_te_to_sw",
    "k_bsn_encode_to_curve", "k_te_msm_prepare", "k_te_msm_accumulate", "k_te_msm_reduce",
    "k_ed_scalar_mul", "k_ed_msm_groups", "k_ed_decode_points", "k_ed25519_map_to_curve",
    "k_p256_scalar_mul", "k_p256_msm_groups", "k_p256_decode_points", "k_p256_map_to_curve",
    "k_bjj_scalar_mul", "k_bjj_msm_groups", "k_bjj_decode_points",
    "k_secp256k1_scalar_mul", "k_secp256k1_msm_groups", "k_secp256k1_decode_points", "k_secp256k1_map_to_curve",
    "k_c25519_scalar_mul", "k_c25519_msm_groups", "k_c25519_decode_points", "k_curve25519_map_to_curve",
    "k_blsg1_map_to_curve", "k_blsg1_scalar_mul", "k_blsg1_msm_groups", "k_blsg1_decode_points",
    "k_blsg2_map_iso", "k_blsg2_sum_clear", "k_blsg2_scalar_mul", "k_blsg2_check_points",
    "k_ed448_map_to_curve", "k_ed448_scalar_mul", "k_ed448_msm_groups", "k_ed448_check_points",
    "k_g1_accumulate", "k_g1_decompress", "k_g1_digits", "k_g1_horner", "k_g1_part_scatter", "k_g1_part_sort", "k_g1_reduce_chunks",
    "k_g1_reduce_windows", "k_g1_results_affine", "k_g1_scatter", "k_g1_sort_sets", "k_scan", "k_size_sort", "k_syndiv",
    "k_ring_aggpoly", "k_ring_chain", "k_ring_columns", "k_ring_constraints", "k_ring_diff", "k_ring_eval", "k_ring_linpoly", "k_ring_pad",
    "k_ring_quotient", "k_ntt_local", "k_ntt_strided", "k_ntt_twiddles", "wipe",
]
# Refusals that come after a launch: the SW boundary maps the points to their TE images (k_sw_to_te, on valid points) before the inner call
# looks at the scalars.  Recorded with that launch, so that the order of the boundary's checks is pinned; no kernel sees the null.
REFUSED_AFTER_SW_TO_TE = {f"{label}/Bandersnatch_SW/null_scalars" for label in ("te_scalar_mul_batch", "te_msm_groups", "te_msm", "te_fixed_base")}
POOL = 16                      # distinct points per curve: (j + 2) G, reused cyclically
UNKNOWN_CURVE = 12             # (not assigned)


class Ctx:
    """stands for the context argument"""


class Out:
    """an output buffer of n bytes"""

    def __init__(self, n):
        self.n = n


class U64:
    """an array of 64-bit offsets"""

    def __init__(self, values):
        self.values = list(values)


class Lazy:
    """an expected value that only the recorder computes"""

    def __init__(self, f):
        self.f = f


class Case:
    def __init__(self, key, fn, args, expect=None, fresh=False):
        self.key, self.fn, self.args, self.expect, self.fresh = key, fn, args, expect or {}, fresh


def brief(raw: bytes) -> str:
    """an output as the file keeps it: "-" where the call left it untouched, hex up to 64 bytes, beyond that 16 hex digits of its SHA-256"""
    if raw == b"\xa5" * len(raw):
        return "-"
    return raw.hex() if len(raw) <= 64 else "#" + hashlib.sha256(raw).hexdigest()[:16]


def run(lib, ctx, case):
    """one call: {"rc", and where there is any "err", "out", "launches"} and the raw output buffers"""
    outs, cargs = [], []
    for a in case.args:
        if isinstance(a, Out):
            outs.append(ctypes.create_string_buffer(b"\xa5" * a.n, a.n))
            cargs.append(outs[-1])
        elif isinstance(a, U64):
            cargs.append((ctypes.c_uint64 * len(a.values))(*a.values))
        else:
            cargs.append(ctx if a is Ctx else a)
    lib.dr_prof_reset(ctx)
    rc = getattr(lib, case.fn)(*cargs)
    record = {"rc": rc}
    if rc:
        record["err"] = lib.dr_last_error().decode()
    launches = {}
    for name in LAUNCH_NAMES:
        count = ctypes.c_int(0)
        lib.dr_prof_get(ctx, name.encode(), None, ctypes.byref(count))
        if count.value:
            launches[name] = count.value
    raws = [o.raw for o in outs]
    if any(brief(r) != "-" for r in raws):
        record["out"] = [brief(r) for r in raws]
    if launches:
        record["launches"] = launches
    return record, raws


def run_all(lib, cases):
    """{key: record} and {key: raw outputs} of the whole table; `fresh` cases start on a new context"""
    from dot_ring_amd import _native

    records, raws, ctx = {}, {}, None
    try:
        for case in cases:
            if ctx is None or case.fresh:
                if ctx is not None:
                    lib.dr_ctx_destroy(ctx)
                ctx = ctypes.c_void_p()
                _native._check(lib.dr_ctx_create(0, ctypes.byref(ctx)))
                lib.dr_prof_enable(ctx, 1)
            assert case.key not in records, case.key
            records[case.key], raws[case.key] = run(lib, ctx, case)
    finally:
        if ctx is not None:
            lib.dr_ctx_destroy(ctx)
    return records, raws


def check_expectations(cases, raws):
    """what the restatements say, against the raw outputs (expect = {output index: bytes, or {item: bytes} of equal-sized items}): the
    list of outputs that differ"""
    failures = []
    for case in cases:
        for index, want in case.expect.items():
            got = raws[case.key][index]
            for item, blob in want.items() if isinstance(want, dict) else [(0, want)]:
                blob = blob.f() if isinstance(blob, Lazy) else blob
                if got[len(blob) * item : len(blob) * (item + 1)] != blob or (not isinstance(want, dict) and len(got) != len(blob)):
                    failures.append(f"{case.key}: output {index}, item {item}")
    return failures


# ------------------------------------------------------------------ the curves of the 64-byte entry points
class Group:
    """one curve id of the dr_te_* entry points through its restatement: the field, the order, (j + 2) G for j < POOL, a G for any a"""

    def __init__(self, name, cid, p, order, g, add, mul, raw=None, identity=bytes(64), fr=False):
        self.name, self.cid, self.p, self.order, self.g, self.add, self.mul, self.identity, self.fr = name, cid, p, order, g, add, mul, identity, fr
        self._raw = raw or (lambda pt: pt[0].to_bytes(32, "little") + pt[1].to_bytes(32, "little"))
        self._pool = None

    def raw(self, pt):
        return self.identity if pt is None or self._raw(pt) == self.identity else self._raw(pt)

    @property
    def pool(self):
        if self._pool is None:
            pts = [self.add(self.g, self.g)]
            while len(pts) < POOL:
                pts.append(self.add(pts[-1], self.g))
            self._pool = pts
        return self._pool

    def times_g(self, a):
        return Lazy(lambda: self.identity if a % self.order == 0 else self.raw(self.mul(a % self.order, self.g)))


def _jubjub(f):
    def inner(*args):
        with bsn.using(bsn.JUBJUB):
            return f(*args)
    return inner


TE_IDENTITY = bytes(32) + (1).to_bytes(32, "little")
GROUPS = [
    Group("Bandersnatch", 0, bsn.P, bsn.N, bsn.G, bsn.add, lambda k, pt: coracle.te_mul(pt, k), identity=TE_IDENTITY, fr=True),
    Group("JubJub", 1, bsn.P, bsn._CURVES["jubjub"]["N"], bsn._CURVES["jubjub"]["G"], _jubjub(bsn.add), _jubjub(lambda k, pt: bsn.mul_py(pt, k)),
          identity=TE_IDENTITY, fr=True),
    Group("Bandersnatch_SW", 2, sw_ref.P, sw_ref.N, sw_ref.G, sw_ref.add, sw_ref.mul, sw_ref.raw, fr=True),
    Group("Ed25519", 3, ed25519_ref.P, ed25519_ref.N, ed25519_ref.G, ed25519_ref.add, ed25519_ref.mul, identity=TE_IDENTITY),
    Group("P256", 4, p256_ref.P, p256_ref.N, p256_ref.G, p256_ref.add, p256_ref.mul, p256_ref.raw),
    Group("P256_RO", 8, p256_ref.P, p256_ref.N, p256_ref.G, p256_ref.add, p256_ref.mul, p256_ref.raw),
    Group("BabyJubJub", 5, babyjubjub_ref.P, babyjubjub_ref.N, babyjubjub_ref.G, babyjubjub_ref.add, babyjubjub_ref.mul, identity=TE_IDENTITY),
    Group("Secp256k1", 6, secp256k1_ref.P, secp256k1_ref.N, secp256k1_ref.G, secp256k1_ref.add, secp256k1_ref.mul, secp256k1_ref.raw),
    Group("Curve25519_RO", 13, ed25519_ref.P, ed25519_ref.N, curve25519_ref.G, curve25519_ref.add, curve25519_ref.mul, identity=b"\xff" * 64),
]
BY_NAME = {g.name: g for g in GROUPS}


def terms(g, n, tag):
    """n terms on curve g: pool indices, 256-bit scalars (term 0: the order + 5), their bytes, and the packed points"""
    rng = random.Random(f"entry-surface/{g.name}/{tag}/{n}")
    idx = [i % POOL for i in range(n)]
    ks = [rng.getrandbits(256) for _ in range(n)]
    if n:
        ks[0] = g.order + 5
    return idx, ks, b"".join(g.raw(g.pool[j]) for j in idx), b"".join(k.to_bytes(32, "little") for k in ks)


def some(n):
    """the items whose expected value the recorder computes: all of a small output, the ends of a long one"""
    return range(n) if n <= 4 else (0, 1, n // 2, n - 1)


def group_sums(g, idx, ks, groups, m):
    """{group: bytes} of sum k_i (idx_i + 2) G over each group's m terms, for some() of the groups"""
    return {q: g.times_g(sum(ks[q * m + j] * (idx[q * m + j] + 2) for j in range(m))) for q in some(groups)}


def te_cases():
    cases = []
    for g in GROUPS:
        cid, tag = g.cid, g.name
        # ---- dr_te_scalar_mul_batch
        for n in (1, 3, 65):
            idx, ks, pts, sc = terms(g, n, "mul")
            cases.append(Case(f"te_scalar_mul_batch/{tag}/n{n}", "dr_te_scalar_mul_batch", [Ctx, cid, pts, sc, n, Out(64 * n)],
                              {0: {i: g.times_g(ks[i] * (idx[i] + 2)) for i in some(n)}}))
        idx, ks, pts, sc = terms(g, 3, "mul")
        cases.append(Case(f"te_scalar_mul_batch/{tag}/n0", "dr_te_scalar_mul_batch", [Ctx, cid, pts, sc, 0, Out(64)]))
        for pos, what in ((0, "ctx"), (2, "pts"), (3, "scalars"), (5, "out")):
            args = [Ctx, cid, pts, sc, 3, Out(192)]
            args[pos] = None
            cases.append(Case(f"te_scalar_mul_batch/{tag}/null_{what}", "dr_te_scalar_mul_batch", args))
        bad = g.p.to_bytes(32, "little") + pts[32:]
        cases.append(Case(f"te_scalar_mul_batch/{tag}/x_is_p", "dr_te_scalar_mul_batch", [Ctx, cid, bad, sc, 3, Out(192)]))
        if not g.fr or g.cid == 2:        # (the Fr curves read the points before they look at n; the SW boundary looks at n first)
            cases.append(Case(f"te_scalar_mul_batch/{tag}/oversize", "dr_te_scalar_mul_batch", [Ctx, cid, pts, sc, 1 << 31, Out(64)]))
            cases.append(Case(f"te_scalar_mul_batch/{tag}/null_and_oversize", "dr_te_scalar_mul_batch", [Ctx, cid, None, sc, 1 << 31, Out(64)]))
        # ---- dr_te_msm_groups: 3 groups of m
        for m in (1, 2, 33, 64) if g.fr else (1, 2, 64):
            idx, ks, pts, sc = terms(g, 3 * m, "groups")
            cases.append(Case(f"te_msm_groups/{tag}/m{m}", "dr_te_msm_groups", [Ctx, cid, pts, sc, 3, m, Out(192)], {0: group_sums(g, idx, ks, 3, m)}))
        idx, ks, pts, sc = terms(g, 6, "groups")
        cases.append(Case(f"te_msm_groups/{tag}/groups0", "dr_te_msm_groups", [Ctx, cid, pts, sc, 0, 2, Out(64)]))
        for pos, what in ((0, "ctx"), (2, "pts"), (3, "scalars"), (6, "out")):
            args = [Ctx, cid, pts, sc, 3, 2, Out(192)]
            args[pos] = None
            cases.append(Case(f"te_msm_groups/{tag}/null_{what}", "dr_te_msm_groups", args))
        cases.append(Case(f"te_msm_groups/{tag}/m0", "dr_te_msm_groups", [Ctx, cid, pts, sc, 3, 0, Out(192)]))
        cases.append(Case(f"te_msm_groups/{tag}/m65", "dr_te_msm_groups", [Ctx, cid, pts, sc, 3, 65, Out(192)]))
        cases.append(Case(f"te_msm_groups/{tag}/m0_and_null", "dr_te_msm_groups", [Ctx, cid, None, sc, 3, 0, Out(192)]))
        cases.append(Case(f"te_msm_groups/{tag}/oversize", "dr_te_msm_groups", [Ctx, cid, pts, sc, 1 << 31, 1, Out(64)]))
        cases.append(Case(f"te_msm_groups/{tag}/x_is_p", "dr_te_msm_groups", [Ctx, cid, g.p.to_bytes(32, "little") + pts[32:], sc, 3, 2, Out(192)]))
        # ---- dr_te_msm
        for n in (0, 1, 64, 65, 128, 255, 256):
            idx, ks, pts, sc = terms(g, n, "msm")
            cases.append(Case(f"te_msm/{tag}/n{n}", "dr_te_msm", [Ctx, cid, pts, sc, n, Out(64)], {0: group_sums(g, idx, ks, 1, n)[0]}))
        idx, ks, pts, sc = terms(g, 3, "msm")
        for pos, what in ((0, "ctx"), (2, "pts"), (3, "scalars"), (5, "out")):
            args = [Ctx, cid, pts, sc, 3, Out(64)]
            args[pos] = None
            cases.append(Case(f"te_msm/{tag}/null_{what}", "dr_te_msm", args))
        cases.append(Case(f"te_msm/{tag}/x_is_p", "dr_te_msm", [Ctx, cid, g.p.to_bytes(32, "little") + pts[32:], sc, 3, Out(64)]))
        if g.cid == 2:                    # (the SW boundary alone has a limit that it checks before it reads)
            cases.append(Case(f"te_msm/{tag}/oversize", "dr_te_msm", [Ctx, cid, pts, sc, 1 << 26, Out(64)]))
        # ---- dr_te_fixed_base_msm_groups: m constant bases
        for m in (1, 4):
            for groups in (3, 65):
                rng = random.Random(f"entry-surface/{tag}/fixed/{m}/{groups}")
                ks = [rng.getrandbits(256) for _ in range(groups * m)]
                bases = b"".join(g.raw(pt) for pt in g.pool[:m])
                sc = b"".join(k.to_bytes(32, "little") for k in ks)
                cases.append(Case(f"te_fixed_base/{tag}/m{m}_groups{groups}", "dr_te_fixed_base_msm_groups",
                                  [Ctx, cid, bases, m, sc, groups, Out(64 * groups)], {0: group_sums(g, list(range(m)) * groups, ks, groups, m)}))
        bases = b"".join(g.raw(pt) for pt in g.pool[:5])
        sc = b"".join(k.to_bytes(32, "little") for k in range(7, 22))
        cases.append(Case(f"te_fixed_base/{tag}/groups0", "dr_te_fixed_base_msm_groups", [Ctx, cid, bases, 2, sc, 0, Out(64)]))
        for pos, what in ((0, "ctx"), (2, "bases"), (4, "scalars"), (6, "out")):
            args = [Ctx, cid, bases, 2, sc, 3, Out(192)]
            args[pos] = None
            cases.append(Case(f"te_fixed_base/{tag}/null_{what}", "dr_te_fixed_base_msm_groups", args))
        cases.append(Case(f"te_fixed_base/{tag}/m0", "dr_te_fixed_base_msm_groups", [Ctx, cid, bases, 0, sc, 3, Out(192)]))
        cases.append(Case(f"te_fixed_base/{tag}/m5", "dr_te_fixed_base_msm_groups", [Ctx, cid, bases, 5, sc, 3, Out(192)]))
        cases.append(Case(f"te_fixed_base/{tag}/m0_and_null", "dr_te_fixed_base_msm_groups", [Ctx, cid, None, 0, sc, 3, Out(192)]))
        cases.append(Case(f"te_fixed_base/{tag}/oversize", "dr_te_fixed_base_msm_groups", [Ctx, cid, bases, 1, sc, 1 << 31, Out(64)]))
        cases.append(Case(f"te_fixed_base/{tag}/null_and_oversize", "dr_te_fixed_base_msm_groups", [Ctx, cid, bases, 1, None, 1 << 31, Out(64)]))
    # ---- an unknown curve id, alone and with a null
    pts, sc = bytes(192), bytes(96)
    for fn, args, null_at in (("dr_te_scalar_mul_batch", [Ctx, UNKNOWN_CURVE, pts, sc, 3, Out(192)], 2),
                              ("dr_te_msm_groups", [Ctx, UNKNOWN_CURVE, pts, sc, 3, 1, Out(192)], 2),
                              ("dr_te_msm", [Ctx, UNKNOWN_CURVE, pts, sc, 3, Out(64)], 2),
                              ("dr_te_fixed_base_msm_groups", [Ctx, UNKNOWN_CURVE, pts, 1, sc, 3, Out(192)], 2),
                              ("dr_te_decode_points", [Ctx, UNKNOWN_CURVE, pts, 3, Out(192), Out(3)], 2)):
        cases.append(Case(f"{fn[3:]}/unknown_curve", fn, list(args)))
        args[null_at] = None
        cases.append(Case(f"{fn[3:]}/unknown_curve_and_null", fn, args))
    return cases


# ------------------------------------------------------------------ decoders
def sec1(pt):
    return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(32, "big")


ENCODERS = {   # curve -> (bytes per encoding, encode)
    "Bandersnatch": (32, bsn.enc_point), "JubJub": (32, bsn.enc_point), "Bandersnatch_SW": (33, sw_ref.encode), "Ed25519": (32, ed25519_ref.encode),
    "P256": (33, p256_ref.encode), "P256_RO": (33, sec1), "BabyJubJub": (32, babyjubjub_ref.encode), "Secp256k1": (33, sec1),
    "Curve25519_RO": (64, curve25519_ref.raw),
}
OWN_DECODERS = {"Ed25519": "dr_ed25519_decode_points", "P256": "dr_p256_decode_points", "BabyJubJub": "dr_bjj_decode_points",
                "Secp256k1": "dr_secp256k1_decode_points", "Curve25519_RO": "dr_curve25519_decode_points"}


def junk(width, p):
    """strings a decoder judges: not canonical, small values (some have no root, some are the identity or off the curve), the codecs'
    identity strings"""
    le = lambda v: v.to_bytes(32, "little")  # noqa: E731
    tail = width - 32
    out = [b"\xff" * width, le(p) + bytes(tail), bytes(width), le(1) + bytes(tail), le(2) + bytes(tail), le(5) + bytes(tail)]
    if tail == 1:
        out += [bytes(32) + b"\x40", le(3) + b"\x80", b"\x02" + bytes(32), b"\x03" + (7).to_bytes(32, "big")]
    if tail == 32:
        out += [le(9) + le(1), le(0) + le(0), le(p) + le(1)]
    return out


def decode_strings(g, n):
    """n encodings: valid ones with junk() at every fourth place from 1; {item: the point} of some() valid ones"""
    width, encode = ENCODERS[g.name]
    bad = junk(width, g.p)
    encs, want = [], {}
    for i in range(n):
        if i % 4 == 1:
            encs.append(bad[(i // 4) % len(bad)])
        else:
            encs.append(encode(g.pool[i % POOL]))
            want[i] = g.raw(g.pool[i % POOL])
    keep = [i for i in want if n <= 4 or i in (0, 2, n - 1)]
    return b"".join(encs), {i: want[i] for i in keep}, {i: b"\x01" for i in keep}, bad


def decoder_cases():
    cases = []
    for g in GROUPS:
        width = ENCODERS[g.name][0]
        calls = [("te_decode_points", "dr_te_decode_points", [g.cid])]
        if g.name in OWN_DECODERS:
            calls += [(f"{OWN_DECODERS[g.name][3:]}_check{c}", OWN_DECODERS[g.name], [c]) for c in (1, 0)]
        for label, fn, head in calls:
            key = f"{label}/{g.name}"
            for n in (1, 3, 65):
                enc, pts, flags, bad = decode_strings(g, n)
                cases.append(Case(f"{key}/n{n}", fn, [Ctx] + head + [enc, n, Out(64 * n), Out(n)], {0: pts, 1: flags}, fresh=n == 65))
                if n == 65:               # a small batch of one refused string on the context that has just run the large one
                    cases.append(Case(f"{key}/n1_after_n65", fn, [Ctx] + head + [bad[0], 1, Out(64), Out(1)]))
            enc = decode_strings(g, 3)[0]
            cases.append(Case(f"{key}/n0", fn, [Ctx] + head + [enc, 0, Out(64), Out(1)]))
            at = len(head) + 1
            for pos, what in ((0, "ctx"), (at, "enc"), (at + 2, "out"), (at + 3, "ok")):
                args = [Ctx] + head + [enc, 3, Out(192), Out(3)]
                args[pos] = None
                cases.append(Case(f"{key}/null_{what}", fn, args))
            cases.append(Case(f"{key}/oversize", fn, [Ctx] + head + [enc, 1 << 31, Out(64), Out(1)]))
            cases.append(Case(f"{key}/null_and_oversize", fn, [Ctx] + head + [None, 1 << 31, Out(64), Out(1)]))
    return cases


# ------------------------------------------------------------------ maps of RFC 9380, from the vector files
def _coord(v, width):
    if isinstance(v, dict):
        return int(v["re"], 16).to_bytes(48, "little") + int(v["im"], 16).to_bytes(48, "little")
    return int(v, 16).to_bytes(width, "little")


def vectors(stem, variant, width):
    """[(field elements, P as x || y)] of one file"""
    with open(os.path.join(H2C, f"{stem}_{variant}.json")) as f:
        out = []
        for v in json.load(f)["vectors"]:
            try:
                out.append(([_coord(u, width) for u in v["u"]], _coord(v["P"]["x"], width) + _coord(v["P"]["y"], width)))
            except (KeyError, ValueError, OverflowError):
                continue
    assert len(out) >= 3, stem
    return out


MAPS = [   # (label, entry point, vector file, bytes per coordinate, modulus, takes `clear`, bytes per element, log2 of the exclusive limit)
    ("secp256k1_map_to_curve", "dr_secp256k1_map_to_curve", "secp256k1", 32, secp256k1_ref.P, False, 32, 30),
    ("p256_map_to_curve", "dr_p256_map_to_curve", "p256", 32, p256_ref.P, False, 32, 30),
    ("ed25519_map_to_curve", "dr_ed25519_map_to_curve", "ed25519", 32, ed25519_ref.P, False, 32, 30),
    ("curve25519_map_to_curve", "dr_curve25519_map_to_curve", "curve25519", 32, ed25519_ref.P, True, 32, 30),
    ("blsg1_map_to_curve", "dr_blsg1_map_to_curve", "bls12_381_G1", 48, bls12_381_g1_ref.P, True, 48, 29),
    ("blsg2_map_to_curve", "dr_blsg2_map_to_curve", "bls12_381_G2", 48, bls12_381_g2_ref.P, True, 96, 28),
    ("ed448_map_to_curve", "dr_ed448_map_to_curve", "ed448", 56, ed448_ref.P, True, 56, 28),
]


def map_cases():
    cases = []
    for label, fn, stem, width, p, takes_clear, elem, limit in MAPS:
        clear = [1] if takes_clear else []
        pt = 2 * elem if elem != 96 else 192
        for per_item, variant in ((2, "ro"), (1, "nu")):
            vecs = vectors(stem, variant, width)
            for n in (1, 3, 65):
                items = [vecs[i % len(vecs)] for i in range(n)]
                us = b"".join(b"".join(u) for u, _ in items)
                # (Curve25519's flag says "the identity", the others' "has an image")
                flag = b"\x00" if "curve25519" in label else b"\x01"
                cases.append(Case(f"{label}/per{per_item}_n{n}", fn, [Ctx, us, n, per_item] + clear + [Out(pt * n), Out(n)],
                                  {0: {i: items[i][1] for i in some(n)}, 1: {i: flag for i in some(n)}}, fresh=n == 65))
                if n == 65:
                    cases.append(Case(f"{label}/per{per_item}_n1_after_n65", fn, [Ctx, b"".join(items[1][0]), 1, per_item] + clear + [Out(pt), Out(1)],
                                      {0: items[1][1], 1: flag}))
        us = b"".join(b"".join(u) for u, _ in vectors(stem, "ro", width)[:3])
        tail = clear + [Out(3 * pt), Out(3)]
        cases.append(Case(f"{label}/n0", fn, [Ctx, us, 0, 2] + tail))
        for pos, what in ((0, "ctx"), (1, "us"), (4 + len(clear), "out"), (5 + len(clear), "ok")):
            args = [Ctx, us, 3, 2] + tail
            args[pos] = None
            cases.append(Case(f"{label}/null_{what}", fn, args))
        cases.append(Case(f"{label}/per_item3", fn, [Ctx, us, 2, 3] + tail))
        cases.append(Case(f"{label}/per_item3_and_null", fn, [Ctx, None, 2, 3] + tail))
        cases.append(Case(f"{label}/u_is_p", fn, [Ctx, p.to_bytes(width, "little") + us[width:], 3, 2] + tail))
        cases.append(Case(f"{label}/oversize", fn, [Ctx, us, 1 << limit, 1] + tail))
        cases.append(Case(f"{label}/null_and_oversize", fn, [Ctx, None, 1 << limit, 1] + tail))
    return cases


# ------------------------------------------------------------------ the field selftests and the Bandersnatch map
def limb_images(tag, n, limbs, bits, value_bits, parts=1):
    """n raw limb images of `parts` values below 2^value_bits each, `limbs` limbs of `bits` bits per value"""
    rng = random.Random(f"entry-surface/limbs/{tag}/{n}")
    out = b""
    for _ in range(n * parts):
        v = rng.getrandbits(value_bits)
        out += b"".join(((v >> (bits * j)) & ((1 << bits) - 1)).to_bytes(4, "little") for j in range(limbs))
    return out


SELFTESTS = [  # (entry point, limbs per value, bits per limb, value bits, values per operand, bytes per result, results per pair)
    ("dr_fe25519_ops_selftest", 9, 29, 250, 1, 32, 11), ("dr_p256_field_ops_selftest", 9, 29, 250, 1, 32, 12),
    ("dr_bjj_field_ops_selftest", 9, 29, 250, 1, 32, 12), ("dr_secp256k1_field_selftest", 9, 29, 250, 1, 32, 12),
    ("dr_blsg1_field_selftest", 14, 28, 380, 1, 48, 5), ("dr_blsg2_field_selftest", 14, 28, 380, 2, 96, 5),
    ("dr_ed448_field_selftest", 16, 28, 440, 1, 56, 11),
]

def selftest_cases():
    cases = []
    for fn, limbs, bits, vbits, parts, elem, recs in SELFTESTS:
        label = fn[3:]
        for n in (1, 3, 65):
            a, b = limb_images(label + "/a", n, limbs, bits, vbits, parts), limb_images(label + "/b", n, limbs, bits, vbits, parts)
            cases.append(Case(f"{label}/n{n}", fn, [Ctx, a, b, n, Out(n * recs * elem), Out(n)], fresh=n == 65))
        lb = 4 * limbs * parts                # a batch of one (the last pair of the 65) on the context that has just run the large one
        cases.append(Case(f"{label}/n1_after_n65", fn, [Ctx, a[-lb:], b[-lb:], 1, Out(recs * elem), Out(1)]))
        a, b = limb_images(label + "/a", 3, limbs, bits, vbits, parts), limb_images(label + "/b", 3, limbs, bits, vbits, parts)
        tail = [Out(3 * recs * elem), Out(3)]
        cases.append(Case(f"{label}/n0", fn, [Ctx, a, b, 0] + tail))
        for pos, what in ((0, "ctx"), (1, "a"), (2, "b"), (4, "out"), (5, "flags")):
            args = [Ctx, a, b, 3] + tail
            args[pos] = None
            cases.append(Case(f"{label}/null_{what}", fn, args))
        cases.append(Case(f"{label}/oversize", fn, [Ctx, a, b, 1 << 24] + tail))
        cases.append(Case(f"{label}/null_and_oversize", fn, [Ctx, None, b, 1 << 24] + tail))
    # dr_fr_ops_selftest: canonical elements of the BLS12-381 scalar field
    rng = random.Random("entry-surface/fr")
    fr = lambda n: b"".join(rng.randrange(bsn.P).to_bytes(32, "little") for _ in range(n))  # noqa: E731
    for n in (1, 3, 65):
        cases.append(Case(f"fr_ops_selftest/n{n}", "dr_fr_ops_selftest", [Ctx, fr(n), fr(n), n, Out(384 * n), Out(n)], fresh=n == 65))
    cases.append(Case("fr_ops_selftest/n1_after_n65", "dr_fr_ops_selftest", [Ctx, fr(1), fr(1), 1, Out(384), Out(1)]))
    a, b, tail = fr(3), fr(3), [Out(384 * 3), Out(3)]
    cases.append(Case("fr_ops_selftest/n0", "dr_fr_ops_selftest", [Ctx, a, b, 0] + tail))
    for pos, what in ((0, "ctx"), (1, "a"), (2, "b"), (4, "out"), (5, "is_square")):
        args = [Ctx, a, b, 3] + tail
        args[pos] = None
        cases.append(Case(f"fr_ops_selftest/null_{what}", "dr_fr_ops_selftest", args))
    cases.append(Case("fr_ops_selftest/a_is_p", "dr_fr_ops_selftest", [Ctx, bsn.P.to_bytes(32, "little") + a[32:], b, 3] + tail))
    cases.append(Case("fr_ops_selftest/oversize", "dr_fr_ops_selftest", [Ctx, a, b, 1 << 24] + tail))
    cases.append(Case("fr_ops_selftest/null_and_oversize", "dr_fr_ops_selftest", [Ctx, None, b, 1 << 24] + tail))
    return cases


def ell2_pair(u0, u1):
    """oracle/pyref: the sum of the two Elligator 2 images, times the cofactor 4"""
    def value():
        r = bsn.add(bsn.from_mont(*bsn.map_to_curve_ell2(u0)), bsn.from_mont(*bsn.map_to_curve_ell2(u1)))
        return coracle.te_pack([bsn.double(bsn.double(r))])
    return Lazy(value)


def bsn_encode_cases():
    cases, fn = [], "dr_bsn_encode_to_curve_batch"
    for n in (1, 3, 65):
        rng = random.Random(f"entry-surface/ell2/{n}")
        us = [(rng.randrange(bsn.P), rng.randrange(bsn.P)) for _ in range(n)]
        blob = b"".join(a.to_bytes(32, "little") + b.to_bytes(32, "little") for a, b in us)
        cases.append(Case(f"bsn_encode_to_curve_batch/n{n}", fn, [Ctx, blob, n, Out(64 * n)], {0: {i: ell2_pair(*us[i]) for i in some(n)}}))
    blob = b"".join(v.to_bytes(32, "little") for v in range(11, 17))
    cases.append(Case("bsn_encode_to_curve_batch/n0", fn, [Ctx, blob, 0, Out(64)]))
    for pos, what in ((0, "ctx"), (1, "us"), (3, "out")):
        args = [Ctx, blob, 3, Out(192)]
        args[pos] = None
        cases.append(Case(f"bsn_encode_to_curve_batch/null_{what}", fn, args))
    cases.append(Case("bsn_encode_to_curve_batch/u_is_p", fn, [Ctx, bsn.P.to_bytes(32, "little") + blob[32:], 3, Out(192)]))
    cases.append(Case("bsn_encode_to_curve_batch/oversize", fn, [Ctx, blob, 1 << 31, Out(64)]))
    cases.append(Case("bsn_encode_to_curve_batch/null_and_oversize", fn, [Ctx, None, 1 << 31, Out(64)]))
    # dr_te_scalar_mul_batch at the first n past the GLV branch, once: the C oracle's batch multiplication is the restatement
    g, n = BY_NAME["Bandersnatch"], 16384
    rng = random.Random("entry-surface/16384")
    pts = b"".join(g.raw(g.pool[i % POOL]) for i in range(n))
    sc = b"".join(rng.randrange(g.order).to_bytes(32, "little") for _ in range(n))
    cases.append(Case("te_scalar_mul_batch/Bandersnatch/n16384", "dr_te_scalar_mul_batch", [Ctx, 0, pts, sc, n, Out(64 * n)],
                      {0: Lazy(lambda: coracle.te_mul_batch_raw(pts, sc, n, glv=True))}))
    return cases


# ------------------------------------------------------------------ Curve25519: the identity inside the 64 bytes and as flag bytes
def curve25519_cases():
    g = BY_NAME["Curve25519_RO"]
    cases = []
    idx, ks, pts, sc = terms(g, 3, "identity")
    n_le = g.order.to_bytes(32, "little")
    # item 1 is the identity going in, item 2 comes out as the identity (its scalar is the order)
    pts_ff = pts[:64] + b"\xff" * 64 + pts[128:]
    sc_id = sc[:64] + n_le
    want = {0: g.times_g(ks[0] * 2), 1: g.identity, 2: g.identity}
    cases.append(Case("te_scalar_mul_batch/Curve25519_RO/identities", "dr_te_scalar_mul_batch", [Ctx, 13, pts_ff, sc_id, 3, Out(192)], {0: want}))
    cases.append(Case("te_msm_groups/Curve25519_RO/identities", "dr_te_msm_groups", [Ctx, 13, pts_ff, sc_id, 3, 1, Out(192)], {0: want}))
    cases.append(Case("te_msm/Curve25519_RO/identities", "dr_te_msm", [Ctx, 13, pts_ff, sc_id, 3, Out(64)], {0: want[0]}))
    flagged = {0: {0: want[0], 1: bytes(64), 2: bytes(64)}, 1: b"\x00\x01\x01"}
    fn = "dr_curve25519_scalar_mul_batch"
    cases.append(Case("curve25519_scalar_mul_batch/identities", fn, [Ctx, pts, b"\x00\x01\x00", sc_id, 3, Out(192), Out(3)], flagged))
    cases.append(Case("curve25519_scalar_mul_batch/no_flags_in", fn, [Ctx, pts, None, sc, 3, Out(192), Out(3)],
                      {0: {i: g.times_g(ks[i] * (idx[i] + 2)) for i in range(3)}, 1: bytes(3)}))
    cases.append(Case("curve25519_scalar_mul_batch/ff_is_refused", fn, [Ctx, pts_ff, bytes(3), sc, 3, Out(192), Out(3)]))
    idx65, ks65, pts65, sc65 = terms(g, 65, "flags")
    cases.append(Case("curve25519_scalar_mul_batch/n65", fn, [Ctx, pts65, bytes(65), sc65, 65, Out(64 * 65), Out(65)],
                      {0: {i: g.times_g(ks65[i] * (idx65[i] + 2)) for i in some(65)}, 1: bytes(65)}, fresh=True))
    cases.append(Case("curve25519_scalar_mul_batch/n1_after_n65", fn, [Ctx, pts[:64], b"\x01", sc[:32], 1, Out(64), Out(1)], {0: bytes(64), 1: b"\x01"}))
    cases.append(Case("curve25519_scalar_mul_batch/n0", fn, [Ctx, pts, bytes(3), sc, 0, Out(64), Out(1)]))
    for pos, what in ((0, "ctx"), (1, "pts"), (3, "scalars"), (5, "out"), (6, "id_out")):
        args = [Ctx, pts, bytes(3), sc, 3, Out(192), Out(3)]
        args[pos] = None
        cases.append(Case(f"curve25519_scalar_mul_batch/null_{what}", fn, args))
    cases.append(Case("curve25519_scalar_mul_batch/oversize", fn, [Ctx, pts, bytes(3), sc, 1 << 31, Out(64), Out(1)]))
    fn = "dr_curve25519_msm_groups"
    cases.append(Case("curve25519_msm_groups/identities", fn, [Ctx, pts, b"\x00\x01\x00", sc_id, 3, 1, Out(192), Out(3)], flagged))
    idx6, ks6, pts6, sc6 = terms(g, 6, "flag-groups")
    cases.append(Case("curve25519_msm_groups/m2", fn, [Ctx, pts6, bytes(6), sc6, 3, 2, Out(192), Out(3)], {0: group_sums(g, idx6, ks6, 3, 2), 1: bytes(3)}))
    idx64, ks64, pts64, sc64 = terms(g, 192, "flag-groups")
    cases.append(Case("curve25519_msm_groups/m64", fn, [Ctx, pts64, bytes(192), sc64, 3, 64, Out(192), Out(3)], {0: group_sums(g, idx64, ks64, 3, 64), 1: bytes(3)}))
    idx65, ks65, pts65, sc65 = terms(g, 65, "flag-groups")
    cases.append(Case("curve25519_msm_groups/groups65", fn, [Ctx, pts65, bytes(65), sc65, 65, 1, Out(64 * 65), Out(65)],
                      {0: {i: g.times_g(ks65[i] * (idx65[i] + 2)) for i in some(65)}, 1: bytes(65)}, fresh=True))
    cases.append(Case("curve25519_msm_groups/groups1_after_groups65", fn, [Ctx, pts[:64], b"\x01", sc[:32], 1, 1, Out(64), Out(1)], {0: bytes(64), 1: b"\x01"}))
    cases.append(Case("curve25519_msm_groups/groups0", fn, [Ctx, pts6, bytes(6), sc6, 0, 2, Out(64), Out(1)]))
    for pos, what in ((0, "ctx"), (1, "pts"), (3, "scalars"), (6, "out"), (7, "id_out")):
        args = [Ctx, pts6, bytes(6), sc6, 3, 2, Out(192), Out(3)]
        args[pos] = None
        cases.append(Case(f"curve25519_msm_groups/null_{what}", fn, args))
    cases.append(Case("curve25519_msm_groups/m0", fn, [Ctx, pts6, bytes(6), sc6, 3, 0, Out(192), Out(3)]))
    cases.append(Case("curve25519_msm_groups/m65", fn, [Ctx, pts6, bytes(6), sc6, 3, 65, Out(192), Out(3)]))
    cases.append(Case("curve25519_msm_groups/m0_and_null", fn, [Ctx, None, bytes(6), sc6, 3, 0, Out(192), Out(3)]))
    cases.append(Case("curve25519_msm_groups/oversize", fn, [Ctx, pts6, bytes(6), sc6, 1 << 31, 1, Out(64), Out(1)]))
    return cases


# ------------------------------------------------------------------ the wide suites: 48-, 96- and 56-byte coordinates
class Wide:
    def __init__(self, suite, mod, fe, scalar_bytes, has_groups, flagged_fn, flagged_gives_points, ro, nu, limit):
        self.suite, self.mod, self.fe, self.scalar_bytes, self.has_groups = suite, mod, fe, scalar_bytes, has_groups
        self.flagged_fn, self.flagged_gives_points, self.ro, self.nu = flagged_fn, flagged_gives_points, ro, nu
        self.p, self.g, self.limit = mod.P, mod.G, limit           # limit: log2 of max_points = max_decode (exclusive)
        self.order = getattr(mod, "R_ORDER", None) or mod.N
        self.pt_bytes = 4 * fe if suite == "blsg2" else 2 * fe
        self._pool = None

    def raw(self, pt):
        if pt is None:
            return bytes(self.pt_bytes)
        if self.suite == "blsg2":
            return b"".join(c.to_bytes(48, "little") for xy in pt for c in xy)
        return pt[0].to_bytes(self.fe, "little") + pt[1].to_bytes(self.fe, "little")

    @property
    def pool(self):
        if self._pool is None:
            pts = [self.mod.add(self.g, self.g)]
            while len(pts) < POOL:
                pts.append(self.mod.add(pts[-1], self.g))
            self._pool = pts
        return self._pool

    def times_g(self, a):
        return Lazy(lambda: self.raw(self.mod.mul(a % self.order, self.g)))

    def enc(self, pt):
        """what the flag-returning launch takes: G1's SEC1 compressed string, the others' x || y"""
        return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(48, "big") if self.suite == "blsg1" else self.raw(pt)


WIDES = [
    Wide("blsg1", bls12_381_g1_ref, 48, 32, True, "dr_blsg1_decode_points", True, 15, 16, 30),
    Wide("blsg2", bls12_381_g2_ref, 48, 96, False, "dr_blsg2_check_points", False, 17, 18, 28),
    Wide("ed448", ed448_ref, 56, 56, True, "dr_ed448_decode_points", True, 19, 20, 29),
]


def wide_terms(w, n, tag):
    rng = random.Random(f"entry-surface/{w.suite}/{tag}/{n}")
    idx = [i % POOL for i in range(n)]
    ks = [rng.getrandbits(8 * w.scalar_bytes) for _ in range(n)]
    return idx, ks, b"".join(w.raw(w.pool[j]) for j in idx), b"".join(k.to_bytes(w.scalar_bytes, "little") for k in ks)


def wide_cases():
    cases = []
    for w in WIDES:
        s, pb = w.suite, w.pt_bytes
        fn = f"dr_{s}_scalar_mul_batch"
        for n in (1, 3, 65):
            idx, ks, pts, sc = wide_terms(w, n, "mul")
            cases.append(Case(f"{s}_scalar_mul_batch/n{n}", fn, [Ctx, pts, sc, n, Out(pb * n)], {0: {i: w.times_g(ks[i] * (idx[i] + 2)) for i in some(n)}}))
        idx, ks, pts, sc = wide_terms(w, 3, "mul")
        cases.append(Case(f"{s}_scalar_mul_batch/n0", fn, [Ctx, pts, sc, 0, Out(pb)]))
        for pos, what in ((0, "ctx"), (1, "pts"), (2, "scalars"), (4, "out")):
            args = [Ctx, pts, sc, 3, Out(3 * pb)]
            args[pos] = None
            cases.append(Case(f"{s}_scalar_mul_batch/null_{what}", fn, args))
        x_is_p = w.p.to_bytes(w.fe, "little") + pts[w.fe:]
        cases.append(Case(f"{s}_scalar_mul_batch/x_is_p", fn, [Ctx, x_is_p, sc, 3, Out(3 * pb)]))
        cases.append(Case(f"{s}_scalar_mul_batch/oversize", fn, [Ctx, pts, sc, 1 << w.limit, Out(pb)]))
        cases.append(Case(f"{s}_scalar_mul_batch/null_and_oversize", fn, [Ctx, None, sc, 1 << w.limit, Out(pb)]))
        if w.has_groups:
            fn = f"dr_{s}_msm_groups"
            for m in (1, 2, 64):
                idx, ks, pts, sc = wide_terms(w, 3 * m, "groups")
                want = {q: w.times_g(sum(ks[q * m + j] * (idx[q * m + j] + 2) for j in range(m))) for q in range(3)}
                cases.append(Case(f"{s}_msm_groups/m{m}", fn, [Ctx, pts, sc, 3, m, Out(3 * pb)], {0: want}))
            idx, ks, pts, sc = wide_terms(w, 6, "groups")
            cases.append(Case(f"{s}_msm_groups/groups0", fn, [Ctx, pts, sc, 0, 2, Out(pb)]))
            for pos, what in ((0, "ctx"), (1, "pts"), (2, "scalars"), (5, "out")):
                args = [Ctx, pts, sc, 3, 2, Out(3 * pb)]
                args[pos] = None
                cases.append(Case(f"{s}_msm_groups/null_{what}", fn, args))
            cases.append(Case(f"{s}_msm_groups/m0", fn, [Ctx, pts, sc, 3, 0, Out(3 * pb)]))
            cases.append(Case(f"{s}_msm_groups/m65", fn, [Ctx, pts, sc, 3, 65, Out(3 * pb)]))
            cases.append(Case(f"{s}_msm_groups/m0_and_null", fn, [Ctx, None, sc, 3, 0, Out(3 * pb)]))
            cases.append(Case(f"{s}_msm_groups/oversize", fn, [Ctx, pts, sc, 1 << w.limit, 1, Out(pb)]))
        # ---- the flag-returning launch, both modes: points of the subgroup, with (1, 1) (off the curve) and a coordinate p at places 1 and 5
        fn, label = w.flagged_fn, w.flagged_fn[3:]
        off = w.enc(w.pool[0])[: len(w.enc(w.pool[0])) - 1] + b"\x01" if s != "blsg1" else b"\x02" + (1).to_bytes(48, "big")
        big = (b"\x02" + w.p.to_bytes(48, "big")) if s == "blsg1" else w.p.to_bytes(w.fe, "little") + w.raw(w.pool[0])[w.fe:]
        for check in (1, 0):
            for n in (1, 3, 65):
                encs = [w.enc(w.pool[i % POOL]) for i in range(n)]
                if n > 1:
                    encs[1] = off
                if n > 5 and s != "blsg2":            # (G2's check refuses a coordinate at or above p on the host: its own case below)
                    encs[5] = big
                good = [i for i in some(n) if i not in (1, 5)]
                outs = [Out(pb * n)] if w.flagged_gives_points else []
                expect = {len(outs): {i: b"\x01" for i in good}}
                if w.flagged_gives_points:
                    expect[0] = {i: w.raw(w.pool[i % POOL]) for i in good}
                cases.append(Case(f"{label}_check{check}/n{n}", fn, [Ctx, check, b"".join(encs), n] + outs + [Out(n)], expect, fresh=n == 65))
                if n == 65:
                    cases.append(Case(f"{label}_check{check}/n1_after_n65", fn, [Ctx, check, off, 1] + ([Out(pb)] if outs else []) + [Out(1)]))
        encs = b"".join(w.enc(w.pool[i]) for i in range(3))
        outs = [Out(3 * pb)] if w.flagged_gives_points else []
        cases.append(Case(f"{label}/n0", fn, [Ctx, 1, encs, 0] + outs + [Out(3)]))
        for pos, what in [(0, "ctx"), (2, "in")] + ([(4, "out"), (5, "ok")] if outs else [(4, "ok")]):
            args = [Ctx, 1, encs, 3] + outs + [Out(3)]
            args[pos] = None
            cases.append(Case(f"{label}/null_{what}", fn, args))
        cases.append(Case(f"{label}/x_is_p", fn, [Ctx, 1, big + encs[len(big):], 3] + outs + [Out(3)]))
        cases.append(Case(f"{label}/oversize", fn, [Ctx, 1, encs, 1 << w.limit] + outs + [Out(3)]))
        cases.append(Case(f"{label}/null_and_oversize", fn, [Ctx, 1, None, 1 << w.limit] + outs + [Out(3)]))
        # ---- hashing: hash_to_field on the host, the batch encoder through the map's launches
        msgs = [b"", b"abc", b"abcdef0123456789"]
        data, offs = b"".join(msgs), U64([0, 0, 3, 19])
        elem = 96 if s == "blsg2" else w.fe
        vec = {v: vectors({"blsg1": "bls12_381_G1", "blsg2": "bls12_381_G2", "ed448": "ed448"}[s], v, w.fe) for v in ("ro", "nu")}
        for variant, name, per in ((w.ro, "ro", 2), (w.nu, "nu", 1)):
            fn = f"dr_{s}_hash_to_field_batch"
            cases.append(Case(f"{s}_hash_to_field_batch/{name}", fn, [variant, data, offs, 3, Out(3 * per * elem)],
                              {0: {i: b"".join(vec[name][i][0]) for i in range(3)}}))
            fn = f"dr_{s}_encode_to_curve_batch"
            cases.append(Case(f"{s}_encode_to_curve_batch/{name}", fn, [Ctx, variant, data, offs, None, None, 3, Out(3 * pb)],
                              {0: {i: vec[name][i][1] for i in range(3)}}))
        cases.append(Case(f"{s}_encode_to_curve_batch/salted", f"dr_{s}_encode_to_curve_batch",
                          [Ctx, w.ro, data, offs, b"saltsalt", U64([0, 4, 4, 8]), 3, Out(3 * pb)]))
        other = WIDES[(WIDES.index(w) + 1) % 3].ro
        cases.append(Case(f"{s}_hash_to_field_batch/wrong_variant", f"dr_{s}_hash_to_field_batch", [other, data, offs, 3, Out(6 * elem)]))
        cases.append(Case(f"{s}_hash_to_field_batch/null_off", f"dr_{s}_hash_to_field_batch", [w.ro, data, None, 3, Out(6 * elem)]))
        cases.append(Case(f"{s}_hash_to_field_batch/null_out", f"dr_{s}_hash_to_field_batch", [w.ro, data, offs, 3, None]))
        cases.append(Case(f"{s}_hash_to_field_batch/null_msgs", f"dr_{s}_hash_to_field_batch", [w.ro, None, offs, 3, Out(6 * elem)]))
        cases.append(Case(f"{s}_hash_to_field_batch/decreasing", f"dr_{s}_hash_to_field_batch", [w.ro, data, U64([0, 5, 3, 19]), 3, Out(6 * elem)]))
        fn = f"dr_{s}_encode_to_curve_batch"
        cases.append(Case(f"{s}_encode_to_curve_batch/wrong_variant", fn, [Ctx, other, data, offs, None, None, 3, Out(3 * pb)]))
        cases.append(Case(f"{s}_encode_to_curve_batch/wrong_variant_and_null", fn, [Ctx, other, data, None, None, None, 3, Out(3 * pb)]))
        cases.append(Case(f"{s}_encode_to_curve_batch/count0", fn, [Ctx, w.ro, data, offs, None, None, 0, Out(pb)]))
        for pos, what in ((0, "ctx"), (2, "msgs"), (3, "off"), (7, "out")):
            args = [Ctx, w.ro, data, offs, None, None, 3, Out(3 * pb)]
            args[pos] = None
            cases.append(Case(f"{s}_encode_to_curve_batch/null_{what}", fn, args))
        cases.append(Case(f"{s}_encode_to_curve_batch/salts_without_offsets", fn, [Ctx, w.ro, data, offs, b"salt", None, 3, Out(3 * pb)]))
        cases.append(Case(f"{s}_encode_to_curve_batch/decreasing", fn, [Ctx, w.ro, data, U64([0, 5, 3, 19]), None, None, 3, Out(3 * pb)]))
    return cases


_TABLE = None


def table():
    """every case, in the order they run"""
    global _TABLE
    if _TABLE is None:
        _TABLE = te_cases() + decoder_cases() + map_cases() + selftest_cases() + bsn_encode_cases() + curve25519_cases() + wide_cases()
        assert len({c.key for c in _TABLE}) == len(_TABLE)
    return _TABLE


# the entry points the table must cover with at least one accepted (rc = 0, something launched or written) and one refused case
COVERED = sorted({
    "dr_te_scalar_mul_batch", "dr_te_msm_groups", "dr_te_msm", "dr_te_fixed_base_msm_groups", "dr_te_decode_points", "dr_bsn_encode_to_curve_batch",
    "dr_fr_ops_selftest", "dr_curve25519_scalar_mul_batch", "dr_curve25519_msm_groups"}
    | set(OWN_DECODERS.values()) | {m[1] for m in MAPS} | {s[0] for s in SELFTESTS}
    | {f"dr_{w.suite}_{op}" for w in WIDES for op in ("scalar_mul_batch", "hash_to_field_batch", "encode_to_curve_batch")}
    | {f"dr_{w.suite}_msm_groups" for w in WIDES if w.has_groups} | {w.flagged_fn for w in WIDES})


def load_golden():
    """{key: record}; the file nests the keys at their last "/" (one line per entry point and curve)"""
    with open(GOLDEN) as f:
        return {f"{head}/{case}": record for head, group in json.load(f).items() for case, record in group.items()}


def dump_golden(records, path):
    groups = {}
    for key, record in records.items():
        head, case = key.rsplit("/", 1)
        groups.setdefault(head, {})[case] = record
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(h)}: {json.dumps(g, sort_keys=True, separators=(',', ':'))}" for h, g in groups.items()) + "\n}\n")
