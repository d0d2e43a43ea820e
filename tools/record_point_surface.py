"""Record what the point types of dot_ring_amd.curve do, as JSON tables that tests/test_point_surface_cpu.py and
tests/test_gpu_point_surface.py recompute with the builders below and compare entry by entry:
    python tools/record_point_surface.py --cpu      -> tests/golden/point_surface_cpu.json   (host big-integer code only)
    python tools/record_point_surface.py --gpu      -> tests/golden/point_surface_gpu.json   (whatever launches a kernel)
(--out DIR writes there instead.)
The files were written once, at the commit before curve.py got its common base classes, and are not regenerated: a difference is a
change of behaviour.  Every call goes through outcome(), so an exception is recorded by type and message like any other result.
To keep the files small an entry is kept as its JSON text where that is short and as a digest of it otherwise (brief), and a variant
as its differences from the nearest earlier one (packed); a failing test prints the entry's full present value.
Only dot_ring_amd is imported.  Class internals that a refactor may add (private hooks, defaults) are not looked at; of an MRO the
public class names and the RFC 9380 mixins are kept."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import curve as C  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
NAMES = ["Bandersnatch", "Bandersnatch_SHAKE128", "JubJub", "Bandersnatch_SW", "Ed25519", "Ed25519_TAI", "Ed25519_RO", "Ed25519_NU",
         "P256", "P256_TAI", "P256_RO", "P256_NU", "BabyJubJub", "Secp256k1", "Secp256k1_RO", "Secp256k1_NU", "Curve25519",
         "Curve25519_RO", "Curve25519_NU", "BLS12_381_G1", "BLS12_381_G1_RO", "BLS12_381_G1_NU", "BLS12_381_G2", "BLS12_381_G2_RO",
         "BLS12_381_G2_NU", "Ed448", "Ed448_RO", "Ed448_NU"]
ALIASES = {"Ed25519": "Ed25519_TAI", "P256": "P256_TAI", "Secp256k1": "Secp256k1_RO", "Curve25519": "Curve25519_RO",
           "BLS12_381_G1": "BLS12_381_G1_RO", "BLS12_381_G2": "BLS12_381_G2_RO", "Ed448": "Ed448_RO"}
UNIQUE = [n for n in NAMES if n not in ALIASES]            # an alias is the same object: its tables would be copies
G1, G2, ED448 = ("BLS12_381_G1_RO", "BLS12_381_G1_NU"), ("BLS12_381_G2_RO", "BLS12_381_G2_NU"), ("Ed448_RO", "Ed448_NU")
SW = ("Bandersnatch_SW", "P256_TAI", "P256_RO", "P256_NU", "Secp256k1_RO", "Secp256k1_NU") + G1     # integer short Weierstrass
SEC1 = ("P256_RO", "P256_NU", "Secp256k1_RO", "Secp256k1_NU") + G1                                  # point_to_string(compressed=)


def is_point(v) -> bool:
    return hasattr(v, "is_identity") and hasattr(v, "x") and hasattr(v, "y")


def show(v):
    if is_point(v):
        return repr(v)
    if isinstance(v, (bytes, bytearray)):
        return "hex:" + bytes(v).hex()
    if isinstance(v, (list, tuple)):
        return [show(e) for e in v]
    if v is None or isinstance(v, (bool, int, str)):
        return v
    return repr(v)


def outcome(f, *args, **kw):
    try:
        return show(f(*args, **kw))
    except Exception as exc:  # noqa: BLE001 — the record is of whatever happens
        return {"exc": type(exc).__name__, "msg": str(exc)}


def detail(f):
    """a point with its repr, hash and predicates"""
    try:
        pt = f()
        return {"repr": repr(pt), "hash": hash(pt), "is_identity": pt.is_identity(), "is_on_curve": pt.is_on_curve()}
    except Exception as exc:  # noqa: BLE001
        return {"exc": type(exc).__name__, "msg": str(exc)}


class _Reached(Exception):
    pass


class _NoDevice:
    """stands in for the context: the first library entry point called on it ends the call and is the outcome"""

    def __getattr__(self, name):
        def stop(*args, **kw):
            brief = lambda v: (f"{len(v)} bytes" if isinstance(v, (bytes, bytearray)) else repr(v) if isinstance(v, (int, str, bool)) or v is None  # noqa: E731
                               else f"{type(v).__name__} of {len(v)}" if isinstance(v, (list, tuple)) else type(v).__name__)
            raise _Reached(f"{name}({', '.join([brief(v) for v in args] + [f'{k}={brief(v)}' for k, v in kw.items()])})")
        return stop


def reached(f, *args):
    """which library entry point a call goes to first, and with how much: the branch the Python dispatch takes, without a device"""
    real = C.runtime.context
    C.runtime.context = _NoDevice
    try:
        return outcome(f, *args)
    finally:
        C.runtime.context = real


def variant(name):
    return getattr(d, name)


def multiples(cls):
    """G, 2G, 3G, 5G, -G, G - G by host +, double (where the class has one) and - only"""
    g = cls.generator_point()
    g2 = g.double() if hasattr(g, "double") else g + g
    g3 = g2 + g
    return {"G": g, "2G": g2, "3G": g3, "5G": g3 + g2, "-G": -g, "G-G": g - g}


def modulus(cls) -> int:
    return cls.curve.params.field_modulus


def coord_len(cls) -> int:
    return (modulus(cls).bit_length() + 7) // 8


# ------------------------------------------------------------------ the CPU record
def _rhs(cls, x):
    return (x * x * x + cls._SW_A * x + cls._SW_B) % modulus(cls)


def _is_square(v, p):
    return v == 0 or pow(v, (p - 1) // 2, p) == 1


def cv_sqrt(cls, v):
    p = modulus(cls)
    return pow(v, (p + 1) // 4, p) if p % 4 == 3 else cls.curve.mod_sqrt(v)


def malformed(name, cls):
    """the fixed list of inputs to string_to_point: (case, input)"""
    g, p, n = cls.generator_point(), modulus(cls), coord_len(cls)
    cases = [("empty", b""), ("empty_str", "")]
    if name in G2:
        return cases + [("any", b"\x02" + bytes(96))]
    good = outcome(g.point_to_string)
    if isinstance(good, str) and good.startswith("hex:") and name not in G1:     # (G1's own string is compressed: the decode kernel)
        cases.append(("hex_str", good[4:]))
        cases.append(("bytearray", bytearray(bytes.fromhex(good[4:]))))
    if name in SW:
        be = lambda v: int(v).to_bytes(n, "big")  # noqa: E731
        le = lambda v: int(v).to_bytes(n, "little")  # noqa: E731
        noroot = next(x for x in range(1, 1000) if not _is_square(_rhs(cls, x), p))
        for pre in (0x02, 0x03, 0x04, 0x06, 0x07):
            cases.append((f"sec1_{pre:02x}_short", bytes([pre]) + be(g.x)[:-1]))
            cases.append((f"sec1_{pre:02x}_long", bytes([pre]) + be(g.x) + b"\x00"))
            cases.append((f"sec1_{pre:02x}_5bytes", bytes([pre]) + bytes(4)))
        cases += [
            ("sec1_00", b"\x00"), ("sec1_00_trailing", b"\x00\x00"), ("sec1_00_long", b"\x00" + be(g.x)),
            ("sec1_02_x_p", b"\x02" + be(p)), ("sec1_03_x_p1", b"\x03" + be(p + 1)),
            ("sec1_04_G", b"\x04" + be(g.x) + be(g.y)), ("sec1_04_negG", b"\x04" + be(g.x) + be(p - g.y)),
            ("sec1_04_x_p", b"\x04" + be(p) + be(g.y)), ("sec1_04_x_p1", b"\x04" + be(p + 1) + be(g.y)),
            ("sec1_04_y_p", b"\x04" + be(g.x) + be(p)), ("sec1_04_off_curve", b"\x04" + be(g.x) + be((g.y + 1) % p)),
            ("sec1_04_zeros", b"\x04" + bytes(2 * n)),
            ("hybrid_match", bytes([0x06 + g.y % 2]) + be(g.x) + be(g.y)),
            ("hybrid_wrong_parity", bytes([0x07 - g.y % 2]) + be(g.x) + be(g.y)),
            ("hybrid_off_curve", bytes([0x06 + (g.y + 1) % 2]) + be(g.x) + be((g.y + 1) % p)),
            ("hybrid_x_p", b"\x06" + be(p) + be(g.y)),
        ]
        if name not in G1:                      # on G1 a compressed x below p goes to the decode kernel: the GPU record has those
            cases += [("sec1_02_G", b"\x02" + be(g.x)), ("sec1_03_G", b"\x03" + be(g.x)),
                      ("sec1_02_no_root", b"\x02" + be(noroot)), ("sec1_03_no_root", b"\x03" + be(noroot)),
                      ("sec1_02_x_0", b"\x02" + be(0))]
            # the 33-byte canonical codecs: x little-endian, then a flag byte
            for flag in (0x00, 0x80, 0x01, 0x40, 0xC0, 0x3F, 0x41):
                cases.append((f"flag_{flag:02x}_G", le(g.x) + bytes([flag])))
                cases.append((f"flag_{flag:02x}_zeros", bytes(n) + bytes([flag])))
            cases += [("flag_x_p", le(p) + b"\x00"), ("flag_x_p1", le(p + 1) + b"\x80"), ("flag_no_root", le(noroot) + b"\x00"),
                      ("flag_short", le(g.x)), ("flag_long", le(g.x) + b"\x00\x00"), ("flag_40_nonzero", le(1) + b"\x40")]
            # a canonical string that starts with a SEC1 marker byte (P-256 reads it canonically first): k G with x = 2 or 3 mod 256
            pt = g
            for _ in range(600):
                pt = pt + g
                if pt.x % 256 in (2, 3):
                    cases.append(("flag_00_starts_sec1", le(pt.x) + b"\x00"))
                    cases.append(("flag_80_starts_sec1", le(pt.x) + b"\x80"))
                    cases.append(("sec1_of_that_point", bytes([2 + pt.y % 2]) + be(pt.x)))
                    break
    else:
        # twisted Edwards (y with a sign bit, or x || y), Montgomery (u || v): little-endian strings
        le = lambda v: int(v).to_bytes(n, "little")  # noqa: E731
        cases += [
            ("le_y_p", le(p)), ("le_y_p1", le(p + 1)), ("le_y_G_sign_flipped", le(g.y ^ (1 << (8 * n - 1)))),
            ("le_xy_G", le(g.x) + le(g.y)), ("le_xy_off_curve", le(g.x) + le((g.y + 1) % p)), ("le_xy_x_p", le(p) + le(g.y)),
            ("le_xy_y_p", le(g.x) + le(p)), ("le_xy_zeros", bytes(2 * n)), ("le_xy_ff", b"\xff" * (2 * n)),
            ("le_short", le(g.y)[:-1]), ("le_long", le(g.x) + le(g.y) + b"\x00"), ("le_y_0", le(0)), ("le_y_1", le(1)),
        ]
        cases += [(f"le_y_{v}", le(v)) for v in range(2, 8)]         # some have no x
    return cases


def prefix_sweep(cls):
    """every first byte in front of G's big-endian x: {outcome with the byte's own hex digits blanked: [bytes]}"""
    g, n, table = cls.generator_point(), coord_len(cls), {}
    for b in range(256):
        if b in (0x02, 0x03):
            continue                                            # a well-formed compressed string: among the named cases
        out = outcome(cls.string_to_point, bytes([b]) + int(g.x).to_bytes(n, "big"))
        key = json.dumps(out, sort_keys=True).replace(f"0x{b:02x}", "0x__")
        table.setdefault(key, []).append(b)
    return table


def constructors(name, cls):
    g, p = cls.generator_point(), modulus(cls)
    bump = (lambda v: v + 1) if name in G2 else (lambda v: (v + 1) % p)
    table = {
        "G": outcome(cls, g.x, g.y), "x_p": outcome(cls, p, g.y), "y_p": outcome(cls, g.x, p), "x_negative": outcome(cls, -1, g.y),
        "x_none": outcome(cls, None, g.y), "y_none": outcome(cls, g.x, None), "both_none": outcome(cls, None, None),
        "off_curve": outcome(cls, g.x, bump(g.y)), "zeros": outcome(cls, 0, 0), "zero_one": outcome(cls, 0, 1),
        "identity": detail(cls.identity), "generator_point": detail(cls.generator_point),
    }
    if name in G2:
        table["tuples"] = outcome(cls, g.x.to_tuple(), g.y.to_tuple())
        table["wrong_field"] = outcome(cls, C.Fp2(1, 2, 7), g.y)
    return table


def cpu_variant(name):
    cv = variant(name)
    cls = cv.point_type
    rec = {
        "class": cls.__name__,
        "mro": [c.__name__ for c in cls.__mro__ if c is not object and (not c.__name__.startswith("_") or "Rfc9380" in c.__name__)],
        "N": cls._N, "H": cls._H, "CV": cls._CV, "curve_id": cv.curve.params.curve_id, "curve_is_variants": cls.curve is cv.curve,
        "slots_no_dict": not hasattr(cls.generator_point(), "__dict__"),
    }
    pts = multiples(cls)
    rec["multiples"] = {k: detail(lambda v=v: v) for k, v in pts.items()}
    rec["laws"] = {
        "2G==G+G": pts["2G"] == pts["G"] + pts["G"], "3G-G": outcome(lambda: pts["3G"] - pts["G"]),
        "G+identity": outcome(lambda: pts["G"] + cls.identity()), "identity+G": outcome(lambda: cls.identity() + pts["G"]),
        "G+(-G)": outcome(lambda: pts["G"] + pts["-G"]), "-identity": outcome(lambda: -cls.identity()),
        "identity.double": outcome(lambda: cls.identity().double()), "G+int": outcome(lambda: pts["G"] + 1),
        "G-int": outcome(lambda: pts["G"] - 1), "G==tuple": pts["G"] == (pts["G"].x, pts["G"].y), "G!=2G": pts["G"] != pts["2G"],
        "in_set": len({pts["G"], cls.generator_point(), pts["2G"]}),
    }
    # -- the codec, every flavour of compressed=
    codec = {}
    for k, pt in list(pts.items()) + [("identity", cls.identity())]:
        flavours = {"default": outcome(pt.point_to_string)}
        if name in SEC1:
            flavours["compressed"] = outcome(pt.point_to_string, compressed=True)
            flavours["uncompressed"] = outcome(pt.point_to_string, compressed=False)
            flavours["positional_false"] = outcome(pt.point_to_string, False)
        for fl, s in flavours.items():
            entry = {"string": s}
            gpu_decode = name in G1 and isinstance(s, str) and s[4:6] in ("02", "03")       # the decode kernel: the GPU record
            if isinstance(s, str) and s.startswith("hex:") and not gpu_decode:
                entry["back"] = outcome(cls.string_to_point, bytes.fromhex(s[4:]))
            codec[f"{k}/{fl}"] = entry
    rec["codec"] = codec
    rec["malformed"] = {case: outcome(cls.string_to_point, data) for case, data in malformed(name, cls)}
    if name in SEC1:
        rec["prefix_sweep"] = prefix_sweep(cls)
    rec["constructors"] = constructors(name, cls)
    # -- the host map_to_curve (the wide types' runs a kernel)
    if hasattr(cls, "map_to_curve") and name not in ED448:
        rec["map_to_curve"] = {str(k): outcome(cls.map_to_curve, u) for k, u in (("0", 0), ("1", 1), ("2", 2), ("p-1", modulus(cls) - 1))}
    if cls._H in (1, 4, 8):
        rec["clear_cofactor"] = {k: outcome(pt.clear_cofactor) if hasattr(pt, "clear_cofactor") else "absent" for k, pt in pts.items()}
        if cls._H == 1:
            rec["clear_cofactor"]["G_is_self"] = pts["G"].clear_cofactor() is pts["G"]
    # -- the packers of the 64-byte ABI, round trips with the identity inside
    trio = [pts["G"], cls.identity(), pts["2G"]]
    packed = outcome(C.pack_points, trio)
    rec["pack"] = {"pack_points": packed, "pack_points_flagged": outcome(C.pack_points_flagged, trio)}
    if isinstance(packed, str):
        raw = bytes.fromhex(packed[4:])
        rec["pack"]["unpack_points"] = outcome(C.unpack_points, cls, raw)
        rec["pack"]["round_trip"] = outcome(lambda: C.unpack_points(cls, raw) == trio)
        rec["pack"]["unpack_zeros"] = outcome(C.unpack_points, cls, bytes(64))
        rec["pack"]["unpack_ff"] = outcome(C.unpack_points, cls, b"\xff" * 64)
        flagged = C.pack_points_flagged(trio)
        rec["pack"]["unpack_points_flagged"] = outcome(C.unpack_points_flagged, cls, *flagged)
    rec["pack"]["pack_scalars"] = outcome(C.pack_scalars, [0, 1, -1, cls._N, cls._N + 5], cls._N)
    # -- the dispatch to the library: the first entry point each call reaches
    g, n = pts["G"], cls._N
    cyc = [pts["G"], pts["2G"], pts["3G"], pts["5G"]]
    rec["dispatch"] = {
        "mul": reached(lambda: g * 3), "mul_negative": reached(lambda: g * -3), "mul_wide": reached(lambda: g * (1 << 300)),
        "scalar_mul_batch_distinct": reached(C.scalar_mul_batch, cyc[:3], [3, 5, n + 7]),
        "scalar_mul_batch_same_generator": reached(C.scalar_mul_batch, [g, g, g], [3, 5, n + 7]),
        "scalar_mul_batch_equal_generators": reached(C.scalar_mul_batch, [g, cls.generator_point(), g], [3, 5, 7]),
        "scalar_mul_batch_wide_scalar": reached(C.scalar_mul_batch, cyc[:2], [3, 1 << 300]),
        "msm_groups_m2": reached(C.msm_groups, cyc, [1, 2, 3, 4], 2), "msm_groups_m65": reached(C.msm_groups, cyc * 17, list(range(68)), 68),
        "valid_points": reached(C.valid_points, [g, cls.identity(), pts["2G"]]), "valid_point": reached(cv.curve.valid_point, g),
        "encode_to_curve": reached(cls.encode_to_curve, b"m", b"s"), "encode_to_curve_batch": reached(cls.encode_to_curve_batch, [b"m", b"n"]),
        "public_key_from_secret": reached(cv.public_key_from_secret, bytes([7]) * 32),
    }
    bb = cv.curve.params.auxiliary_points.blinding_base
    if bb:
        rec["dispatch"]["scalar_mul_batch_same_blinding_base"] = reached(lambda: C.scalar_mul_batch([cls(*bb)] * 3, [3, 5, 7]))
    if name not in G2:                               # (G2 has no MSM entry point)
        rec["dispatch"].update({f"msm_{m}": reached(cls.msm, [cyc[i % 4] for i in range(m)], list(range(1, m + 1))) for m in (1, 3, 65)})
    if hasattr(cls, "encode_to_curve_from_field"):
        rec["dispatch"]["from_field"] = reached(lambda: cls.encode_to_curve_from_field(cls.hash_to_field_pairs([b"m", b"n"])))
    if hasattr(cls, "map_to_curve_simple_swu"):
        rec["dispatch"]["map_to_curve_simple_swu"] = reached(cls.map_to_curve_simple_swu, C.Fp2(1, 2, modulus(cls)) if name in G2 else 5)
    if name in ED448:
        rec["dispatch"]["map_to_curve"] = reached(cls.map_to_curve, 5)
    if name in G1 + G2:
        rec["dispatch"]["clear_cofactor"] = reached(g.clear_cofactor)
    if name in G1:
        rec["dispatch"]["string_to_point_compressed"] = reached(cls.string_to_point, g.point_to_string())
    # -- CurveVariant.point
    rec["variant_point"] = {
        "tuple": outcome(cv.point, (g.x, g.y)), "two_args": outcome(cv.point, g.x, g.y), "point": outcome(cv.point, g),
        "point_is_same": cv.point(g) is g, "foreign_point": outcome(cv.point, d.Bandersnatch.point_type.generator_point()),
        "off_curve": outcome(cv.point, (g.x, g.x)), "name": cv.name, "point_type_name": cv.point_type.__name__,
    }
    return rec


def cpu_cross():
    """what the 28 exported variants are to each other"""
    gens = [variant(n).point_type.generator_point() for n in NAMES]
    ids = [variant(n).point_type.identity() for n in NAMES]
    both = gens + ids
    rec = {
        "aliases": {n: variant(n) is variant(ALIASES.get(n, n)) for n in NAMES},
        "equality": {f"{'G' if i < 28 else 'O'}:{NAMES[i % 28]}": "".join("1" if a == b else "0" for b in both) for i, a in enumerate(both)},
        "inequality": {f"{'G' if i < 28 else 'O'}:{NAMES[i % 28]}": "".join("1" if a != b else "0" for b in both) for i, a in enumerate(both)},
        "hash_equal": {NAMES[i]: "".join("1" if hash(a) == hash(b) else "0" for b in gens) for i, a in enumerate(gens)},
    }
    add, sub, add_id = {}, {}, {}
    for i, a in enumerate(gens):
        for j, b in enumerate(gens):
            if NAMES[i] in ALIASES or NAMES[j] in ALIASES:
                continue
            add.setdefault(NAMES[i], {})[NAMES[j]] = outcome(lambda: a + b)
            if i != j and NAMES[j] in ("Bandersnatch", "P256_TAI", "Curve25519_RO", "BLS12_381_G2_RO"):
                sub.setdefault(NAMES[i], {})[NAMES[j]] = outcome(lambda: a - b)
                add_id.setdefault(NAMES[i], {})[NAMES[j]] = outcome(lambda: a + ids[j])
    rec["add"], rec["sub"], rec["add_identity"] = add, sub, add_id
    return rec


def cpu_table():
    return {**{n: cpu_variant(n) for n in UNIQUE}, "cross": cpu_cross()}


# ------------------------------------------------------------------ the GPU record
def outside_subgroup(name, cls):
    """a point of the curve outside the prime-order subgroup, None where the curve has prime order"""
    g, p = cls.generator_point(), modulus(cls)
    if cls._H == 1:
        return None
    if name in G2:
        return cls.map_to_curve_simple_swu(C.Fp2(1, 2, p))
    if name in SW:                                   # the first x with a point (a point of E is outside the subgroup in general)
        x = next(x for x in range(1, 1000) if _is_square(_rhs(cls, x), p))
        y = cv_sqrt(cls, _rhs(cls, x))
        return cls(x, min(y, p - y))
    if name.startswith("Curve25519"):
        return g + cls(0, 0)                         # the point of order 2
    return g + cls(0, p - 1)                         # twisted Edwards: (0, -1) has order 2


def gpu_variant(name):
    cv = variant(name)
    cls = cv.point_type
    pts = multiples(cls)
    g, n = pts["G"], cls._N
    rec = {}
    ks = {"0": 0, "1": 1, "2": 2, "n-1": n - 1, "n": n, "n+1": n + 1, "-1": -1}
    if name in G1:
        ks.update({"2^256": 1 << 256, "hr+1": cls._COFACTOR * n + 1})
    if name in G2:
        ks["2^768"] = 1 << 768
    rec["mul"] = {k: outcome(lambda v=v: g * v) for k, v in ks.items()}
    rec["rmul"] = outcome(lambda: 3 * g)
    rec["mul_identity"] = outcome(lambda: cls.identity() * 5)
    rec["scalar_mul_batch"] = {
        "distinct": outcome(C.scalar_mul_batch, [pts["G"], pts["2G"], pts["3G"]], [3, 5, n + 7]),
        "same_generator": outcome(C.scalar_mul_batch, [g, g, g], [3, 5, n + 7]),
        "equal_generators": outcome(C.scalar_mul_batch, [g, cls.generator_point(), g], [3, 5, 7]),
        "with_identity": outcome(C.scalar_mul_batch, [g, cls.identity()], [2, 3]),
        "empty": outcome(C.scalar_mul_batch, [], []), "lengths": outcome(C.scalar_mul_batch, [g], [1, 2]),
    }
    bb = cv.curve.params.auxiliary_points.blinding_base
    if bb:
        b = outcome(cls, *bb)
        rec["scalar_mul_batch"]["same_blinding_base"] = b if isinstance(b, dict) else outcome(lambda: C.scalar_mul_batch([cls(*bb)] * 3, [3, 5, 7]))
    if name not in G2:                               # (G2 has no MSM entry point)
        cyc = [pts["G"], pts["2G"], pts["3G"], pts["5G"]]
        terms = lambda m: ([cyc[i % 4] for i in range(m)], [(i * i + 1) * (n // 7) + i for i in range(m)])  # noqa: E731
        rec["msm"] = {str(m): outcome(cls.msm, *terms(m)) for m in (0, 1, 3, 65)}
        rec["msm"]["lengths"] = outcome(cls.msm, [g], [1, 2])
        rec["msm"]["with_identity"] = outcome(cls.msm, [g, cls.identity(), pts["2G"]], [2, 3, -1])
        rec["msm_groups"] = {"m2x4": outcome(C.msm_groups, *terms(4), 2), "empty": outcome(C.msm_groups, [], [], 2)}
        if name in ED448:
            rec["msm_groups"]["m65"] = outcome(C.msm_groups, *terms(65), 65)
    out = outcome(outside_subgroup, name, cls)
    rec["outside_subgroup"] = out
    trio = [g, cls.identity()] + ([outside_subgroup(name, cls)] if isinstance(out, str) else [])
    rec["valid_points"] = outcome(C.valid_points, trio)
    rec["valid_points_empty"] = outcome(C.valid_points, [])
    rec["valid_point_G"] = outcome(cv.curve.valid_point, g)
    rec["valid_point_identity"] = outcome(cv.curve.valid_point, cls.identity())
    if name in G1 + G2:
        rec["clear_cofactor"] = {"G": outcome(g.clear_cofactor), "outside": outcome(lambda: trio[2].clear_cofactor())}
    # -- hashing to the curve
    msgs, salts = [b"point surface 0", b"point surface 1"], [b"salt-0", b""]
    h2c = {
        "encode_to_curve": outcome(cls.encode_to_curve, msgs[0]), "encode_to_curve_salt": outcome(cls.encode_to_curve, msgs[0], salts[0]),
        "batch": outcome(cls.encode_to_curve_batch, msgs), "batch_salts": outcome(cls.encode_to_curve_batch, msgs, salts),
        "batch_empty": outcome(cls.encode_to_curve_batch, []),
    }
    if hasattr(cls, "hash_to_field_pairs"):
        us = outcome(cls.hash_to_field_pairs, msgs, salts)
        h2c["hash_to_field_pairs"] = us
        if isinstance(us, str):
            h2c["from_field"] = outcome(cls.encode_to_curve_from_field, bytes.fromhex(us[4:]))
        h2c["from_field_empty"] = outcome(cls.encode_to_curve_from_field, b"")
    us = [0, 1, 2]
    if name in G2:
        us = [C.Fp2(0, 0, modulus(cls)), C.Fp2(1, 0, modulus(cls)), C.Fp2(2, 1, modulus(cls))]
    if hasattr(cls, "map_to_curve_simple_swu"):
        h2c["map_to_curve_simple_swu"] = [outcome(cls.map_to_curve_simple_swu, u) for u in us]
    if name in ED448:
        h2c["map_to_curve"] = [outcome(cls.map_to_curve, u) for u in us + [3]]
    rec["h2c"] = h2c
    rec["public_key_from_secret"] = outcome(cv.public_key_from_secret, (12345).to_bytes(32, "little"))
    rec["public_key_from_secret_type"] = outcome(cv.public_key_from_secret, 5)
    if name in G1:                                   # compressed strings: the decode kernel
        be = lambda v: int(v).to_bytes(48, "big")  # noqa: E731
        noroot = next(x for x in range(1, 1000) if not _is_square(_rhs(cls, x), modulus(cls)))
        rec["compressed_decode"] = {
            k: outcome(cls.string_to_point, s) for k, s in (
                ("02_G", b"\x02" + be(g.x)), ("03_G", b"\x03" + be(g.x)), ("own_G", g.point_to_string()), ("own_negG", pts["-G"].point_to_string()),
                ("own_5G", pts["5G"].point_to_string()), ("02_no_root", b"\x02" + be(noroot)), ("03_no_root", b"\x03" + be(noroot)),
                ("02_x_0", b"\x02" + be(0)), ("02_hex_str", (b"\x02" + be(g.x)).hex()))}
    return rec


def gpu_table():
    return {n: gpu_variant(n) for n in UNIQUE}


# ------------------------------------------------------------------ the files: small enough to read, one line per variant
def entries(tree):
    """{"section/case": value} of one variant's table: what is compared, one by one"""
    out = {}
    for section, val in tree.items():
        if isinstance(val, dict) and "exc" not in val:
            out.update({f"{section}/{case}": v for case, v in val.items()})
        else:
            out[section] = val
    return out


def brief(value, own: str) -> str:
    """an entry as the file keeps it: its JSON text where that is short, else eight hex digits of its SHA-256.  The variant's own class
    name is blanked first (the entry `class` keeps it), so that the RO and NU variants of a suite share most entries"""
    text = json.dumps(value, sort_keys=True).replace(own, "<cls>")
    return text if len(text) <= 18 else "#" + hashlib.sha256(text.encode()).hexdigest()[:8]


def briefed(name, tree):
    return {k: v if k == "class" else brief(v, f"{name}Point") for k, v in entries(tree).items()}


def packed(tables):
    """{name: briefed entries} with each table written as its differences (null: absent) from the earlier table nearest to it"""
    out, done = {}, {}
    for name, tab in tables.items():
        cost = lambda base: sum(tab.get(k) != v for k, v in done[base].items()) + sum(k not in done[base] for k in tab)  # noqa: E731
        base = min(done, key=cost, default=None)
        if base is None or cost(base) > len(tab) // 2:
            out[name] = {"set": tab}
        else:
            diff = {k: v for k, v in tab.items() if done[base].get(k) != v}
            diff.update({k: None for k in done[base] if k not in tab})
            out[name] = {"like": base, "set": diff}
        done[name] = tab
    return out


def load(kind):
    """{name: briefed entries} from the file"""
    with open(os.path.join(GOLDEN, f"point_surface_{kind}.json")) as f:
        stored = json.load(f)
    out = {}
    for name, rec in stored.items():
        tab = {**out.get(rec.get("like"), {}), **rec["set"]}
        out[name] = {k: v for k, v in tab.items() if v is not None}
    return out


def write(tables, path):
    stored = packed({name: briefed(name, tree) for name, tree in tables.items()})
    with open(path, "w") as f:
        f.write("{\n" + ",\n".join(f"{json.dumps(n)}: {json.dumps(rec, sort_keys=True, separators=(',', ':'))}" for n, rec in stored.items()) + "\n}\n")
    print(f"{path}: {os.path.getsize(path)} bytes, {sum(len(entries(t)) for t in tables.values())} entries")


def main():
    kinds = [a[2:] for a in sys.argv[1:] if a in ("--cpu", "--gpu")]
    if not kinds:
        raise SystemExit(__doc__)
    out_dir = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else GOLDEN
    os.makedirs(out_dir, exist_ok=True)
    for kind in kinds:
        write(cpu_table() if kind == "cpu" else gpu_table(), os.path.join(out_dir, f"point_surface_{kind}.json"))


if __name__ == "__main__":
    main()
