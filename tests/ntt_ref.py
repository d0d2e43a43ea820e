"""What the NTT tests share, in plain Python integers: roots of unity of Fr, seeded inputs, and the ring prover's element formats
restated from their descriptions (include/dotring_hip.h: dr_ntt_formats_selftest) without any of the device's helpers."""
import hashlib
import struct

P = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001       # the BLS12-381 scalar field
TWO_ADICITY = 32
G32 = pow(7, (P - 1) >> TWO_ADICITY, P)                                       # 7 generates Fr*: G32 has order exactly 2^32

STD8, FS9, STD8_SCALED, FS9_COSETS = 0, 1, 2, 3
R = 1 << 261                                                                  # an FS9 record of limb value v stands for v / R mod p
R_INV = pow(R, -1, P)
M29 = (1 << 29) - 1
# the input interval of the network's lazy bookkeeping (tests/native/ring_bounds_check.cpp, "ntt (constraint-kernel input)";
# csrc/ring_body.hip.h: body_constraints): limbs 0..7 within (-2^30, 2^30 + 2^29), |value| < 3.3 p
LIMB_LO, LIMB_HI = -(1 << 30), (1 << 30) + (1 << 29)
VALUE_BOUND = 33 * P // 10


def omega(log2n: int) -> int:
    """a primitive 2^log2n-th root of unity"""
    return pow(G32, 1 << (TWO_ADICITY - log2n), P)


def stream_elements(count: int, tag: bytes = b"dot-ring-amd ntt shapes") -> bytes:
    """count 32-byte little-endian elements from ONE SHAKE256 stream (a longer request extends a shorter one), the top two bits of
    each cleared: below 2^254 < p, so canonical"""
    raw = bytearray(hashlib.shake_256(tag).digest(32 * count))
    raw[31::32] = bytes(b & 0x3F for b in raw[31::32])
    return bytes(raw)


def b32(v: int) -> bytes:
    return v.to_bytes(32, "little")


def ints_of(raw: bytes) -> list:
    return [int.from_bytes(raw[i : i + 32], "little") for i in range(0, len(raw), 32)]


def first_diffs(got: bytes, want: bytes, rec: int = 32, limit: int = 8) -> str:
    """the first differing element indices of two record arrays (they name the pass and the tile that went wrong)"""
    if len(got) != len(want):
        return f"length {len(got)} != {len(want)}"
    bad, total = [], 0
    for i in range(0, len(got), 1 << 16):                       # whole chunks first: equal ones cost one memcmp
        if got[i : i + (1 << 16)] == want[i : i + (1 << 16)]:
            continue
        for j in range(i, min(i + (1 << 16), len(got)), rec):
            if got[j : j + rec] != want[j : j + rec]:
                total += 1
                if len(bad) < limit:
                    bad.append(j // rec)
    return f"{total} elements differ, first at {bad}"


# ---------------------------------------------------------------------------------------------- FS9 records
def fs9_limbs(v: int) -> list:
    """the carried image of a signed integer: limbs 0..7 in [0, 2^29), the rest in the signed top limb"""
    return [(v >> (29 * i)) & M29 for i in range(8)] + [v >> 232]


def fs9_value(limbs) -> int:
    return sum(l << (29 * i) for i, l in enumerate(limbs))


def fs9_pack(limbs) -> bytes:
    return struct.pack("<9i", *limbs)


def fs9_unpack(raw: bytes) -> list:
    """[nine signed limbs] per 36-byte record"""
    return [rec for rec in struct.iter_unpack("<9i", raw)]


def fs9_push(limbs, shifts) -> list:
    """Move shifts[i] * 2^29 units into limb i out of limb i + 1 (one unit of limb i + 1 is 2^29 of limb i: the value does not
    change), i = 0..7, each shift shortened towards zero until limb i lies strictly inside (LIMB_LO, LIMB_HI)."""
    out, borrowed = list(limbs), 0
    for i in range(8):
        t, base = shifts[i], out[i] - borrowed
        while not LIMB_LO < base + (t << 29) < LIMB_HI:
            t -= 1 if t > 0 else -1
        out[i], borrowed = base + (t << 29), t
    out[8] -= borrowed
    assert fs9_value(out) == fs9_value(limbs) and all(LIMB_LO < l < LIMB_HI for l in out[:8])
    return out


PUSH_PATTERNS = ([2] * 8, [-2] * 8, [2, -2] * 4, [-2, 2] * 4, [0] * 8, [1, -1, 2, -2, 0, 2, -1, 1])


def bound_records(count: int, tag: bytes):
    """count (record bytes, canonical record bytes, value it stands for) triples on the edges of the FS9 input contract: a residue x
    taken to x + m p, m = -3..3 (|x + m p| < 3.3 p), its limbs pushed to both ends of the limb range in every PUSH_PATTERNS way."""
    xs = ints_of(stream_elements(count, tag))
    edge = [0, 1, P - 1, (P - 1) // 2, (P + 1) // 2, VALUE_BOUND - 3 * P - 1]      # (the last: 3.3 p - 1 with m = 3)
    out = []
    for i, x in enumerate(xs):                                 # blocks of 42 = every m with every pattern; the first blocks on the edge residues
        x = edge[i // 42] if i < 42 * len(edge) else x % P
        m = i % 7 - 3
        if abs(x + m * P) >= VALUE_BOUND:                      # only m = 3 with x >= 0.3 p
            x %= VALUE_BOUND - 3 * P
        v = x + m * P
        assert abs(v) < VALUE_BOUND
        limbs = fs9_push(fs9_limbs(v), PUSH_PATTERNS[(i // 7) % len(PUSH_PATTERNS)])
        out.append((fs9_pack(limbs), fs9_pack(fs9_limbs(x)), x * R_INV % P))
    return out


def pick(count: int, pool_size: int, tag: bytes) -> list:
    """count seeded indices into a pool; the first pool_size of them visit every entry once, in strides that cross the pool's blocks"""
    assert pool_size % 211 and pool_size < 1 << 16
    raw = hashlib.shake_256(b"pick " + tag).digest(2 * count)
    return [(100 + i * 211) % pool_size if i < pool_size else int.from_bytes(raw[2 * i : 2 * i + 2], "little") % pool_size for i in range(count)]
