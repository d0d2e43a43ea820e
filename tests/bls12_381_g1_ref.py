"""Big-integer restatement of the reference's BLS12_381_G1_RO / BLS12_381_G1_NU (specs/bls12_381_G1.py over its generic short
Weierstrass point), written from RFC 9380 (section 5: hash_to_field by expand_message_xmd over SHA-256 with a 64-byte Z_pad and L = 64;
6.6.2: simplified SWU; 6.6.3 and appendix E.2: the 11-isogeny from E': y^2 = x^3 + A' x + B' to E: y^2 = x^3 + 4; 8.8.1: Z = 11 and
h_eff = 0xd201000000010001) and the reference's behaviour:

  the sum of two images (RO) or one image (NU) on E, then times h_eff;
  points in the generic SEC1 form: 0x02 / 0x03 by the parity of y and x in 48 bytes big-endian (49 bytes), 0x04 / 0x06 / 0x07 with
  both coordinates (97 bytes), b"\\x00" for the identity;
  valid_point: on the curve, not the identity, and r P = O.

Points are (x, y) tuples of E(Fp), the identity is None.  E(Fp) has order H * R_ORDER; a point of it need not lie in G1."""
import hashlib

P = 0x1A0111EA397FE69A4B1BA7B6434BACD764774B84F38512BF6730D2A0F6B0F6241EABFFFEB153FFFFB9FEFFFFFFFFAAAB
R_ORDER = 0x73EDA753299D7D483339D80809A1D80553BDA402FFFE5BFEFFFFFFFF00000001
H = 0x396C8C005555E1568C00AAAB0000AAAB           # the cofactor: #E(Fp) = H * R_ORDER
H_EFF = 0xD201000000010001                         # RFC 9380 8.8.1: what hashing multiplies by (the reference's `cofactor`)
CURVE_B = 4
G = (
    0x17F1D3A73197D7942695638C4FA9AC0FC3688C4F9774B905A14E3A3F171BAC586C55E83FF97A1AEFFB3AF00ADB22C6BB,
    0x08B3F481E3AAA0F1A09E30ED741D8AE4FCF5E095D5D00AF600DB18CB2C04B3EDD03CC744A2888AE40CAA232946C5E7E1,
)
DST_RO = b"QUUX-V01-CS02-with-BLS12381G1_XMD:SHA-256_SSWU_RO_"
DST_NU = b"QUUX-V01-CS02-with-BLS12381G1_XMD:SHA-256_SSWU_NU_"
SSWU_Z = 11
# E' and the isogeny's coefficient lists, lowest degree first as RFC 9380 appendix E.2 numbers them (k_(i,0), k_(i,1), ...); the two
# denominators are monic and their leading 1 is not listed
ISO_A = 0x144698a3b8e9433d693a02c96d4982b0ea985383ee66a8d8e8981aefd881ac98936f8da0e0f97f5cf428082d584c1d
ISO_B = 0x12e2908d11688030018b12e8753eee3b2016c1f0f24f4070a0b9c14fcef35ef55a23215a316ceaa5d1cc48e98e172be0
ISO_XNUM = (
    0x11a05f2b1e833340b809101dd99815856b303e88a2d7005ff2627b56cdb4e2c85610c2d5f2e62d6eaeac1662734649b7,
    0x17294ed3e943ab2f0588bab22147a81c7c17e75b2f6a8417f565e33c70d1e86b4838f2a6f318c356e834eef1b3cb83bb,
    0xd54005db97678ec1d1048c5d10a9a1bce032473295983e56878e501ec68e25c958c3e3d2a09729fe0179f9dac9edcb0,
    0x1778e7166fcc6db74e0609d307e55412d7f5e4656a8dbf25f1b33289f1b330835336e25ce3107193c5b388641d9b6861,
    0xe99726a3199f4436642b4b3e4118e5499db995a1257fb3f086eeb65982fac18985a286f301e77c451154ce9ac8895d9,
    0x1630c3250d7313ff01d1201bf7a74ab5db3cb17dd952799b9ed3ab9097e68f90a0870d2dcae73d19cd13c1c66f652983,
    0xd6ed6553fe44d296a3726c38ae652bfb11586264f0f8ce19008e218f9c86b2a8da25128c1052ecaddd7f225a139ed84,
    0x17b81e7701abdbe2e8743884d1117e53356de5ab275b4db1a682c62ef0f2753339b7c8f8c8f475af9ccb5618e3f0c88e,
    0x80d3cf1f9a78fc47b90b33563be990dc43b756ce79f5574a2c596c928c5d1de4fa295f296b74e956d71986a8497e317,
    0x169b1f8e1bcfa7c42e0c37515d138f22dd2ecb803a0c5c99676314baf4bb1b7fa3190b2edc0327797f241067be390c9e,
    0x10321da079ce07e272d8ec09d2565b0dfa7dccdde6787f96d50af36003b14866f69b771f8c285decca67df3f1605fb7b,
    0x6e08c248e260e70bd1e962381edee3d31d79d7e22c837bc23c0bf1bc24c6b68c24b1b80b64d391fa9c8ba2e8ba2d229,
)
ISO_XDEN = (
    0x8ca8d548cff19ae18b2e62f4bd3fa6f01d5ef4ba35b48ba9c9588617fc8ac62b558d681be343df8993cf9fa40d21b1c,
    0x12561a5deb559c4348b4711298e536367041e8ca0cf0800c0126c2588c48bf5713daa8846cb026e9e5c8276ec82b3bff,
    0xb2962fe57a3225e8137e629bff2991f6f89416f5a718cd1fca64e00b11aceacd6a3d0967c94fedcfcc239ba5cb83e19,
    0x3425581a58ae2fec83aafef7c40eb545b08243f16b1655154cca8abc28d6fd04976d5243eecf5c4130de8938dc62cd8,
    0x13a8e162022914a80a6f1d5f43e7a07dffdfc759a12062bb8d6b44e833b306da9bd29ba81f35781d539d395b3532a21e,
    0xe7355f8e4e667b955390f7f0506c6e9395735e9ce9cad4d0a43bcef24b8982f7400d24bc4228f11c02df9a29f6304a5,
    0x772caacf16936190f3e0c63e0596721570f5799af53a1894e2e073062aede9cea73b3538f0de06cec2574496ee84a3a,
    0x14a7ac2a9d64a8b230b3f5b074cf01996e7f63c21bca68a81996e1cdf9822c580fa5b9489d11e2d311f7d99bbdcc5a5e,
    0xa10ecf6ada54f825e920b3dafc7a3cce07f8d1d7161366b74100da67f39883503826692abba43704776ec3a79a1d641,
    0x95fc13ab9e92ad4476d6e3eb3a56680f682b4ee96f7d03776df533978f31c1593174e4b4b7865002d6384d168ecdd0a,
)
ISO_YNUM = (
    0x90d97c81ba24ee0259d1f094980dcfa11ad138e48a869522b52af6c956543d3cd0c7aee9b3ba3c2be9845719707bb33,
    0x134996a104ee5811d51036d776fb46831223e96c254f383d0f906343eb67ad34d6c56711962fa8bfe097e75a2e41c696,
    0xcc786baa966e66f4a384c86a3b49942552e2d658a31ce2c344be4b91400da7d26d521628b00523b8dfe240c72de1f6,
    0x1f86376e8981c217898751ad8746757d42aa7b90eeb791c09e4a3ec03251cf9de405aba9ec61deca6355c77b0e5f4cb,
    0x8cc03fdefe0ff135caf4fe2a21529c4195536fbe3ce50b879833fd221351adc2ee7f8dc099040a841b6daecf2e8fedb,
    0x16603fca40634b6a2211e11db8f0a6a074a7d0d4afadb7bd76505c3d3ad5544e203f6326c95a807299b23ab13633a5f0,
    0x4ab0b9bcfac1bbcb2c977d027796b3ce75bb8ca2be184cb5231413c4d634f3747a87ac2460f415ec961f8855fe9d6f2,
    0x987c8d5333ab86fde9926bd2ca6c674170a05bfe3bdd81ffd038da6c26c842642f64550fedfe935a15e4ca31870fb29,
    0x9fc4018bd96684be88c9e221e4da1bb8f3abd16679dc26c1e8b6e6a1f20cabe69d65201c78607a360370e577bdba587,
    0xe1bba7a1186bdb5223abde7ada14a23c42a0ca7915af6fe06985e7ed1e4d43b9b3f7055dd4eba6f2bafaaebca731c30,
    0x19713e47937cd1be0dfd0b8f1d43fb93cd2fcbcb6caf493fd1183e416389e61031bf3a5cce3fbafce813711ad011c132,
    0x18b46a908f36f6deb918c143fed2edcc523559b8aaf0c2462e6bfe7f911f643249d9cdf41b44d606ce07c8a4d0074d8e,
    0xb182cac101b9399d155096004f53f447aa7b12a3426b08ec02710e807b4633f06c851c1919211f20d4c04f00b971ef8,
    0x245a394ad1eca9b72fc00ae7be315dc757b3b080d4c158013e6632d3c40659cc6cf90ad1c232a6442d9d3f5db980133,
    0x5c129645e44cf1102a159f748c4a3fc5e673d81d7e86568d9ab0f5d396a7ce46ba1049b6579afb7866b1e715475224b,
    0x15e6be4e990f03ce4ea50b3b42df2eb5cb181d8f84965a3957add4fa95af01b2b665027efec01c7704b456be69c8b604,
)
ISO_YDEN = (
    0x16112c4c3a9c98b252181140fad0eae9601a6de578980be6eec3232b5be72e7a07f3688ef60c206d01479253b03663c1,
    0x1962d75c2381201e1a0cbd6c43c348b885c84ff731c4d59ca4a10356f453e01f78a4260763529e3532f6102c2e49a03d,
    0x58df3306640da276faaae7d6e8eb15778c4855551ae7f310c35a5dd279cd2eca6757cd636f96f891e2538b53dbf67f2,
    0x16b7d288798e5395f20d23bf89edb4d1d115c5dbddbcd30e123da489e726af41727364f2c28297ada8d26d98445f5416,
    0xbe0e079545f43e4b00cc912f8228ddcc6d19c9f0f69bbb0542eda0fc9dec916a20b15dc0fd2ededda39142311a5001d,
    0x8d9e5297186db2d9fb266eaac783182b70152c65550d881c5ecd87b6f0f5a6449f38db9dfa9cce202c6477faaf9b7ac,
    0x166007c08a99db2fc3ba8734ace9824b5eecfdfa8d0cf8ef5dd365bc400a0051d5fa9c01a58b1fb93d1a1399126a775c,
    0x16a3ef08be3ea7ea03bcddfabba6ff6ee5a4375efa1f4fd7feb34fd206357132b920f5b00801dee460ee415a15812ed9,
    0x1866c8ed336c61231a1be54fd1d74cc4f9fb0ce4c6af5920abc5750c4bf39b4852cfe2f7bb9248836b233d9d55535d4a,
    0x167a55cda70a6e1cea820597d94a84903216f763e13d87bb5308592e7ea7d4fbc7385ea3d529b35e346ef48bb8913f55,
    0x4d2f259eea405bd48f010a01ad2911d9c6dd039bb61a6290e591b36e636a5c871a5c29f4f83060400f8b49cba8f6aa8,
    0xaccbb67481d033ff5852c1e48c50c477f94ff8aefce42d28c0f9a88cea7913516f968986f7ebbea9684b529e2561092,
    0xad6b9514c767fe3c3613144b45f1496543346d98adf02267d5ceef9a00d9b8693000763e3b90ac11e99b138573345cc,
    0x2660400eb2e4f3b628bdd0d53cd76f2bf565b94e72927c1cb748df27942480e420517bd8714cc80d1fadc1326ed06f7,
    0xe0fa1d816ddc03e6b24255e0d7819c171c40f65e273b853324efcd6356caa205ca2f570f13497804415473a1d634b8f,
)
assert (len(ISO_XNUM), len(ISO_XDEN), len(ISO_YNUM), len(ISO_YDEN)) == (12, 10, 16, 15)
# Field elements whose SSWU image lies in the kernel of the isogeny (the 11-torsion subgroup of E' it divides out is rational): the x of
# sswu(u) is a root of both denominators, so iso_map raises.  Found by factoring the x-denominator over Fp and solving the map's
# quadratics for u; test_bls12_381_g1_cpu.py checks each one.  No message is known to hash to one.
KERNEL_US = (
    0x1377C0192D99508A317127ABF17C64205C7AAD448380027EFB47AE73EA231DBD6ECD3F2841B63D309C35BB8FD13E48F0,
    0xA2605E5991FCF3E63728A7A1468D79BACAA5F23F3816AADCD38EFDD330C6D4F5BBF450F92156E0E23E16E3252BCD042,
    0x146850B3BDC2495ED73BB803DFAA951A88ABFF0ACB5C7AEAC52B48F3C808E87CE3885B98CE916E17CAEF21A6CBC6B598,
    0xA92437E90BC473049AB549B4C4A145FEB4FB5CD39F7EE85C11FA62A8F5317220B398BE420CA5D8364D460F6EE1EFD29,
)


# ---------------------------------------------------------------- hash to field (RFC 9380 section 5)
def expand_message_xmd(msg, dst, length):
    dst_prime = dst + bytes([len(dst)])
    b0 = hashlib.sha256(bytes(64) + msg + length.to_bytes(2, "big") + b"\x00" + dst_prime).digest()
    blocks = [hashlib.sha256(b0 + b"\x01" + dst_prime).digest()]
    for i in range(2, -(-length // 32) + 1):
        blocks.append(hashlib.sha256(bytes(x ^ y for x, y in zip(b0, blocks[-1])) + bytes([i]) + dst_prime).digest())
    return b"".join(blocks)[:length]


def hash_to_field(msg, count, dst):
    raw = expand_message_xmd(msg, dst, 64 * count)
    return [int.from_bytes(raw[64 * i : 64 * i + 64], "big") % P for i in range(count)]


# ---------------------------------------------------------------- the group E(Fp): y^2 = x^3 + 4
def sqrt(v):
    """a root of v (p = 3 mod 4), None if v is no square"""
    r = pow(v, (P + 1) // 4, P)
    return r if r * r % P == v % P else None


def on_curve(pt):
    return pt is None or (pt[1] * pt[1] - pt[0] ** 3 - CURVE_B) % P == 0


def neg(pt):
    return None if pt is None else (pt[0], -pt[1] % P)


def add(p1, p2):
    if p1 is None:
        return p2
    if p2 is None:
        return p1
    if p1[0] == p2[0]:
        if (p1[1] + p2[1]) % P == 0:
            return None
        lam = 3 * p1[0] * p1[0] * pow(2 * p1[1], -1, P) % P
    else:
        lam = (p2[1] - p1[1]) * pow(p2[0] - p1[0], -1, P) % P
    x = (lam * lam - p1[0] - p2[0]) % P
    return x, (lam * (p1[0] - x) - p1[1]) % P


def mul(k, pt):
    """k pt for any integer k and any point of E(Fp) (no reduction of k: the point's order need not divide R_ORDER)"""
    if k < 0:
        return mul(-k, neg(pt))
    acc = None
    for bit in bin(k)[2:] if k else "":
        acc = add(acc, acc)
        if bit == "1":
            acc = add(acc, pt)
    return acc


def clear_cofactor(pt):
    return mul(H_EFF, pt)


def valid_point(pt):
    return pt is not None and on_curve(pt) and mul(R_ORDER, pt) is None


# ---------------------------------------------------------------- simplified SWU onto E' (RFC 9380 6.6.2) and the isogeny (E.2)
def sswu(u):
    """(x, y) on E'; tv1 = 0 (u = 0, and u^2 = -1 / Z) takes x1 = B' / (Z A')"""
    a, b, z = ISO_A, ISO_B, SSWU_Z
    tv1 = (z * z * pow(u, 4, P) + z * u * u) % P
    if tv1 == 0:
        x1 = b * pow(z * a % P, -1, P) % P
    else:
        x1 = -b * pow(a, -1, P) * (1 + pow(tv1, -1, P)) % P
    rhs = lambda x: (x * x * x + a * x + b) % P  # noqa: E731
    x, y = x1, sqrt(rhs(x1))
    if y is None:
        x = z * u * u * x1 % P
        y = sqrt(rhs(x))
    if u % 2 != y % 2:
        y = P - y
    return x, y


def _poly(coeffs, x, monic):
    acc = 1 if monic else 0
    for c in reversed(coeffs):
        acc = (acc * x + c) % P
    return acc


def iso_map(pt):
    """E' -> E; ValueError where a denominator vanishes (the reference's modular inverse raises there)"""
    x, y = pt
    xd, yd = _poly(ISO_XDEN, x, True), _poly(ISO_YDEN, x, True)
    if xd == 0 or yd == 0:
        raise ValueError("base is not invertible for the given modulus")
    return _poly(ISO_XNUM, x, False) * pow(xd, -1, P) % P, y * _poly(ISO_YNUM, x, False) * pow(yd, -1, P) % P


def map_to_curve(u):
    """map_to_curve_simple_swu: a point of E(Fp), before any cofactor clearing"""
    pt = iso_map(sswu(u))
    assert on_curve(pt)
    return pt


def map_sum(us, clear):
    acc = None
    for u in us:
        acc = add(acc, map_to_curve(u))
    return clear_cofactor(acc) if clear else acc


def encode_to_curve_ro(data):
    return map_sum(hash_to_field(data, 2, DST_RO), True)


def encode_to_curve_nu(data):
    return map_sum(hash_to_field(data, 1, DST_NU), True)


# ---------------------------------------------------------------- the SEC1 codec of the reference's short Weierstrass point
def sec1_encode(pt, compressed=True):
    if pt is None:
        return b"\x00"
    if compressed:
        return bytes([2 + (pt[1] & 1)]) + pt[0].to_bytes(48, "big")
    return b"\x04" + pt[0].to_bytes(48, "big") + pt[1].to_bytes(48, "big")


def sec1_decode(data):
    """string_to_point: a point, None for b"\\x00", 'bad' for what the reference refuses"""
    if len(data) == 0:
        return "bad"
    first = data[0]
    if first == 0:
        return None if len(data) == 1 else "bad"
    if first in (2, 3):
        if len(data) != 49:
            return "bad"
        x = int.from_bytes(data[1:], "big")
        if x >= P:
            return "bad"
        y = sqrt((x * x * x + CURVE_B) % P)
        if y is None:
            return "bad"
        return x, (y if y % 2 == first % 2 else P - y)
    if first in (4, 6, 7):
        if len(data) != 97:
            return "bad"
        x, y = int.from_bytes(data[1:49], "big"), int.from_bytes(data[49:], "big")
        if x >= P or y >= P or not on_curve((x, y)):
            return "bad"
        if first != 4 and y % 2 != first % 2:
            return "bad"
        return x, y
    return "bad"
