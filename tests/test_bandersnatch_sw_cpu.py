"""Bandersnatch_SW without a GPU: the Python codec against the suite's vectors and the big-integer restatement (sw_ref.py),
every rejection rule of the decoder, the SW <-> TE maps, and the ring-proof refusal."""
import glob
import json
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import sw_ref as r  # noqa: E402

import dot_ring_amd as d  # noqa: E402
from dot_ring_amd import _native  # noqa: E402

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FILES = sorted(glob.glob(os.path.join(GOLDEN, "*", "bandersnatch_sw_sha*_tai_*.json")))


def test_eight_vector_files():
    assert len(FILES) == 8


@pytest.mark.parametrize("path", FILES, ids=lambda p: "/".join(p.split(os.sep)[-2:]))
def test_codec_round_trips_pk_and_h(path):
    P = d.Bandersnatch_SW.point_type
    for e in json.load(open(path)):
        for key in ("pk", "h", "gamma"):
            enc = bytes.fromhex(e[key])
            pt = P.string_to_point(enc)
            assert (pt.x, pt.y) == r.decode(enc)
            assert pt.point_to_string() == enc and len(enc) == 33


def _pt():
    return r.mul(12345, r.G)


def _nonsquare_x():
    x = 1
    while r.sqrt(x ** 3 + r.A * x + r.B) is not None:
        x += 1
    return x


@pytest.mark.parametrize("case", ["inf", "inf_neg", "low_bit", "x_ge_p", "nonsquare"])
def test_rejections(case):
    P = d.Bandersnatch_SW.point_type
    good = r.encode(_pt())
    enc = {
        "inf": bytes(32) + b"\x40",
        "inf_neg": bytes(32) + b"\xc0",
        "low_bit": good[:32] + bytes([good[32] | 0x01]),
        "x_ge_p": (r.P + 1).to_bytes(32, "little") + b"\x00",
        "nonsquare": _nonsquare_x().to_bytes(32, "little") + b"\x00",
    }[case]
    with pytest.raises(ValueError):
        P.string_to_point(enc)
    assert r.decode(enc) is None


def test_each_low_flag_bit_rejected():
    good = r.encode(_pt())
    for bit in range(6):
        enc = good[:32] + bytes([good[32] | (1 << bit)])
        with pytest.raises(ValueError, match="flags"):
            d.Bandersnatch_SW.point_type.string_to_point(enc)


def test_two_torsion_has_y_zero_and_no_encoding():
    # the cubic splits: three points of order 2, all with y = 0, which _y_recover refuses
    roots = _cubic_roots()
    assert len(roots) == 3
    for x in roots:
        with pytest.raises(ValueError):
            d.Bandersnatch_SW.point_type.string_to_point(x.to_bytes(32, "little") + b"\x00")


def _cubic_roots():
    # the SW 2-torsion is the image of the Montgomery model's: s = 0 and the two roots of s^2 + A_M s + 1, x = (s + A3) / MB
    a, dd = r.TE_A % r.P, r.TE_D
    am = 2 * (a + dd) * pow(a - dd, -1, r.P) % r.P
    disc = r.sqrt(am * am - 4)
    half = pow(2, -1, r.P)
    roots = {(s + r.A3) * pow(r.MB, -1, r.P) % r.P for s in (0, (-am + disc) * half % r.P, (-am - disc) * half % r.P)}
    assert all((x ** 3 + r.A * x + r.B) % r.P == 0 for x in roots)
    return sorted(roots)


def test_maps_send_generator_to_te_generator_and_back():
    assert r.to_te(r.G) == tuple(d.Bandersnatch.curve.params.generator)
    assert r.from_te(tuple(d.Bandersnatch.curve.params.generator)) == r.G


def test_blinding_base_maps_to_point_of_order_n():
    bt = r.to_te(r.BLINDING)
    assert bt != (0, 1) and r.te_mul(r.N, bt) == (0, 1)
    assert tuple(d.Bandersnatch_SW.curve.params.auxiliary_points.blinding_base) == r.BLINDING


def test_suite_parameters():
    sp = d.Bandersnatch_SW.curve.params
    assert sp.suite_id == b"Bandersnatch-SW-SHA512-TAI-v1" and sp.encoding.point_len == 33
    assert sp.curve_id == _native.CURVE_BANDERSNATCH_SW == 2 and sp.subgroup_order == r.N and sp.cofactor == 4
    assert "Bandersnatch_SW" in d.__all__


def test_host_group_law_matches_restatement():
    P = d.Bandersnatch_SW.point_type
    p1, p2 = r.mul(7, r.G), r.mul(11, r.G)
    a, b = P(*p1), P(*p2)
    assert ((a + b).x, (a + b).y) == r.add(p1, p2)
    assert (a.double().x, a.double().y) == r.double(p1)
    assert (a - a).is_identity() and (a + P.identity()) == a
    assert P.identity().point_to_string() == bytes(32) + b"\x40"


def test_ring_params_refuse_sw():
    with pytest.raises(ValueError, match="ring proofs require a Twisted Edwards curve"):
        d.RingProofParams(cv=d.Bandersnatch_SW)
