"""GPU: the four phases of the batched ring prover (dr_ring_prove_witness / _quotient / _evals / _openings) at CHOSEN challenges, against
the big-integer reference of ring_phase_ref.py.  Bit-exact, no tolerance.

Every other GPU test of the prover draws alphas, zeta and nus from the Fiat-Shamir transcript: 255-bit random values.  The cases of
ring_phase_cases.py put 0, 1, p - 1, one-hot vectors, limb boundaries and points of the domain there, where k_ring_eval, k_syndiv_*,
k_ring_lin_scalars, k_ring_aggpoly and the host glue (is_inf, empty MSM sets, the padding of the second opening quotient) branch or
degenerate.  In phase order a case compares the relation point and the four witness commitments, the peeked coefficient columns, C_q and
the peeked q, the eight evaluation words and the peeked lin, and both openings; None stands for the is_inf flag on both sides.
Commitments are compared with the reference's points, which over the known-tau SRS are f(tau) G by one scalar multiplication
(test_ring_phase_ref_cpu.py proves those equal to the MSM over the SRS at every case); the small batches also take the MSM.

One prover per curve at N = 512 (ring of 8 keys, one undecodable), module-scoped; the two big runs of a curve (the cases without hidden
rows, zk_rows = NULL, and those with) are made once and the tests of the phases read their records."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_phase_cases as rc  # noqa: E402
import ring_phase_ref as ref  # noqa: E402
from oracle.pyref import kzg as okzg  # noqa: E402
from oracle.pyref import ring as oring  # noqa: E402

pytestmark = pytest.mark.gpu
P = rc.P
# (curve, N) -> cases; the module's own count: a case that goes missing from the tables fails test_the_module_runs_every_case
CASES = {("bandersnatch", 512): 143, ("jubjub", 512): 143, ("bandersnatch", 1024): 28}


def _ints(raw):
    return [int.from_bytes(raw[i : i + 32], "little") for i in range(0, len(raw), 32)]


def _pt(p):
    return None if p is None else okzg.serialize(p)


class Device:
    """the product's Ring over the known-tau SRS and its device prover"""

    def __init__(self, curve, n):
        import dot_ring_amd as d
        from dot_ring_amd.ring_proof import device_prover
        from dot_ring_amd.ring_proof.pcs import SRS

        self.curve, self.n = curve, n
        self.ref = rc.reference(curve, n, by_tau=True)
        cv = {"bandersnatch": d.Bandersnatch, "jubjub": d.JubJub}[curve]
        srs = SRS.synthetic(rc.TAU, 3 * n + 1)
        o_srs = rc.known_tau_srs(n)
        assert srs.g1_points[1] == o_srs.g1[1] and srs.g1_points[3 * n] == o_srs.g1[3 * n]
        params = d.RingProofParams.from_ring_size(rc.RING_KEYS[n], cv=cv, pcs=d.KZG.with_srs(srs))
        assert params.domain_size == n and params.max_ring_size == self.ref.params.max_ring
        self.ring = d.Ring(self.ref.keys, params)
        root = d.RingRoot.from_ring(self.ring, params)
        assert root.encode() == self.ref.root.encode()
        self.prover = device_prover.get_device_prover(self.ring)
        fixed = _ints(self.prover.fixed_coeffs())
        self.fixed = [fixed[j * n : (j + 1) * n] for j in range(3)]
        assert self.fixed == [self.ref.root.px, self.ref.root.py, self.ref.root.s]
        self.records = {}

    def run(self, cases):
        """all four phases on one batch, with a peek after each of the first three; returns one record per proof"""
        dp, n, B = self.prover, self.n, len(cases)
        pinned = cases[0].witness.zk_rows is not None
        assert all((c.witness.zk_rows is not None) == pinned for c in cases)
        zk = b"".join(c.witness.zk_bytes() for c in cases) if pinned else None
        rel, wit = dp.witness([c.witness.producer for c in cases], b"".join(ref.le32(c.witness.blinding) for c in cases), zk)
        cols = _ints(dp.peek(dp.PEEK_COLUMNS, B))
        c_q = dp.quotient(B, b"".join(ref.le32(a) for c in cases for a in c.alphas))
        q = _ints(dp.peek(dp.PEEK_QUOTIENT, B))
        ev = _ints(dp.evals(B, b"".join(ref.le32(c.zeta) for c in cases)))
        lin = _ints(dp.peek(dp.PEEK_LIN, B))
        op = dp.openings(B, b"".join(ref.le32(v) for c in cases for v in c.nus))
        qn = 3 * n + 1
        return [dict(relation=(int.from_bytes(rel[64 * i : 64 * i + 32], "little"), int.from_bytes(rel[64 * i + 32 : 64 * i + 64], "little")),
                     commitments=wit[4 * i : 4 * i + 4], cols=[cols[(4 * i + j) * n : (4 * i + j + 1) * n] for j in range(4)],
                     c_q=c_q[i], q=q[i * qn : (i + 1) * qn], evals=ev[8 * i : 8 * i + 8], lin=lin[i * n : (i + 1) * n],
                     phi_z=op[2 * i], phi_zw=op[2 * i + 1]) for i in range(B)]

    def big_runs(self):
        """every case of the table: one batch without hidden rows, one with (for N = 512: 47 and 96 proofs)"""
        if not self.records:
            for cases in (self.ref.t.unpinned(), self.ref.t.pinned()):
                for c, rec in zip(cases, self.run(cases)):
                    self.records[c.name] = rec
        return self.records


_devices = {}


def _device(curve, n=512):
    if (curve, n) not in _devices:
        _devices[(curve, n)] = Device(curve, n)
    return _devices[(curve, n)]


@pytest.fixture(scope="module", params=rc.CURVES)
def dev(request):
    return _device(request.param)


@pytest.fixture(scope="module")
def dev1024():
    return _device("bandersnatch", 1024)


def _first_diff(got, want):
    return next((i for i, (a, b) in enumerate(zip(got, want)) if a != b), None)


PHASES = {
    "witness": ("relation", "commitments", "cols"),
    "quotient": ("c_q", "q"),
    "evals": ("evals", "lin"),
    "openings": ("phi_z", "phi_zw"),
}


def _mismatches(rec, r, fields):
    """names of what differs between a device record and the reference's snapshot, with the first differing coefficient of a polynomial"""
    want = dict(relation=tuple(r.relation), commitments=[_pt(c) for c in r.commitments], cols=r.cols, c_q=_pt(r.c_q), q=r.q,
                evals=list(r.evals) + [r.l_zw], lin=r.lin, phi_z=_pt(r.phi_z), phi_zw=_pt(r.phi_zw))
    out = []
    for f in fields:
        if rec[f] != want[f]:
            if f == "cols":
                out += [f"{ref.COLUMNS[j]}[{_first_diff(g, w)}]" for j, (g, w) in enumerate(zip(rec[f], want[f])) if g != w]
            elif f in ("q", "lin", "evals", "commitments"):
                out.append(f"{f}[{_first_diff(rec[f], want[f])}]")
            else:
                out.append(f"{f}: is_inf {rec[f] is None} for {want[f] is None}" if None in (rec[f], want[f]) else f)
    return out


def _check(D, cases, records, fields, R=None):
    R = R or D.ref
    bad = {}
    for c, rec in zip(cases, records):
        miss = _mismatches(rec, R.result(c), fields)
        if miss:
            bad[c.name] = miss
    assert not bad, bad


ALL = tuple(f for fs in PHASES.values() for f in fs)


def test_the_module_runs_every_case():
    for (curve, n), count in CASES.items():
        t = rc.tables(curve, n)
        assert len(t.cases) == count == rc.EXPECTED_COUNTS[n] and len(t.unpinned()) + len(t.pinned()) == count
        assert {c.kind for c in t.cases} == ({"alpha", "zeta", "nu", "product"} if n == 512 else {"zeta"})


@pytest.mark.parametrize("phase", list(PHASES))
def test_phase_at_every_case(dev, phase):
    """the whole table of a curve in two batches of 47 and 96 proofs (the second crosses the 64-lane blocks of k_ring_alpha_aux,
    k_ring_lin_scalars and k_syndiv_link), one phase's outputs per test"""
    records = dev.big_runs()
    cases = dev.ref.t.cases
    assert len(records) == len(cases) == CASES[(dev.curve, 512)]
    _check(dev, cases, [records[c.name] for c in cases], PHASES[phase])


def test_degenerate_results_are_flagged_on_the_device(dev):
    """is_inf and zero exactly where the case says so: q = 0 (zero alphas), lin = 0 (term = 0, alphas 0..2 zero), constant aggregate"""
    records = dev.big_runs()
    for c in dev.ref.t.cases:
        rec = records[c.name]
        got = {k for k, hit in (("c_q", rec["c_q"] is None), ("l_zw", rec["evals"][7] == 0), ("phi_z", rec["phi_z"] is None),
                                ("phi_zw", rec["phi_zw"] is None)) if hit}
        assert got == set(c.degenerate), c.name
        if "c_q" in c.degenerate:
            assert not any(rec["q"])
        if "phi_zw" in c.degenerate:
            assert not any(rec["lin"])


def test_commitments_are_the_polynomials_at_tau(dev):
    """through the known tau, with the DEVICE's own peeked polynomials: every commitment is f(tau) G for the f the device holds"""
    records = dev.big_runs()
    for c in dev.ref.t.cases:
        rec = records[c.name]
        assert rec["commitments"] == [_pt(rc.tau_commitment(col)) for col in rec["cols"]], c.name
        assert rec["c_q"] == _pt(rc.tau_commitment(rec["q"])), c.name
        zw = c.zeta * dev.ref.t.omega % P
        # phi_zw commits lin's quotient w: (tau - zeta w) w(tau) = lin(tau) - l(zeta w)
        den = (rc.TAU - zw) % P
        assert den
        w_tau = (rc.at_tau(rec["lin"]) - rec["evals"][7]) * pow(den, -1, P) % P
        assert rec["phi_zw"] == _pt(rc.coracle.g1_mul(okzg.G1_GEN, w_tau) if w_tau else None), c.name
        # phi_z commits the quotient of agg = sum nu_i f_i over px, py, s, the four columns and q: (tau - zeta) w(tau) = agg(tau) - agg(zeta)
        polys = dev.fixed + rec["cols"] + [rec["q"]]
        at_zeta = rec["evals"][:7] + [oring.horner(rec["q"], c.zeta)]
        den = (rc.TAU - c.zeta) % P
        if den:                                        # (zeta = tau is a case: there the quotient's value at tau is agg'(tau))
            num = sum(nu * (rc.at_tau(f) - v) for nu, f, v in zip(c.nus, polys, at_zeta)) % P
            w_tau = num * pow(den, -1, P) % P
            assert rec["phi_z"] == _pt(rc.coracle.g1_mul(okzg.G1_GEN, w_tau) if w_tau else None), c.name


@pytest.mark.parametrize("shape", ["one-empty", "one-empty-no-rows", "three", "seventeen-degenerate"])
def test_small_batches(dev, shape):
    """a batch of one whose three MSMs are all empty (with and without hidden rows), three proofs whose challenges differ in kind, and 17
    proofs that are all degenerate, so that the batched MSMs see zero scalars only; against the reference that commits by MSM over the SRS"""
    t = dev.ref.t
    cases = {"one-empty": lambda: t.batch_of_1(True), "one-empty-no-rows": lambda: t.batch_of_1(False), "three": t.batch_of_3,
             "seventeen-degenerate": t.batch_degenerate_17}[shape]()
    assert len(cases) == {"one-empty": 1, "one-empty-no-rows": 1, "three": 3, "seventeen-degenerate": 17}[shape]
    recs = dev.run(cases)
    _check(dev, cases, recs, ALL, rc.reference(dev.curve, 512))
    if shape != "three":
        assert all(r["c_q"] is None and r["phi_z"] is None and r["phi_zw"] is None for r in recs)
    assert dev.prover.residue() == 0


def test_batch_of_65_with_every_kind_of_case(dev):
    """every alpha, zeta and nu vector and every product once in ONE call, padded with random cases: per-proof indexing of alphas9,
    alpha_aux, ks, nus9, zetas and chunkv across the 64-lane blocks, above the 16 proofs from which the by-parts MSM sorts in LDS"""
    cases = dev.ref.t.batch_mixed_65()
    assert len(cases) == 65
    _check(dev, cases, dev.run(cases), ALL)
    # the same cases in another order give the same records: nothing depends on a proof's neighbours
    turned = cases[::-1]
    _check(dev, turned, dev.run(turned), ALL)


def test_zeta_edges_at_domain_1024(dev1024):
    """k_ring_eval with 4 and 13 coefficients per lane (N = 1024, ring of 300): the zeta edges alone"""
    t = dev1024.ref.t
    assert len(t.cases) == CASES[("bandersnatch", 1024)]
    for cases in (t.unpinned(), t.pinned()):
        assert len(cases) == 14
        _check(dev1024, cases, dev1024.run(cases), ALL)


def test_refusals_leave_the_state_untouched(dev):
    """a challenge equal to p is refused in each phase, and the phase called again with canonical challenges gives the reference's result;
    peek is refused before its phase, for an unknown selector, for a short buffer and after the openings, which wipe"""
    import ctypes

    from dot_ring_amd import _native

    dp, t = dev.prover, dev.ref.t
    cases = [t.by_name["alpha-random/random"], t.by_name["zeta-last-zero-nus/max-zero-max"]]
    B, n = 2, dev.n
    enc = lambda vals: b"".join(ref.le32(v) for v in vals)
    bad = lambda vals, at: b"".join(ref.le32(P if i == at else v) for i, v in enumerate(vals))
    rel, wit = dp.witness([c.witness.producer for c in cases], enc(c.witness.blinding for c in cases), b"".join(c.witness.zk_bytes() for c in cases))
    for what in (dp.PEEK_QUOTIENT, dp.PEEK_LIN, 3, -1):
        with pytest.raises(ValueError):
            dp.peek(what, B)
    cols = dp.peek(dp.PEEK_COLUMNS, B)
    short = ctypes.create_string_buffer(len(cols))
    assert _native.lib().dr_ring_prover_peek(dp.handle, dp.PEEK_COLUMNS, short, len(cols) - 1) == _native.DR_ERR_INVALID
    assert _native.lib().dr_ring_prover_peek(dp.handle, dp.PEEK_COLUMNS, None, len(cols)) == _native.DR_ERR_INVALID
    alphas = [a for c in cases for a in c.alphas]
    for at in (0, 13):
        with pytest.raises(ValueError):
            dp.quotient(B, bad(alphas, at))
    with pytest.raises(ValueError):
        dp.peek(dp.PEEK_QUOTIENT, B)                         # a refused phase has not run
    c_q = dp.quotient(B, enc(alphas))
    q = _ints(dp.peek(dp.PEEK_QUOTIENT, B))
    zetas = [c.zeta for c in cases]
    for at in (0, 1):
        with pytest.raises(ValueError):
            dp.evals(B, bad(zetas, at))
    with pytest.raises(ValueError):
        dp.peek(dp.PEEK_LIN, B)
    ev = _ints(dp.evals(B, enc(zetas)))
    lin = _ints(dp.peek(dp.PEEK_LIN, B))
    assert dp.peek(dp.PEEK_COLUMNS, B) == cols and _ints(dp.peek(dp.PEEK_QUOTIENT, B)) == q       # peeking changes nothing
    nus = [v for c in cases for v in c.nus]
    for at in (0, 15):
        with pytest.raises(ValueError):
            dp.openings(B, bad(nus, at))
    assert _ints(dp.peek(dp.PEEK_LIN, B)) == lin                # a refused last phase has not wiped
    op = dp.openings(B, enc(nus))
    qn, cw = 3 * n + 1, _ints(cols)
    recs = [dict(relation=(int.from_bytes(rel[64 * i : 64 * i + 32], "little"), int.from_bytes(rel[64 * i + 32 : 64 * i + 64], "little")),
                 commitments=wit[4 * i : 4 * i + 4], cols=[cw[(4 * i + j) * n : (4 * i + j + 1) * n] for j in range(4)], c_q=c_q[i],
                 q=q[i * qn : (i + 1) * qn], evals=ev[8 * i : 8 * i + 8], lin=lin[i * n : (i + 1) * n], phi_z=op[2 * i], phi_zw=op[2 * i + 1])
            for i in range(B)]
    _check(dev, cases, recs, ALL)
    for what in (dp.PEEK_COLUMNS, dp.PEEK_QUOTIENT, dp.PEEK_LIN):
        with pytest.raises(ValueError):
            dp.peek(what, B)
    assert dp.residue() == 0
