"""CPU: the phase-wise reference of the ring prover (ring_phase_ref.py) and its case tables (ring_phase_cases.py), before
test_gpu_ring_phases.py holds the device phases against them.

  * with the Fiat-Shamir challenges the four functions give oracle.pyref.ring.prove_ring's 592 bytes;
  * at every chosen-challenge case they give the bytes of prove_ring with FsTranscript.challenges overridden to return the case's values;
  * the quotient as a linear combination of the seven per-constraint quotients equals the one divided out of the aggregate;
  * over the known-tau SRS every commitment is f(tau) G (infinity where f(tau) = 0 because f = 0) and every opening quotient satisfies
    (tau - z) w(tau) = f(tau) - f(z): the reference is not right only by agreeing with a restatement of itself;
  * the tables meet their own conditions, and the degenerate results appear exactly where a case says so."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_phase_cases as rc  # noqa: E402
import ring_phase_ref as ref  # noqa: E402
from oracle.pyref import bandersnatch as bsn  # noqa: E402
from oracle.pyref import ring as oring  # noqa: E402

P = rc.P
TABLES = [(cv, 512) for cv in rc.CURVES] + [("bandersnatch", 1024)]
KINDS = ("alpha", "zeta", "nu", "product")


@pytest.fixture
def chosen_challenges():
    """install(alphas, zeta, nus): prove_ring then draws these instead of hashing; the transcript's own method comes back afterwards"""
    original = oring.FsTranscript.challenges
    chosen = {}

    def challenges(self, label, n):
        out = list(chosen[label])
        assert len(out) == n
        return out

    def install(alphas, zeta, nus):
        chosen.update({b"constraints_aggregation": alphas, b"evaluation_point": (zeta,), b"kzg_aggregation": nus})
        oring.FsTranscript.challenges = challenges

    try:
        yield install
    finally:
        oring.FsTranscript.challenges = original


def _oracle_proof(R, w):
    """prove_ring for a table's witness: test-vector parameters where the witness has no hidden rows, pinned rows otherwise"""
    with bsn.using(R.suite):
        if w.zk_rows is None:
            return oring.prove_ring(R.ring_tv, R.root_tv, R.keys[w.producer], w.blinding)
        return oring.prove_ring(R.ring, R.root, R.keys[w.producer], w.blinding, w.zk_rows)


@pytest.mark.parametrize("curve,n", TABLES)
def test_tables_are_the_fixed_lists(curve, n):
    t = rc.tables(curve, n)
    assert len(t.cases) == rc.EXPECTED_COUNTS[n] == len(t.by_name)
    again = rc.Tables(curve, n)
    assert [(c.name, c.alphas, c.zeta, c.nus) for c in again.cases] == [(c.name, c.alphas, c.zeta, c.nus) for c in t.cases]
    assert len(t.zetas) == 14 and len(t.nus) == 11 and len(t.alphas) == 19
    z = dict(t.zetas)
    dom = [pow(t.omega, i, P) for i in range(n)]
    assert z["w^-1"] * t.omega % P == 1 and z["last"] == dom[n - 4] and [z[f"hidden-{i}"] for i in range(3)] == dom[n - 3 :]
    assert pow(z["w4n"], 4 * n, P) == 1 and pow(z["w4n"], n, P) != 1 and z["tau"] == rc.TAU and z["max"] == P - 1 and z["half"] * 2 + 1 == P
    a = dict(t.alphas)
    assert {a[f"limb-{k + 1}-0"][0] for k in (29, 58, 232, 252)} == {1 << k for k in (29, 58, 232, 252)}
    assert {a[f"limb-{k}-1"][0] for k in (29, 58, 232, 252)} == {(1 << k) - 1 for k in (29, 58, 232, 252)}
    assert a["000rrrr"][:3] == (0, 0, 0) and len(set(a["000rrrr"][3:])) == 1 and a["000rrrr"][3]
    ws = t.witnesses
    assert ws["none"].zk_rows is None and {w.kind for w in ws.values()} == {"none", "random", "edge"}
    edge = {0, 1, P - 1, (P - 1) // 2, (P + 1) // 2}
    assert all(set(v for col in w.zk_rows.values() for v in col) <= edge for w in ws.values() if w.kind == "edge")
    assert {w.blinding for w in ws.values()} == {1, t.order - 1, 1 << (t.order.bit_length() - 1), int("55" * 32, 16) % t.order}
    assert {w.producer for w in ws.values()} == {0, rc.RING_KEYS[n] - 1}
    if n == 512:
        # every challenge vector meets the three kinds of witness
        for kind, names in (("alpha", a), ("zeta", z), ("nu", dict(t.nus))):
            for name in names:
                assert {c.witness.kind for c in t.cases if c.name.startswith(f"{kind}-{name}/")} == {"none", "random", "edge"}, (kind, name)
        assert len(t.batch_mixed_65()) == 65 and len(t.batch_degenerate_17()) == 17 and len(t.batch_of_3()) == 3
        groups = {c.name.split("/")[0] for c in t.pinned()}
        assert groups == {c.name.split("/")[0] for c in t.batch_mixed_65()}
        assert all(c.witness.zk_rows is not None for c in t.batch_mixed_65() + t.batch_degenerate_17() + t.batch_of_3())
        assert len({c.kind for c in t.batch_of_3()}) > 1


@pytest.mark.parametrize("curve,n", TABLES)
def test_phases_with_the_transcript_challenges_give_prove_ring(curve, n):
    R = rc.reference(curve, n)
    for w in R.t.witnesses.values():
        if n != 512 and w.name not in ("none", "max-zero-max"):
            continue
        with bsn.using(R.suite):
            got = ref.prove_with_transcript(R.state(w.name))
        assert got == _oracle_proof(R, w), w.name


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("curve,n", TABLES)
def test_phases_at_chosen_challenges_give_prove_ring(curve, n, kind, chosen_challenges):
    R = rc.reference(curve, n)
    cases = [c for c in R.t.cases if c.kind == kind]
    assert cases or n != 512
    for c in cases:
        got = R.result(c).payload
        chosen_challenges(c.alphas, c.zeta, c.nus)
        assert got == _oracle_proof(R, c.witness), c.name


@pytest.mark.parametrize("curve", rc.CURVES)
def test_quotient_from_the_constraint_quotients_equals_the_direct_one(curve):
    R = rc.reference(curve, 512)
    a = dict(R.t.alphas)
    for wn in ("none", "random", "all-max"):
        st = R.state(wn)
        with bsn.using(R.suite):
            for an in ("random", "max", "e1", "zero"):
                saved = st.commit
                st.commit = lambda coeffs: None                     # the polynomial alone
                try:
                    q, _ = ref.quotient(st, a[an])
                finally:
                    st.commit = saved
                assert q == ref.quotient_direct(st, a[an]) and len(q) == 3 * 512 + 1, (wn, an)
                assert any(q) == (an != "zero")


@pytest.mark.parametrize("curve,n", TABLES)
def test_commitments_and_openings_through_the_known_tau(curve, n):
    R = rc.reference(curve, n)
    tau, w = rc.TAU, R.t.omega
    for name in R.t.witnesses:
        st = R.state(name)
        assert st.commitments == [rc.tau_commitment(c) for c in st.cols] and None not in st.commitments
        assert len(st.cols) == 4 and all(len(c) == n for c in st.cols)
    for c in R.t.cases:
        r = R.result(c)
        assert len(r.q) == 3 * n + 1 and len(r.lin) == n and len(r.agg) == 3 * n + 1 and len(r.w1) == 3 * n and len(r.w2) == n - 1
        assert r.c_q == rc.tau_commitment(r.q) and r.phi_z == rc.tau_commitment(r.w1) and r.phi_zw == rc.tau_commitment(r.w2), c.name
        assert (tau - c.zeta) * rc.at_tau(r.w1) % P == (rc.at_tau(r.agg) - oring.horner(r.agg, c.zeta)) % P, c.name
        zw = c.zeta * w % P
        assert (tau - zw) * rc.at_tau(r.w2) % P == (rc.at_tau(r.lin) - r.l_zw) % P and r.l_zw == oring.horner(r.lin, zw), c.name
        # the commitment by one scalar multiplication, which the GPU module's reference uses, is the same point
        assert rc.tau_commitment(r.q) == r.c_q


@pytest.mark.parametrize("curve,n", TABLES)
def test_degenerate_results_appear_exactly_where_a_case_says_so(curve, n):
    R = rc.reference(curve, n)
    seen = set()
    for c in R.t.cases:
        r = R.result(c)
        got = {name for name, hit in (("c_q", r.c_q is None), ("l_zw", r.l_zw == 0), ("phi_z", r.phi_z is None), ("phi_zw", r.phi_zw is None)) if hit}
        assert got == set(c.degenerate), (c.name, got)
        assert (r.c_q is None) == (not any(r.q)) and (r.phi_zw is None) == (not any(r.lin)) and (r.phi_z is None) == (not any(r.w1))
        seen |= got
    assert seen == ({"c_q", "l_zw", "phi_z", "phi_zw"} if n == 512 else {"l_zw", "phi_zw"})
    if n == 512:
        for c in R.t.batch_degenerate_17():
            assert {"c_q", "phi_z", "phi_zw"} <= c.degenerate
        only = R.t.batch_of_1(True)[0]
        assert only.degenerate == {"c_q", "l_zw", "phi_z", "phi_zw"} and only.nus == rc.one_hot(8, 7) and not any(only.alphas)
