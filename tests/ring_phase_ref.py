"""The ring prover of oracle/pyref/ring.py (prove_ring) restated phase by phase, as the device API cuts it (dr_ring_prove_witness,
_quotient, _evals, _openings): the challenges are ARGUMENTS and the intermediate polynomials are RETURN VALUES, all Python integers.
prove_ring draws its challenges from the Fiat-Shamir transcript, so they are always 255-bit random values; here a caller can put 0, 1,
p - 1 or a point of the domain where a kernel branches or degenerates, and see which polynomial differs, not only which commitment.

Built from the oracle's own helpers (intt, eval_on_domain, horner, kzg.synthetic_div, kzg.commit); nothing of dot_ring_amd is imported.
test_ring_phase_ref_cpu.py proves it against prove_ring (byte for byte, with the transcript's and with overridden challenges) and,
through a known-tau SRS, against f(tau) G.

A State is one witness.  The phases record what they were given and what they made in it, in the order the device runs them:
    st = witness(ring, root, producer, blinding, zk_rows)     st.relation, st.cols, st.commitments
    q, c_q = quotient(st, alphas)                             also st.alphas, st.q, st.c_q
    values, lin, l_zw = evals(st, zeta)                       also st.zeta, st.evals, st.lin, st.l_zw
    agg, w1, w2, phi_z, phi_zw = openings(st, nus)            also st.nus, ...
The quotient is linear in the alphas: the seven per-constraint quotients are computed once per State (constraint_quotients), and any
alpha vector is a linear combination of them; quotient_direct aggregates first and divides afterwards, as prove_ring does."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle.pyref import bandersnatch as bsn  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref import ring as oring  # noqa: E402

P = bsn.P
COLUMNS = ("b", "accip", "accx", "accy")            # the order of the device's commitments, hidden rows and coefficient columns


class State:
    pass


def le32(v):
    return int(v).to_bytes(32, "little")


def witness(ring, root, producer, blinding, zk_rows=None, commit=None):
    """producer: row of the signer's key; zk_rows: {column: [3 ints]} for rows N-3..N-1, None for zeros (test-vector mode).  Must run
    under bsn.using(suite) of the ring's suite, like every call of the oracle.  commit: kzg.commit over the ring's SRS unless given
    (with a known-tau SRS, f -> f(tau) G is the same point for one scalar multiplication: ring_phase_cases.tau_commitment)."""
    pr = ring.params
    n, suite, k = pr.N, pr.suite, producer
    bits = [1 if i == k else 0 for i in range(pr.max_ring)]
    bits += [int(c) for c in bin(blinding)[2:][::-1]]
    assert len(bits) <= n - oring.PADDING_ROWS
    bits += [0] * (n - oring.PADDING_ROWS - len(bits)) + [0]
    acc = [suite.accumulator_base]
    for i in range(1, n - oring.PADDING_ROWS + 1):
        acc.append(bsn._te_add_ref(acc[-1], ring.points[i - 1]) if bits[i - 1] else acc[-1])
    accip = [0]
    for i in range(1, n - oring.PADDING_ROWS + 1):
        accip.append(accip[-1] + bits[i - 1] * root.s_evals[i - 1])
    rows = {"b": bits, "accip": accip, "accx": [pt[0] for pt in acc], "accy": [pt[1] for pt in acc]}
    st = State()
    st.ring, st.root, st.params, st.producer, st.blinding, st.zk_rows = ring, root, pr, producer, blinding, zk_rows
    st.commit = commit or (lambda coeffs: kzg.commit(coeffs, pr.srs))
    st.cols, st.commitments = [], []
    for name in COLUMNS:
        ev = list(rows[name])
        ev += [0] * (n - oring.ZK_ROWS - len(ev))
        ev += [v % P for v in zk_rows[name]] if zk_rows else [0] * oring.ZK_ROWS
        assert len(ev) == n
        coeffs = oring.intt(ev, pr.omega)
        st.cols.append(coeffs)
        st.commitments.append(st.commit(coeffs))
    st.relation = bsn._te_add_ref(ring.points[k], bsn.mul(suite.blinding_base, blinding))
    st.result = bsn._te_add_ref(st.relation, suite.accumulator_base)
    st._cq = None
    return st


def constraint_evals(st):
    """c1..c7 on the 4N domain, one list per constraint (constraints.py:43-151 as prove_ring restates them)"""
    pr, root = st.params, st.root
    n, m, w4 = pr.N, pr.radix, pr.radix_omega
    b_c, accip_c, accx_c, accy_c = st.cols
    px4, py4, s4 = (oring.eval_on_domain(c, m, w4) for c in (root.px, root.py, root.s))
    b4, ax4, ay4, ip4 = (oring.eval_on_domain(c, m, w4) for c in (b_c, accx_c, accy_c, accip_c))
    inv_n = pow(n, -1, P)

    def lagrange(i):
        inv_xi = pow(pr.domain[i], -1, P)
        out, cur = [], inv_n
        for _ in range(n):
            out.append(cur)
            cur = cur * inv_xi % P
        return out

    l0 = oring.eval_on_domain(lagrange(0), m, w4)
    ln = oring.eval_on_domain(lagrange(pr.last_index), m, w4)
    last_root = pr.domain[pr.last_index]
    (sx, sy), (rx, ry) = pr.suite.accumulator_base, st.result
    shift = m // n
    a = bsn.A
    cs = [[] for _ in range(7)]
    x = 1
    for i in range(m):
        j = (i + shift) % m
        nl = (x - last_root) % P
        x1, y1, x2, y2, x3, y3, b = ax4[i], ay4[i], px4[i], py4[i], ax4[j], ay4[j], b4[i]
        cs[0].append((ip4[j] - ip4[i] - b * s4[i]) * nl % P)
        cs[1].append((b * (x3 * (y1 * y2 + a * x1 * x2) - (x1 * y1 + x2 * y2)) + (1 - b) * (x3 - x1)) * nl % P)
        cs[2].append((b * (y3 * (x1 * y2 - x2 * y1) - (x1 * y1 - x2 * y2)) + (1 - b) * (y3 - y1)) * nl % P)
        cs[3].append(b * (1 - b) % P)
        cs[4].append(((x1 - sx) * l0[i] + (x1 - rx) * ln[i]) % P)
        cs[5].append(((y1 - sy) * l0[i] + (y1 - ry) * ln[i]) % P)
        cs[6].append((ip4[i] * l0[i] + (ip4[i] - 1) * ln[i]) % P)
        x = x * w4 % P
    return cs


def _tail(pr):
    tail = [1]
    for off in range(1, 4):
        tail = oring._poly_mul_small(tail, [(-pr.domain[-off]) % P, 1])
    return tail


def divide_out(pr, evals4):
    """evaluations on the 4N domain -> coefficients, times (X - w^-1)(X - w^-2)(X - w^-3), over X^N - 1 (proof_builder.py:165-195,
    ops.py:207): exactly 3N + 1 coefficients, zero-padded"""
    n = pr.N
    c = oring._poly_mul_small(_tail(pr), oring.intt(evals4, pr.radix_omega))
    while c and c[-1] == 0:
        c.pop()
    q = [0] if len(c) < n else [sum(c[j + i * n] for i in range(1, len(c) // n + 1) if j + i * n < len(c)) % P for j in range(len(c) - n)]
    assert len(q) <= 3 * n + 1 or not any(q[3 * n + 1 :])
    q = q[: 3 * n + 1]
    return q + [0] * (3 * n + 1 - len(q))


def constraint_quotients(st):
    if st._cq is None:
        st._cq = [divide_out(st.params, c) for c in constraint_evals(st)]
    return st._cq


def quotient(st, alphas):
    qs = constraint_quotients(st)
    alphas = [a % P for a in alphas]
    assert len(alphas) == 7
    q = [sum(a * qi[j] for a, qi in zip(alphas, qs)) % P for j in range(3 * st.params.N + 1)]
    st.alphas, st.q, st.c_q = alphas, q, st.commit(q)
    return q, st.c_q


def quotient_direct(st, alphas):
    """prove_ring's order: aggregate the constraints point by point, then interpolate and divide"""
    cs = constraint_evals(st)
    agg = [sum(a * c[i] for a, c in zip(alphas, cs)) % P for i in range(st.params.radix)]
    return divide_out(st.params, agg)


def evals(st, zeta):
    """the seven register values (px, py, s, b, accip, accx, accy at zeta), lin (N coefficients) and l(zeta w); the alphas are those of
    the quotient phase"""
    pr, root = st.params, st.root
    zeta %= P
    b_c, accip_c, accx_c, accy_c = st.cols
    values = [oring.horner(c, zeta) for c in (root.px, root.py, root.s, b_c, accip_c, accx_c, accy_c)]
    pxz, pyz, _sz, bz, _ipz, axz, ayz = values
    term = (zeta - pr.domain[pr.last_index]) % P
    fx = (bz * (ayz * pyz + bsn.A * axz * pxz) + (1 - bz)) * term % P
    fy = (bz * (axz * pyz - pxz * ayz) + (1 - bz)) * term % P
    al = st.alphas
    lin = [(al[0] * term % P * ci + al[1] * fx % P * cx + al[2] * fy % P * cy) % P for ci, cx, cy in zip(accip_c, accx_c, accy_c)]
    st.zeta, st.evals, st.lin, st.l_zw = zeta, values, lin, oring.horner(lin, zeta * pr.omega % P)
    return values, lin, st.l_zw


def openings(st, nus):
    """the nu-aggregate of px, py, s, b, accip, accx, accy, q (3N + 1 coefficients), its quotient by (X - zeta), lin's quotient by
    (X - zeta w), and their commitments"""
    pr, root = st.params, st.root
    nus = [v % P for v in nus]
    assert len(nus) == 8
    b_c, accip_c, accx_c, accy_c = st.cols
    polys = [root.px, root.py, root.s, b_c, accip_c, accx_c, accy_c, st.q]
    width = 3 * pr.N + 1
    agg = [sum(nu * (p[i] if i < len(p) else 0) for nu, p in zip(nus, polys)) % P for i in range(width)]
    w1, _ = kzg.synthetic_div(agg, st.zeta)
    w2, _ = kzg.synthetic_div(st.lin, st.zeta * pr.omega % P)
    st.nus, st.agg, st.w1, st.w2 = nus, agg, w1, w2
    st.phi_z, st.phi_zw = st.commit(w1), st.commit(w2)
    return agg, w1, w2, st.phi_z, st.phi_zw


def payload(st):
    """the 592 bytes of proof_payload.py:68 from a State that has been through all four phases"""
    b, accip, accx, accy = st.commitments
    return (b"".join(kzg.compress(c) for c in (b, accip, accx, accy)) + b"".join(le32(e) for e in st.evals)
            + kzg.compress(st.c_q) + le32(st.l_zw) + kzg.compress(st.phi_z) + kzg.compress(st.phi_zw))


def prove_with_transcript(st):
    """all four phases with the challenges of the Fiat-Shamir transcript, as prove_ring draws them"""
    pr = st.params
    prefix = oring.FsTranscript(pr.suite.suite_id)
    prefix.absorb(b"vk", st.root.vk_bytes())
    t = prefix.fork()
    t.absorb(b"instance", le32(st.relation[0]) + le32(st.relation[1]))
    t.absorb(b"committed_cols", b"".join(kzg.serialize(c) for c in st.commitments))
    _, c_q = quotient(st, t.challenges(b"constraints_aggregation", 7))
    t.absorb(b"quotient", kzg.serialize(c_q))
    (zeta,) = t.challenges(b"evaluation_point", 1)
    values, _, l_zw = evals(st, zeta)
    t.absorb(b"register_evaluations", b"".join(le32(e) for e in values))
    t.absorb(b"shifted_linearization_evaluation", le32(l_zw))
    openings(st, t.challenges(b"kzg_aggregation", 8))
    return payload(st)


def prove_with(st, alphas, zeta, nus):
    quotient(st, alphas)
    evals(st, zeta)
    openings(st, nus)
    return payload(st)
