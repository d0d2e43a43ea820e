"""The chosen-challenge cases of the ring prover's phases, shared by test_ring_phase_ref_cpu.py, which proves the big-integer reference
(ring_phase_ref.py) at each of them, and test_gpu_ring_phases.py, which runs the device phases at them.

A case is (witness, alphas, zeta, nus).  One challenge is structured per case and the others are random, so that a degenerate alpha does
not hide what a zeta does; the cases of kind "product" are the exceptions.  Every challenge vector meets witnesses of three kinds:
no hidden rows (the device's zk_rows = NULL path), random hidden rows, and hidden rows from {0, 1, p-1, (p-1)/2, (p+1)/2}.

Everything here is a fixed list: `Tables(curve, n)` builds the same cases on every run (seeded), and EXPECTED_COUNTS pins their number."""
import os
import random
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import ring_phase_ref as ref  # noqa: E402
from oracle import coracle  # noqa: E402
from oracle.pyref import bandersnatch as bsn  # noqa: E402
from oracle.pyref import kzg  # noqa: E402
from oracle.pyref import ring as oring  # noqa: E402

P = bsn.P
H = (P - 1) // 2
SUITES = {"bandersnatch": bsn.SHA512, "jubjub": bsn.JUBJUB}
CURVES = tuple(SUITES)
TAU = int.from_bytes(b"ring-phase-tau".ljust(31, b"\x07"), "little") % P
RING_KEYS = {512: 8, 1024: 300}
LIMB_EDGES = tuple(v for k in (29, 58, 232, 252) for v in ((1 << k) - 1, 1 << k))   # limb boundaries of the 29- and 32-bit forms


def _rng(*key):
    return random.Random("ring-phases/" + "/".join(str(k) for k in key))


def keys_of(curve, count):
    """ring keys (multiples of the generator under the curve's constants); key 1 does not decode"""
    with bsn.using(SUITES[curve]):
        rng = _rng(curve, "keys", count)
        keys = [bsn.enc_point(bsn.mul(bsn.G, rng.randrange(1, bsn.N))) for _ in range(count)]
    keys[1] = bytes(32)
    return keys


class Witness:
    def __init__(self, name, kind, producer, blinding, zk_rows):
        self.name, self.kind, self.producer, self.blinding, self.zk_rows = name, kind, producer, blinding, zk_rows

    def zk_bytes(self):
        return b"".join(ref.le32(v) for c in ref.COLUMNS for v in self.zk_rows[c])


class Case:
    def __init__(self, name, kind, witness, alphas, zeta, nus, degenerate=()):
        self.name, self.kind, self.witness, self.alphas, self.zeta, self.nus = name, kind, witness, tuple(alphas), zeta, tuple(nus)
        # which of c_q, l_zw, phi_z, phi_zw the case is built to make the point at infinity / zero
        self.degenerate = frozenset(degenerate)
        assert len(self.alphas) == 7 and len(self.nus) == 8 and all(0 <= v < P for v in self.alphas + self.nus + (zeta,))


def one_hot(n, i, v=1):
    return tuple(v if j == i else 0 for j in range(n))


class Tables:
    def __init__(self, curve, n=512):
        self.curve, self.n, self.suite = curve, n, SUITES[curve]
        with bsn.using(self.suite):
            order = bsn.N
        self.order = order
        pr = oring.Params(domain_size=n, suite=self.suite)            # for the domain only
        self.omega, self.omega_4n, self.last_index = pr.omega, pr.radix_omega, pr.last_index
        dom = pr.domain
        last_row = RING_KEYS[n] - 1
        rng = _rng(curve, n)
        rnd = lambda: rng.randrange(P)
        top = 1 << (order.bit_length() - 1)
        alt = 0x5555555555555555555555555555555555555555555555555555555555555555 % order
        edge_vals = (0, 1, P - 1, H, H + 1)
        rows = lambda f: {c: [f() for _ in range(3)] for c in ref.COLUMNS}
        self.witnesses = {w.name: w for w in (
            Witness("none", "none", 0, 1, None),
            Witness("random", "random", last_row, order - 1, rows(rnd)),
            Witness("edge", "edge", 0, top, rows(lambda: rng.choice(edge_vals))),
            Witness("all-zero", "edge", last_row, alt, rows(lambda: 0)),
            Witness("all-max", "edge", last_row, alt, rows(lambda: P - 1)),
            Witness("max-zero-max", "edge", 0, order - 1, {c: [P - 1, 0, P - 1] for c in ref.COLUMNS}),
        )}
        assert {v for w in ("edge",) for c in ref.COLUMNS for v in self.witnesses[w].zk_rows[c]} <= set(edge_vals)
        r = rnd()
        self.alphas = [("zero", (0,) * 7)] + [(f"e{i}", one_hot(7, i)) for i in range(7)] + [("max", (P - 1,) * 7), ("000rrrr", (0, 0, 0, r, r, r, r))]
        self.alphas += [(f"limb-{v.bit_length()}-{v & 1}", (v,) * 7) for v in LIMB_EDGES]
        self.alphas.append(("random", tuple(rnd() for _ in range(7))))
        w_inv = pow(self.omega, -1, P)
        self.zetas = [("0", 0), ("1", 1), ("max", P - 1), ("w", self.omega), ("w^-1", w_inv), ("last", dom[self.last_index]),
                      ("hidden-0", dom[n - 3]), ("hidden-1", dom[n - 2]), ("hidden-2", dom[n - 1]), ("w4n", self.omega_4n), ("tau", TAU),
                      ("2^252", 1 << 252), ("half", H), ("random", rnd())]
        assert dom[n - 1] == w_inv and dom[n - 3] * self.omega % P == dom[n - 2]
        self.nus = [("zero", (0,) * 8)] + [(f"e{i}", one_hot(8, i)) for i in range(8)] + [("max", (P - 1,) * 8), ("random", tuple(rnd() for _ in range(8)))]
        def zdeg(zn, w):
            """what a zeta makes zero by itself.  `last`: term = 0, so lin = 0.  hidden-0 / hidden-1: zeta w is the next hidden row, where lin is
            a combination of the three accumulator columns' values: l(zeta w) = 0 when those rows are zero.  w^-1: zeta is the last hidden
            row, where px = py = 0, so with b = 1 there fx = fy = 0 and l(zeta w) = lin(1) = alpha_0 term accip(1) = 0, accip starting at 0."""
            row = lambda col, i: w.zk_rows[col][i] if w.zk_rows else 0
            if zn == "last":
                return ("l_zw", "phi_zw")
            if zn in ("hidden-0", "hidden-1") and not any(row(c, int(zn[-1]) + 1) for c in ("accip", "accx", "accy")):
                return ("l_zw",)
            if zn in ("w^-1", "hidden-2") and row("b", 2) == 1:         # (the same point under two names)
                return ("l_zw",)
            return ()

        if n != 512:
            # the larger domain repeats the zeta edges alone (k_ring_eval's coefficients per lane and idle lanes depend on N)
            self.cases = [Case(f"zeta-{zn}/{wn}", "zeta", self.witnesses[wn], tuple(rnd() for _ in range(7)), z, tuple(rnd() for _ in range(8)),
                               zdeg(zn, self.witnesses[wn]))
                          for zn, z in self.zetas for wn in ("none", "max-zero-max")]
            self.by_name = {c.name: c for c in self.cases}
            return
        trio = lambda i: ("none", "random", ("edge", "all-zero", "all-max", "max-zero-max")[i % 4])
        cases = []
        for i, (an, a) in enumerate(self.alphas):
            deg = ("c_q", "l_zw", "phi_zw") if an == "zero" else ("l_zw", "phi_zw") if an in ("000rrrr", "e3", "e4", "e5", "e6") else ()
            for wn in trio(i):
                cases.append(Case(f"alpha-{an}/{wn}", "alpha", self.witnesses[wn], a, rnd(), tuple(rnd() for _ in range(8)), deg))
        for i, (zn, z) in enumerate(self.zetas):
            for wn in trio(i):
                cases.append(Case(f"zeta-{zn}/{wn}", "zeta", self.witnesses[wn], tuple(rnd() for _ in range(7)), z, tuple(rnd() for _ in range(8)),
                                  zdeg(zn, self.witnesses[wn])))
        for i, (nn, v) in enumerate(self.nus):
            for wn in trio(i):
                cases.append(Case(f"nu-{nn}/{wn}", "nu", self.witnesses[wn], tuple(rnd() for _ in range(7)), rnd(), v, ("phi_z",) if nn == "zero" else ()))
        zero7, zero8 = (0,) * 7, (0,) * 8
        for wn in ("none", "random", "max-zero-max"):
            w = self.witnesses[wn]
            cases += [
                # q = 0, lin = 0 and the aggregate is nu_7 q = 0: all three MSMs of the case are empty
                Case(f"zero-alphas-nu-e7/{wn}", "product", w, zero7, rnd(), one_hot(8, 7), ("c_q", "l_zw", "phi_z", "phi_zw")),
                Case(f"zero-alphas-zero-nus/{wn}", "product", w, zero7, rnd(), zero8, ("c_q", "l_zw", "phi_z", "phi_zw")),
                Case(f"zeta-last-zero-nus/{wn}", "product", w, tuple(rnd() for _ in range(7)), dom[self.last_index], zero8, ("l_zw", "phi_z", "phi_zw")),
            ]
        # p - 1 everywhere: alphas, nus and the hidden rows together
        cases.append(Case("max-everywhere/all-max", "product", self.witnesses["all-max"], (P - 1,) * 7, rnd(), (P - 1,) * 8))
        cases.append(Case("max-everywhere-zeta-max/all-max", "product", self.witnesses["all-max"], (P - 1,) * 7, P - 1, (P - 1,) * 8))
        self.cases = cases
        self.by_name = {c.name: c for c in cases}
        assert len(self.by_name) == len(cases)

    # ------------------------------------------------------------ batches of the GPU module (names of cases; one zk mode per batch)
    def pinned(self):
        return [c for c in self.cases if c.witness.zk_rows is not None]

    def unpinned(self):
        return [c for c in self.cases if c.witness.zk_rows is None]

    def batch_degenerate_17(self):
        """17 proofs, every one degenerate: the batched MSMs see zero scalars only, across many sets"""
        pool = [c for c in self.pinned() if c.kind == "product" and {"c_q", "phi_z", "phi_zw"} <= c.degenerate]
        return [pool[i % len(pool)] for i in range(17)]

    def batch_mixed_65(self):
        """every kind of case once (each alpha, zeta and nu vector and each product), then random cases up to 65 proofs"""
        groups = {}
        for c in self.pinned():
            groups.setdefault(c.name.split("/")[0], []).append(c)
        out = [g[i % len(g)] for i, g in enumerate(groups.values())]
        rnd = [c for c in self.pinned() if c.name.split("/")[0] in ("alpha-random", "zeta-random", "nu-random")]
        assert len(out) <= 65
        i = 0
        while len(out) < 65:
            out.append(rnd[i % len(rnd)])
            i += 1
        return out

    def batch_of_3(self):
        return [self.by_name["zero-alphas-nu-e7/random"], self.by_name["alpha-random/random"], self.by_name["zeta-last-zero-nus/max-zero-max"]]

    def batch_of_1(self, pinned):
        return [self.by_name["zero-alphas-nu-e7/random" if pinned else "zero-alphas-nu-e7/none"]]


# cases per table: 512 -> 3 witnesses x (19 alpha + 14 zeta + 11 nu vectors) + 3 x 3 products + 2; 1024 -> 14 zetas x 2 witnesses
EXPECTED_COUNTS = {512: 3 * (19 + 14 + 11) + 9 + 2, 1024: 28}

_tables = {}


def tables(curve, n=512):
    if (curve, n) not in _tables:
        _tables[(curve, n)] = Tables(curve, n)
    return _tables[(curve, n)]


# ---------------------------------------------------------------- the reference side: ring, known-tau SRS, one State per witness
_srs = {}
_refs = {}


def known_tau_srs(n):
    if n not in _srs:
        _srs[n] = kzg.SRS.from_tau(TAU, 3 * n + 1)
        _srs[n].g2_raw = list(kzg.default_srs().g2_raw)      # transcript bytes only (vk_bytes); no pairing is taken here
    return _srs[n]


class Reference:
    """oracle ring and root over the known-tau SRS, the States of the table's witnesses, and each case's results (computed once)"""

    def __init__(self, curve, n, commit=None):
        self.t = tables(curve, n)
        self.commit = commit
        self.suite = SUITES[curve]
        self.keys = keys_of(curve, RING_KEYS[n])
        srs = known_tau_srs(n)
        with bsn.using(self.suite):
            self.params = oring.Params(domain_size=n, suite=self.suite, srs=srs)
            self.params_tv = oring.Params(domain_size=n, suite=self.suite, srs=srs, test_vectors=True)
            self.ring, self.ring_tv = oring.Ring(self.keys, self.params), oring.Ring(self.keys, self.params_tv)
            self.root, self.root_tv = oring.RingRoot(self.ring), oring.RingRoot(self.ring_tv)
        self._states, self._results = {}, {}

    def state(self, wname):
        if wname not in self._states:
            w = self.t.witnesses[wname]
            with bsn.using(self.suite):
                self._states[wname] = ref.witness(self.ring, self.root, w.producer, w.blinding, w.zk_rows, self.commit)
        return self._states[wname]

    def result(self, case):
        """a snapshot of what the four phases make at this case"""
        if case.name not in self._results:
            st = self.state(case.witness.name)
            with bsn.using(self.suite):
                ref.prove_with(st, case.alphas, case.zeta, case.nus)
            snap = ref.State()
            for k in ("relation", "cols", "commitments", "q", "c_q", "evals", "lin", "l_zw", "agg", "w1", "w2", "phi_z", "phi_zw"):
                setattr(snap, k, getattr(st, k))
            snap.payload = ref.payload(st)
            self._results[case.name] = snap
        return self._results[case.name]


def reference(curve, n=512, by_tau=False):
    """by_tau: commitments as f(tau) G (one scalar multiplication each) instead of the MSM over the SRS; test_ring_phase_ref_cpu.py proves
    the two equal at every case"""
    if (curve, n, by_tau) not in _refs:
        _refs[(curve, n, by_tau)] = Reference(curve, n, tau_commitment if by_tau else None)
    return _refs[(curve, n, by_tau)]


def at_tau(poly):
    return oring.horner(poly, TAU)


def tau_commitment(poly):
    """f(tau) G by one scalar multiplication of the C oracle, None for infinity"""
    v = at_tau(poly)
    return coracle.g1_mul(kzg.G1_GEN, v) if v else None
