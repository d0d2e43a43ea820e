"""Ring, RingRoot and RingVRF (dot_ring/vrf/ring/{members,root,vrf}.py, ring_proof/proof_payload.py)."""
from __future__ import annotations

import ctypes

import hashlib
import os
import secrets
import threading
from dataclasses import dataclass
from functools import lru_cache

from .. import _native, runtime
from ..curve import valid_points
from ..ring_proof.columns import Column
from ..ring_proof.params import RingProofParams
from ..ring_proof.pcs import KZG
from ..ring_proof.poly import inverse_fft_batch
from ..ring_proof import device_prover
from ..ring_proof.prover import build_ring_proofs
from ..ring_proof.transcript import FiatShamirTranscript, serialize_verifier_key
from ..ring_proof.verifier import batch_inverse, linear_pcs_verifications, replay_challenges, zeta_denominators
from .base import VRF
from .codec import point_len

_PK_MEMO_LOCK = threading.Lock()          # guards every RingVRF class's _pk_memo (prove_batch)
from .pedersen import PedersenVRF

RING_SCALAR_LEN = 32


def verify_tree_descent(count: int, holds) -> tuple:
    """Which of `count` items fail, from tests of spans: holds(lo, hi) says whether items [lo, hi) hold together.  The descent of
    csrc/verify_tree.hpp over the same tree (leaves padded to a power of two): the whole span is tested once; a span is tested only
    if its parent failed; a span whose sibling held under a failed parent fails without a test; padding is never tested.
    Returns (list of bool, number of tests): 1 test when nothing fails, at most 1 + 2 k ceil(log2 count) for k failing items."""
    if count == 0:
        return [], 0
    tests = 1
    if holds(0, count):
        return [True] * count, tests
    width = 1 << max(count - 1, 0).bit_length()
    failed = [0]                                   # first leaves of the failed spans of the current width
    while width > 1:
        half = width // 2
        nxt = []
        for lo in failed:
            mid = lo + half
            if mid >= count:                       # the right half is padding: the left half inherits the failure
                nxt.append(lo)
                continue
            tests += 1
            if holds(lo, mid):
                nxt.append(mid)
                continue
            nxt.append(lo)
            tests += 1
            if not holds(mid, min(count, mid + half)):
                nxt.append(mid)
        failed, width = nxt, half
    verdicts = [True] * count
    for lo in failed:
        verdicts[lo] = False
    return verdicts, tests



# ------------------------------------------------------------------ Ring (members.py:18-101)
class Ring:
    def __init__(self, keys, params: RingProofParams | None = None):
        if params is None:
            params = RingProofParams.from_ring_size(len(keys))
        self.params = params
        aux = params.cv.curve.params.auxiliary_points
        if not aux.padding_point:
            raise ValueError("padding point is not configured in curve parameters")
        if len(keys) > params.max_ring_size:
            raise ValueError(f"ring size {len(keys)} exceeds max supported size {params.max_ring_size}")
        points = [pt if pt is not None else aux.padding_point for pt in self._decode_keys(keys)]
        points += [aux.padding_point] * (params.max_ring_size - len(points))
        fill = params.domain_size - params.padding_rows - len(points)
        if fill > 0:
            if not aux.blinding_base:
                raise ValueError("blinding base is not configured in curve parameters")
            points += list(_blinding_base_powers(params.cv.point_type, aux.blinding_base, fill))
        points += [(0, 0)] * params.padding_rows
        self.nm_points = tuple(points)

    def _decode_keys(self, keys):
        """Decode + subgroup-check all keys in one kernel launch; invalid / identity keys -> None."""
        cv = self.params.cv
        slots = [i for i, key in enumerate(keys) if len(key) == point_len(cv)]
        out = [None] * len(keys)
        if not slots:
            return out
        raw, ok = runtime.context().bsn_decode_points(b"".join(bytes(keys[i]) for i in slots), cv.curve.params.curve_id)
        frm = int.from_bytes
        for j, slot in enumerate(slots):
            if ok[j]:
                out[slot] = (frm(raw[64 * j : 64 * j + 32], "little"), frm(raw[64 * j + 32 : 64 * j + 64], "little"))
        return out

    @classmethod
    def from_keys(cls, keys, params: RingProofParams | None = None) -> "Ring":
        return _ring(tuple(bytes(k) for k in keys))

    def indices_of(self, keys) -> list:
        """index_of for several keys with two kernel launches in total."""
        padding = self.params.cv.curve.params.auxiliary_points.padding_point
        lookup = getattr(self, "_row_of", None)
        if lookup is None:
            lookup = {}
            for row, pt in enumerate(self.nm_points[: self.params.max_ring_size]):
                lookup.setdefault(pt, row)
            self._row_of = lookup
        out = []
        memo = self.__dict__.setdefault("_decoded_producers", {})       # key bytes -> decoded point (or None): decode once
        distinct = [k for k in dict.fromkeys(bytes(k) for k in keys) if k not in memo]   # a batch usually repeats few producer keys
        if distinct:
            if len(memo) + len(distinct) > 65536:
                memo.clear()
            memo.update(zip(distinct, self._decode_keys(distinct)))
        for point in (memo[bytes(k)] for k in keys):
            if point is None:
                raise ValueError("invalid ring key")
            if point == padding or point not in lookup:
                raise ValueError("producer key is not in ring")
            out.append(lookup[point])
        return out

    def index_of(self, key: bytes) -> int:
        return self.indices_of([key])[0]


@lru_cache(maxsize=8)
def _blinding_base_powers(point_type, blinding_base, count):
    out, point = [], point_type(*blinding_base)
    for _ in range(count):
        out.append((point.x, point.y))
        point = point + point
    return tuple(out)


@lru_cache(maxsize=2)
def _params(keys_len: int) -> RingProofParams:
    return RingProofParams.from_ring_size(keys_len)


@lru_cache(maxsize=8)
def _ring(keys: tuple) -> Ring:
    return Ring(keys, _params(len(keys)))


# ------------------------------------------------------------------ RingRoot (root.py:14-173)
@dataclass
class RingRoot:
    px: Column
    py: Column
    s: Column
    params: RingProofParams | None = None

    @classmethod
    def from_ring(cls, ring: Ring, params: RingProofParams | None = None) -> "RingRoot":
        if params is None:
            params = ring.params
        n = params.domain_size
        s_evals, s_coeffs, s_cm = _selector_column_data(n, params.max_ring_size, params.omega, params.prime, params.pcs)
        px_e, px_c, px_cm, py_e, py_c, py_cm = _public_keys_column_data(ring.nm_points, n, params.omega, params.prime, params.pcs)
        return cls(px=Column("px", list(px_e), coeffs=list(px_c), _commitment=px_cm, size=n, _has_commitment=True),
                   py=Column("py", list(py_e), coeffs=list(py_c), _commitment=py_cm, size=n, _has_commitment=True),
                   s=Column("s", list(s_evals), coeffs=list(s_coeffs), _commitment=s_cm, size=n, _has_commitment=True),
                   params=params)

    def fixed_commitments(self) -> list:
        return [self.px.commitment, self.py.commitment, self.s.commitment]

    def _verifier_key(self) -> bytes:
        if self.params is None:
            raise ValueError("Ring root verifier transcript requires ring proof parameters")
        pcs = self.params.pcs
        srs = pcs._srs() if hasattr(pcs, "_srs") else pcs.srs
        return serialize_verifier_key(srs.g1_raw[:96], srs.g2_raw, [pcs.serialize_g1_uncompressed(c) for c in self.fixed_commitments()])

    def verifier_transcript_prefix(self, transcript_challenge: bytes | None = None) -> FiatShamirTranscript:
        vk = self._verifier_key()
        if transcript_challenge is None:
            transcript_challenge = self.params.cv.curve.params.suite_id
        t = FiatShamirTranscript(self.params.prime, transcript_challenge)
        t.absorb_labeled(b"vk", vk)
        return t

    def verifier_transcript_prefix_bytes(self, transcript_challenge: bytes | None = None) -> bytes:
        """The byte stream verifier_transcript_prefix() has absorbed (input of the native batch prover)."""
        vk = self._verifier_key()
        label = transcript_challenge if transcript_challenge is not None else self.params.cv.curve.params.suite_id
        be = lambda v: len(v).to_bytes(4, "big")
        return label + be(label) + b"vk" + be(b"vk") + vk + be(vk)

    @staticmethod
    def encoded_len(params: RingProofParams | None = None) -> int:
        return 3 * (params.pcs.commitment_size if params is not None else KZG.commitment_size)

    def encode(self) -> bytes:
        pcs = self.params.pcs if self.params is not None else KZG
        return b"".join(pcs.compress_g1(c) for c in self.fixed_commitments())

    @classmethod
    def decode(cls, data: bytes, ring=None) -> "RingRoot":
        params = ring.params if isinstance(ring, Ring) else ring
        if params is None:
            params = RingProofParams()
        size = params.pcs.commitment_size
        if len(data) != cls.encoded_len(params):
            raise ValueError(f"invalid ring root length: ring root must be exactly {cls.encoded_len(params)} bytes, got {len(data)}")
        cms = [params.pcs.decompress_g1(data[size * i : size * (i + 1)]) for i in range(3)]
        n = params.domain_size
        cols = [Column(name, [], _commitment=cm, size=n, _has_commitment=True) for name, cm in zip(("px", "py", "s"), cms)]
        return cls(px=cols[0], py=cols[1], s=cols[2], params=params)

    def matches_ring(self, ring: Ring) -> bool:
        return RingRoot.from_ring(ring).encode() == self.encode()


@lru_cache(maxsize=2)
def _selector_column_data(domain_size, max_ring_size, omega, prime, pcs):
    evals = [1 if i < max_ring_size else 0 for i in range(domain_size)]
    coeffs = inverse_fft_batch([evals], omega, prime)[0]
    return tuple(evals), tuple(coeffs), pcs.commit(coeffs)


@lru_cache(maxsize=8)
def _public_keys_column_data(nm_points, domain_size, omega, prime, pcs):
    px_e, py_e = [pt[0] for pt in nm_points], [pt[1] for pt in nm_points]
    px_c, py_c = inverse_fft_batch([px_e, py_e], omega, prime)
    if hasattr(pcs, "commit_batch"):
        px_cm, py_cm = pcs.commit_batch([px_c, py_c])
    else:
        px_cm, py_cm = pcs.commit(px_c), pcs.commit(py_c)
    return tuple(px_e), tuple(px_c), px_cm, tuple(py_e), tuple(py_c), py_cm


# ------------------------------------------------------------------ RingVRF (vrf.py:30-305, proof_payload.py)
@dataclass
class RingVRF(VRF):
    RING = True                   # (VRF.__class_getitem__: the suites whose points the ring proof's 32-byte columns cannot hold are refused)

    pedersen_proof: PedersenVRF
    c_b: Column
    c_accip: Column
    c_accx: Column
    c_accy: Column
    px_zeta: int
    py_zeta: int
    s_zeta: int
    b_zeta: int
    accip_zeta: int
    accx_zeta: int
    accy_zeta: int
    c_q: Column
    l_zeta_omega: int
    open_agg_zeta: object
    open_l_zeta_omega: object

    _FIELDS = ("pedersen_proof", "c_b", "c_accip", "c_accx", "c_accy", "px_zeta", "py_zeta", "s_zeta", "b_zeta", "accip_zeta",
               "accx_zeta", "accy_zeta", "c_q", "l_zeta_omega", "open_agg_zeta", "open_l_zeta_omega")

    @classmethod
    def _from_batch(cls, raw_blob: bytes, aux_blob: bytes, count: int, blind_blob=None) -> list:
        """The proofs of one dr_ringvrf_prove_batch call: every object only points into the two shared byte strings; its own 784 +
        960 bytes are sliced out when something first asks for them (1024 objects: 0.35 ms instead of 1.2 ms), and batch_verify
        of exactly these proofs, untouched and in order, hands the shared string to the library without re-assembling it.
        The shared auxiliary string holds NO secret: the blinding factors were moved out of it (dr_ringvrf_aux_take_blindings) and
        each proof keeps its own 32 bytes only — holding or pickling one proof does not keep another proof's blinding factor alive."""
        new = object.__new__
        out = []
        for i in range(count):
            p = new(cls)
            p.__dict__["_batch"] = (raw_blob, aux_blob, i, None if blind_blob is None else blind_blob[32 * i : 32 * i + 32])
            out.append(p)
        return out

    @classmethod
    def _from_encoded(cls, blob: bytes, count: int) -> list:
        """`count` proofs that arrived ENCODED in one byte string (the gather of a sharded prove_batch, a block of proofs off the
        wire): every object only points into the shared string.  encode() and batch_verify never decode them; the first read of a
        field decodes that proof (decode(): every point validated) and fills all fields."""
        if len(blob) != 784 * count:
            raise ValueError(f"expected {count} proofs of 784 bytes, got {len(blob)} bytes")
        new = object.__new__
        out = []
        for i in range(count):
            p = new(cls)
            p.__dict__["_batch"] = (blob, None, i, None)
            out.append(p)
        return out

    @staticmethod
    def _unbatch(d) -> None:
        b = d.pop("_batch", None)
        if b is not None:
            raw_blob, aux_blob, i, blind = b
            d["_raw"] = raw_blob[784 * i : 784 * i + 784]
            if aux_blob is None:                      # encoded only: fields come from decode() when first read
                d["_lazy"] = True
                return
            ab = _native.RINGVRF_AUX_BYTES
            aux = aux_blob[ab * i : ab * i + ab]
            if blind is not None:
                aux = aux[:256] + blind + aux[288:]
            d["_aux"] = aux

    def __getattr__(self, name):
        d = self.__dict__
        if name not in RingVRF._FIELDS or ("_aux" not in d and "_batch" not in d and "_lazy" not in d):
            raise AttributeError(name)
        RingVRF._unbatch(d)
        if d.pop("_lazy", False):
            decoded = type(self).decode(d["_raw"])
            for nm in RingVRF._FIELDS:
                d[nm] = decoded.__dict__[nm]
            d["_snapshot"] = self._field_state()
            return d[name]
        raw, aux = d["_raw"], d.pop("_aux")
        cv = self.cv
        pt = lambda i: cv.point_type._trusted(int.from_bytes(aux[64 * i : 64 * i + 32], "little"), int.from_bytes(aux[64 * i + 32 : 64 * i + 64], "little"))
        le = lambda off: int.from_bytes(raw[off : off + 32], "little")
        d["pedersen_proof"] = PedersenVRF[cv](output_point=pt(0), blinded_pk=pt(1), result_point=pt(2), ok=pt(3), s=le(128), sb=le(160),
                                             _blinding_factor=int.from_bytes(aux[256:288], "little"))
        g1 = lambda i: None if aux[288 + 96 * i] & 0x40 else aux[288 + 96 * i : 384 + 96 * i]
        for i, nm in enumerate(("c_b", "c_accip", "c_accx", "c_accy")):
            d[nm] = Column(nm, [], _commitment=g1(i), _has_commitment=True)
        for i, nm in enumerate(("px_zeta", "py_zeta", "s_zeta", "b_zeta", "accip_zeta", "accx_zeta", "accy_zeta")):
            d[nm] = le(384 + 32 * i)
        d["c_q"] = Column("C_q", [], _commitment=g1(4), _has_commitment=True)
        d["l_zeta_omega"] = le(656)
        d["open_agg_zeta"], d["open_l_zeta_omega"] = g1(5), g1(6)
        d["_snapshot"] = self._field_state()
        return d[name]

    def __setattr__(self, name, value):
        d = self.__dict__
        if name in RingVRF._FIELDS and ("_aux" in d or "_batch" in d or "_lazy" in d):
            self.__getattr__(name)          # fill every field from the auxiliary record first: the lazy fill must not undo this write
        object.__setattr__(self, name, value)

    def _field_state(self):
        """What the encoded bytes depend on, as plain values: a natively produced proof keeps its 784 bytes only while this
        still equals the state captured when the fields were materialised (the reference's tests mutate proofs in place,
        tests/test_ark_vrf.py:146, and every later encode() / verify must see the mutation)."""
        d = self.__dict__
        ped = d.get("pedersen_proof")
        pts = tuple((q.x, q.y) for q in (ped.output_point, ped.blinded_pk, ped.result_point, ped.ok)) if ped is not None else None
        cm = lambda c: getattr(c, "_commitment", c)
        return (pts, None if ped is None else (ped.s, ped.sb), tuple(cm(d.get(nm)) for nm in ("c_b", "c_accip", "c_accx", "c_accy", "c_q")),
                tuple(d.get(nm) for nm in ("px_zeta", "py_zeta", "s_zeta", "b_zeta", "accip_zeta", "accx_zeta", "accy_zeta", "l_zeta_omega")),
                d.get("open_agg_zeta"), d.get("open_l_zeta_omega"))

    @classmethod
    def _payload_len(cls, params) -> int:
        return 7 * params.pcs.commitment_size + 8 * RING_SCALAR_LEN

    @classmethod
    def proof_len(cls) -> int:
        return PedersenVRF[cls.cv].proof_len() + cls._payload_len(RingProofParams(cv=cls.cv))

    def encode(self) -> bytes:
        d = self.__dict__
        RingVRF._unbatch(d)
        raw = d.get("_raw")
        if raw is not None:
            if "_aux" in d or "_lazy" in d or d.get("_snapshot") == self._field_state():       # fields never read, or read and unchanged
                return raw
            d.pop("_raw", None)                                                # mutated in place: the stored bytes are stale
        pcs = RingProofParams(cv=self.cv).pcs
        le = lambda v: int(v).to_bytes(RING_SCALAR_LEN, "little")
        return (self.pedersen_proof.encode()
                + b"".join(pcs.compress_g1(c.commitment) for c in (self.c_b, self.c_accip, self.c_accx, self.c_accy))
                + b"".join(le(v) for v in (self.px_zeta, self.py_zeta, self.s_zeta, self.b_zeta, self.accip_zeta, self.accx_zeta, self.accy_zeta))
                + pcs.compress_g1(self.c_q.commitment) + le(self.l_zeta_omega)
                + pcs.compress_g1(self.open_agg_zeta) + pcs.compress_g1(self.open_l_zeta_omega))

    @classmethod
    def decode(cls, proof: bytes) -> "RingVRF":
        expected = cls.proof_len()
        if len(proof) != expected:
            raise ValueError(f"invalid Ring VRF proof length: Ring VRF proof must be exactly {expected} bytes, got {len(proof)}")
        ped_len = PedersenVRF[cls.cv].proof_len()
        pedersen_proof = PedersenVRF[cls.cv].decode(proof[:ped_len])
        params = RingProofParams(cv=cls.cv)
        data, off = proof[ped_len:], 0
        size = params.pcs.commitment_size

        def commitment():
            nonlocal off
            cm = params.pcs.decompress_g1(data[off : off + size])
            off += size
            return cm

        def scalar():
            nonlocal off
            v = int.from_bytes(data[off : off + RING_SCALAR_LEN], "little")
            if v >= params.prime:
                raise ValueError("scalar is not canonical")
            off += RING_SCALAR_LEN
            return v

        def col(name):
            return Column(name=name, evals=[], _commitment=commitment(), _has_commitment=True)

        fields = [col("c_b"), col("c_accip"), col("c_accx"), col("c_accy")]
        fields += [scalar() for _ in range(7)]
        fields += [col("c_q"), scalar(), commitment(), commitment()]
        if off != len(data):
            raise ValueError(f"trailing bytes in ring proof payload: {len(data) - off}")
        return cls(pedersen_proof, *fields)

    @classmethod
    def decode_batch(cls, proofs) -> list:
        """decode() for many 784-byte proofs with two kernel launches in total: the 4B Bandersnatch points are decompressed
        and subgroup-checked by dr_bsn_decode_points, the 7B G1 points by dr_g1_decompress_batch; scalars are checked
        for canonicity on the host.  Raises ValueError like decode() if any proof is malformed."""
        blobs = [bytes(p) for p in proofs]
        expected = cls.proof_len()
        for b in blobs:
            if len(b) != expected:
                raise ValueError(f"invalid Ring VRF proof length: Ring VRF proof must be exactly {expected} bytes, got {len(b)}")
        if not blobs:
            return []
        if expected != 784:
            return [cls.decode(b) for b in blobs]
        cv = cls.cv
        ctx = runtime.context()
        order, prime = cv.curve.params.subgroup_order, RingProofParams(cv=cv).prime
        te_raw, te_ok = ctx.bsn_decode_points(b"".join(b[:128] for b in blobs), cv.curve.params.curve_id)
        if not all(te_ok):
            raise ValueError("Invalid point in proof")
        g1_pts, g1_ok = ctx.g1_decompress_batch(b"".join(b[192:384] + b[608:656] + b[688:784] for b in blobs))
        if not all(g1_ok):
            raise ValueError("invalid BLS12-381 G1 encoding")
        frm, mk = int.from_bytes, cv.point_type._trusted
        out = []
        for i, b in enumerate(blobs):
            pts = [mk(frm(te_raw[256 * i + 64 * k : 256 * i + 64 * k + 32], "little"), frm(te_raw[256 * i + 64 * k + 32 : 256 * i + 64 * k + 64], "little"))
                   for k in range(4)]
            s, sb = frm(b[128:160], "little"), frm(b[160:192], "little")
            if s >= order or sb >= order:
                raise ValueError("scalar is not canonical")
            ped = PedersenVRF[cv](output_point=pts[0], blinded_pk=pts[1], result_point=pts[2], ok=pts[3], s=s, sb=sb)
            evals = [frm(b[384 + 32 * k : 416 + 32 * k], "little") for k in range(7)]
            lzw = frm(b[656:688], "little")
            if any(v >= prime for v in evals) or lzw >= prime:
                raise ValueError("scalar is not canonical")
            g = g1_pts[7 * i : 7 * i + 7]
            cols = [Column(nm, [], _commitment=g[k], _has_commitment=True) for k, nm in enumerate(("c_b", "c_accip", "c_accx", "c_accy"))]
            out.append(cls(ped, *cols, *evals, Column("c_q", [], _commitment=g[4], _has_commitment=True), lzw, g[5], g[6]))
        return out

    # -- proving
    @classmethod
    def _prove_gen(cls, alphas, additional_data, secret_keys, producer_keys, ring, root, salts, slot=0):
        """One slice of a batch as a generator of GPU tasks: Pedersen part, then the ring part."""
        cv = cls.cv
        pedersen = yield from PedersenVRF[cv]._prove_gen(alphas, secret_keys, additional_data, salts)
        blindings = [pp._blinding_factor for pp in pedersen]
        if device_prover.supported(ring.params):
            indices = yield (lambda: ring.indices_of(producer_keys))
            payloads = yield from device_prover.ring_proofs_gen(ring, root, indices, blindings, slot=slot)
        else:       # custom PCS / domain layout: generic phase-batched prover (NTT + MSM seams only)
            payloads = yield (lambda: build_ring_proofs(ring, root, producer_keys, blindings))
        return [cls(pp, *payload) for pp, payload in zip(pedersen, payloads)]

    @classmethod
    def prove_batch(cls, alphas, additional_data, secret_keys, producer_keys, ring: Ring, ring_root: RingRoot | None = None,
                    salts=None) -> list:
        """Additive API: a batch of proofs over ONE ring; element i equals
        prove(alphas[i], additional_data[i], secret_keys[i], producer_keys[i], ring, ring_root)."""
        count = len(alphas)
        if not (len(additional_data) == len(secret_keys) == len(producer_keys) == count):
            raise ValueError("batch arguments must have equal lengths")
        if count == 0:
            return []
        cv = cls.cv
        from ..curve import scalar_mul_batch
        from ..pipeline import drive

        gen = cv.point_type.generator_point()
        # one scalar multiplication per distinct key not seen before (sk -> pk is deterministic; a small per-class memo
        # saves a latency-bound launch per call when a signer proves repeatedly)
        # the memo is keyed by a hash of the secret key: the process keeps no copy of secret material beyond the call
        tag = lambda sk: hashlib.blake2b(sk, digest_size=16, person=b"dotring-pk-memo").digest()
        sk_bytes = [bytes(sk) for sk in secret_keys]
        tag_of = {sk: tag(sk) for sk in dict.fromkeys(sk_bytes)}     # one hash per distinct key of THIS call (a local, not kept)
        tags = [tag_of[sk] for sk in sk_bytes]
        # prove_batch may run on several threads at once (application lanes): lookups, the clear() at the size
        # cap and the update all happen under one lock, and the comparison below uses this call's own snapshot
        with _PK_MEMO_LOCK:
            memo = cls.__dict__.get("_pk_memo")
            if memo is None:
                memo = {}
                cls._pk_memo = memo
            known = {t: memo[t] for t in tag_of.values() if t in memo}
        distinct = {t: sk for sk, t in tag_of.items() if t not in known}
        if distinct:
            derived = scalar_mul_batch([gen] * len(distinct), [int.from_bytes(sk, "little") for sk in distinct.values()])
            fresh = {t: pt.point_to_string() for t, pt in zip(distinct, derived)}
            known.update(fresh)
            with _PK_MEMO_LOCK:
                if len(memo) + len(fresh) > 4096:
                    memo.clear()
                memo.update(fresh)
        for t, pk in zip(tags, producer_keys):
            if pk != known[t]:
                raise ValueError("producer_key does not match secret_key")
        root = ring_root
        if root is None or root.px.coeffs is None or root.py.coeffs is None or root.s.coeffs is None or len(root.s.evals) < ring.params.domain_size:
            computed = RingRoot.from_ring(ring, ring.params)
            if root is not None and computed.encode() != root.encode():
                raise ValueError("ring_root does not match ring")
            root = computed
        if device_prover.supported(ring.params) and os.environ.get("DOTRING_NATIVE_HOST", "1") != "0":
            return cls._prove_batch_native(alphas, additional_data, secret_keys, producer_keys, ring, root, salts)
        # Python orchestration over the same kernels (custom PCS / domain layouts, DOTRING_NATIVE_HOST=0)
        if device_prover.supported(ring.params):
            device_prover.get_device_prover(ring, 0)                       # per-ring tables
        return drive(cls._prove_gen(alphas, additional_data, secret_keys, producer_keys, ring, root, salts or [b""] * count, 0))

    @classmethod
    def _prove_batch_native(cls, alphas, additional_data, secret_keys, producer_keys, ring, root, salts) -> list:
        """The batch through dr_ringvrf_prove_batch: transcripts hashed on the library's worker threads between the GPU
        phases; this method only marshals the inputs and wraps the 784-byte results."""
        cv = cls.cv
        sp = cv.curve.params
        le = lambda v: int(v).to_bytes(32, "little")
        suite = cls._suite_struct()
        indices = ring.indices_of(producer_keys)
        prefix = root.verifier_transcript_prefix_bytes()
        ab = _native.RINGVRF_AUX_BYTES

        def provers_of_the_device_set() -> list:
            """one prover of this ring per device of runtime.device_ids() (their SRS and ring tables are built on first use)"""
            ctxs = runtime.device_contexts()
            if len(ctxs) == 1:
                return [device_prover.get_device_prover(ring, 0)]
            mine, out = runtime.context(), []
            try:
                for c in ctxs:
                    runtime.set_context(c)
                    out.append(device_prover.get_device_prover(ring, 0))
            finally:
                runtime.set_context(mine)
            return out

        def prove_span(lo: int, hi: int) -> list:
            # runs on the calling thread or on a helper thread: runtime.context() / get_device_prover give each thread its own
            # stream, scratch and per-ring prover state
            # hidden rows: 12 x 48 random bytes per proof, expanded from a fresh 32-byte OS seed by the library's worker threads
            # (SHAKE256 in counter mode; os.urandom alone took 1.5 ms per 1024 proofs on the calling thread)
            zk = None if ring.params.test_vectors else _native.random_expand(secrets.token_bytes(32), 48 * 12 * (hi - lo))
            n = hi - lo
            provers = provers_of_the_device_set()
            aux = blind = None
            try:
                sk_blob = b"".join(bytes(sk) if len(sk) == 32 else le(int.from_bytes(sk, "little") % sp.subgroup_order) for sk in secret_keys[lo:hi])
                if len(provers) > 1:          # the span sharded over the process's device set, all proofs back in this buffer
                    raw, aux = _native.ringvrf_prove_batch_multi(provers, suite, alphas[lo:hi], additional_data[lo:hi], salts[lo:hi] if salts else None,
                                                                 sk_blob, indices[lo:hi], prefix, zk)
                else:
                    raw, aux = provers[0].ringvrf_prove_batch(suite, alphas[lo:hi], additional_data[lo:hi], salts[lo:hi] if salts else None,
                                                              sk_blob, indices[lo:hi], prefix, zk)
                blind = _native.aux_take_blindings(aux, n)          # the shared auxiliary string below carries no secret
                return cls._from_batch(ctypes.string_at(raw, 784 * n), ctypes.string_at(aux, ab * n), n, ctypes.string_at(blind, 32 * n))
            finally:
                # the per-thread buffers are reused: wiped whether or not the native call succeeded
                for buf in (aux, blind):
                    if buf is not None:
                        _native.wipe(buf)
                if aux is None:
                    _native.wipe_thread_buffer("prove_aux")

        count = len(alphas)
        out = []
        step = device_prover.MAX_DEVICE_BATCH * len(runtime.device_ids())
        for lo in range(0, count, step):
            out.extend(prove_span(lo, min(count, lo + step)))
        return out

    @classmethod
    def prove(cls, alpha: bytes, additional_data: bytes, secret_key: bytes, producer_key: bytes, ring: Ring,
              ring_root: RingRoot | None = None, salt: bytes = b"") -> "RingVRF":
        return cls.prove_batch([alpha], [additional_data], [secret_key], [producer_key], ring, ring_root, [salt])[0]

    @classmethod
    def parse_keys(cls, keys: bytes) -> list:
        size = point_len(cls.cv)
        if len(keys) % size != 0:
            raise ValueError(f"invalid concatenated key length: expected multiple of {size}, got {len(keys)}")
        return [keys[size * i : size * (i + 1)] for i in range(len(keys) // size)]

    # -- verification
    def _linear_claims(self, message, ring: Ring, ring_root: RingRoot):
        cv = ring.params.cv
        if isinstance(message, (bytes, bytearray)):
            try:
                message = cv.point_type.string_to_point(bytes(message))
            except ValueError as exc:
                raise ValueError("Invalid message point") from exc
        aux = cv.curve.params.auxiliary_points
        if not aux.accumulator_base:
            raise ValueError("Curve does not have an accumulator base point for Ring VRF")
        seed = cv.point_type(*aux.accumulator_base)
        return linear_pcs_verifications(self, ring_root.fixed_commitments(), message, seed + message, seed, ring.params,
                                        ring_root.verifier_transcript_prefix())

    def verify_ring_proof(self, message, ring: Ring, ring_root: RingRoot) -> bool:
        if not ring_root.matches_ring(ring):
            return False
        return bool(ring.params.pcs.batch_verify_linear_preconverted(list(self._linear_claims(message, ring, ring_root))))

    def verify(self, input: bytes, ad_data: bytes, ring: Ring, ring_root: RingRoot) -> bool:
        cls = type(self)
        if cls._native_verifier_serves(ring, ring_root):
            # one proof through the native verifier (dr_ringvrf_verify_batch with B = 1): below DOTRING_VERIFY_HOST_MAX proofs it
            # decodes the points and folds the two small G1 MSMs on host cores while the Pedersen checks run on the GPU — every
            # kernel launch chain it would otherwise wait for is 0.7 - 2 ms of pure latency
            return ring_root.matches_ring(ring) and cls._batch_verify_native([self], [input], [ad_data], ring, ring_root)
        p_ok = self.pedersen_proof.verify(input, ad_data)
        r_ok = self.verify_ring_proof(self.pedersen_proof.blinded_pk, ring, ring_root)
        return p_ok and r_ok

    @classmethod
    def _native_verifier_serves(cls, ring: Ring, ring_root: RingRoot) -> bool:
        return (device_prover.supported(ring.params) and os.environ.get("DOTRING_NATIVE_HOST", "1") != "0"
                and cls.proof_len() == 784 and ring_root.params is not None)

    @classmethod
    def proof_to_hash(cls, gamma, mul_cofactor: bool = False) -> bytes:
        return PedersenVRF[cls.cv].proof_to_hash(gamma, mul_cofactor)

    @classmethod
    def _suite_struct(cls):
        sp = cls.cv.curve.params
        le = lambda v: int(v).to_bytes(32, "little")
        gen, bb = sp.generator, sp.auxiliary_points.blinding_base
        return _native.vrf_suite(sp.suite_id, sp.xof, le(gen[0]) + le(gen[1]), le(bb[0]) + le(bb[1]), sp.curve_id)

    @classmethod
    def _shared_encoding(cls, proofs):
        """The encoded bytes of `proofs` without touching them one by one, when they are untouched consecutive proofs of ONE native
        batch (prove_batch's output, a gathered shard, a slice of either): a slice of the shared string; None otherwise."""
        count = len(proofs)
        first = proofs[0].__dict__.get("_batch") if count and type(proofs[0]) is cls else None
        if first is None:
            return None
        blob, i0 = first[0], first[2]
        if 784 * (i0 + count) > len(blob):
            return None
        for i, p in enumerate(proofs):
            if type(p) is not cls:
                return None
            b = p.__dict__.get("_batch")
            if b is None or b[0] is not blob or b[2] != i0 + i:
                return None
        return blob if i0 == 0 and len(blob) == 784 * count else blob[784 * i0 : 784 * (i0 + count)]

    @classmethod
    def encode_batch(cls, proofs) -> bytes:
        """b"".join(p.encode() for p in proofs); for the untouched output of one prove_batch call that is the string they share."""
        shared = cls._shared_encoding(proofs) if proofs else b""
        return shared if shared is not None else b"".join(p.encode() for p in proofs)

    @classmethod
    def _native_vk(cls, ring: Ring, ring_root: RingRoot):
        """dr_ring_verifier_key of (ring, root), kept on the root object."""
        params = ring.params
        pcs = params.pcs
        vk = ring_root.__dict__.get("_native_vk")
        if vk is None:
            srs = pcs._srs()
            seed = params.cv.curve.params.auxiliary_points.accumulator_base
            le = lambda v: int(v).to_bytes(32, "little")
            vk = _native.ring_verifier_key(
                params.domain_size.bit_length() - 1, params.omega, le(seed[0]) + le(seed[1]),
                b"".join(pcs.serialize_g1_uncompressed(c) for c in ring_root.fixed_commitments()), srs.g1_raw[:96],
                srs.g2_raw[0] + srs.g2_raw[1], ring_root.verifier_transcript_prefix_bytes())
            ring_root.__dict__["_native_vk"] = vk
        return vk

    @classmethod
    def _batch_verify_native(cls, proofs, inputs, additional_data, ring: Ring, ring_root: RingRoot) -> bool:
        """dr_ringvrf_verify_batch over the encoded proofs: point decoding/validation on the GPU, transcripts on the
        library's worker threads, one Bandersnatch MSM + two G1 MSMs + one pairing equation for the whole batch."""
        vk = cls._native_vk(ring, ring_root)
        suite = cls._suite_struct()
        count = len(proofs)
        if not (count == len(inputs) == len(additional_data)):
            return False
        # the untouched output of ONE prove_batch call (or a run of it), in order: its encoded bytes already lie in one string
        joined = cls._shared_encoding(proofs)
        blobs = None
        if joined is None:
            try:
                blobs = [p.encode() for p in proofs]
                if any(len(b) != 784 for b in blobs):
                    return False
            except (AttributeError, TypeError, ValueError):
                return False
        ctxs = runtime.device_contexts()
        step = device_prover.MAX_DEVICE_BATCH * len(ctxs)
        for lo in range(0, count, step):
            hi = min(count, lo + step)
            part = joined[784 * lo : 784 * hi] if joined is not None else b"".join(blobs[lo:hi])
            if joined is not None and lo == 0 and hi == count:
                part = joined
            ins, ads_ = [bytes(x) for x in inputs[lo:hi]], [bytes(x) for x in additional_data[lo:hi]]
            if len(ctxs) > 1:                 # the span sharded over the process's device set, the verdicts AND-ed
                ok = _native.ringvrf_verify_batch_multi(ctxs, suite, vk, part, ins, ads_, None, secrets.token_bytes(32))
            else:
                ok = ctxs[0].ringvrf_verify_batch(suite, vk, part, ins, ads_, None, secrets.token_bytes(32))
            if not ok:
                return False
        return True

    @classmethod
    def _verify_each_native(cls, joined: bytes, inputs, additional_data, ring: Ring, ring_root: RingRoot, stats: dict) -> list:
        """dr_ringvrf_verify_each over the 784-byte strings of `joined`: the phases of _batch_verify_native, then per-proof claim points and their sum
        tree on the GPU and pairings only where a subtree fails.  Spans longer than one native call are chunked as there."""
        vk = cls._native_vk(ring, ring_root)
        suite = cls._suite_struct()
        ctxs = runtime.device_contexts()
        step = device_prover.MAX_DEVICE_BATCH * len(ctxs)
        out = []
        count = len(joined) // 784
        for lo in range(0, count, step):
            hi = min(count, lo + step)
            part = joined if lo == 0 and hi == count else joined[784 * lo : 784 * hi]
            ins, ads_ = [bytes(x) for x in inputs[lo:hi]], [bytes(x) for x in additional_data[lo:hi]]
            if len(ctxs) > 1:                 # the span sharded over the process's device set, every shard its slice of the verdicts
                verdicts, st = _native.ringvrf_verify_each_multi(ctxs, suite, vk, part, ins, ads_, None, secrets.token_bytes(32))
            else:
                verdicts, st = ctxs[0].ringvrf_verify_each(suite, vk, part, ins, ads_, None, secrets.token_bytes(32))
            out.extend(verdicts)
            stats["pairings"] += st[0]
            stats["excluded"] += st[1]
            stats["depth"] = max(stats["depth"], st[2])
        return out

    @classmethod
    def verify_each(cls, proofs, inputs, additional_data, ring: Ring, ring_root: RingRoot, *, stats: dict | None = None) -> list:
        """A verdict per proof from one batch pass: [p.verify(i, ad, ring, ring_root) for ...] from one pairing equation when all
        proofs hold (measured on one MI355X at 1024 proofs, ring 1024: 1.9 x batch_verify's time) and about 2 log2(count) more per
        failing proof (DESIGN 8ah has the figures).  Unequal lengths raise ValueError; a root that does not match the
        ring gives all False; a proof object that does not encode to 784 bytes is False and the rest still go through.  `stats`
        (optional dict) receives "pairings" (pairing equations — or batch_verify calls on the fallback route — evaluated),
        "excluded" (malformed proofs left out before the fold) and "depth" (of the sum tree)."""
        count = len(proofs)
        if not (count == len(inputs) == len(additional_data)):
            raise ValueError("proofs, inputs and additional_data must have equal lengths")
        st = {"pairings": 0, "excluded": 0, "depth": 0}
        try:
            if count == 0:
                return []
            if not ring_root.matches_ring(ring):
                return [False] * count
            if not cls._native_verifier_serves(ring, ring_root):
                # the same descent in Python over batch_verify (which answers False for a span with a malformed member)
                def holds(lo, hi):
                    try:
                        return bool(cls.batch_verify(proofs[lo:hi], inputs[lo:hi], additional_data[lo:hi], ring, ring_root))
                    except (AttributeError, TypeError, ValueError):       # an object without a proof's fields
                        return False

                verdicts, st["pairings"] = verify_tree_descent(count, holds)
                st["depth"] = max(count - 1, 0).bit_length()
                return verdicts
            # the untouched output of ONE prove_batch call (or a run of it), in order: its encoded bytes already lie in one string
            joined = cls._shared_encoding(proofs)
            if joined is not None:
                return [bool(v) for v in cls._verify_each_native(joined, inputs, additional_data, ring, ring_root, st)]
            blobs, where = [], []
            for i, p in enumerate(proofs):
                try:
                    b = p.encode()
                except (AttributeError, TypeError, ValueError):
                    continue
                if isinstance(b, (bytes, bytearray)) and len(b) == 784:
                    blobs.append(bytes(b))
                    where.append(i)
            st["excluded"] = count - len(where)
            verdicts = [False] * count
            got = cls._verify_each_native(b"".join(blobs), [inputs[i] for i in where], [additional_data[i] for i in where], ring, ring_root, st)
            for i, v in zip(where, got):
                verdicts[i] = bool(v)
            return verdicts
        finally:
            if stats is not None:
                stats.update(st)

    @classmethod
    def batch_verify(cls, proofs, inputs, additional_data, ring: Ring, ring_root: RingRoot) -> bool:
        if not ring_root.matches_ring(ring):
            return False
        if cls._native_verifier_serves(ring, ring_root):
            return cls._batch_verify_native(proofs, inputs, additional_data, ring, ring_root)
        if not PedersenVRF[cls.cv].batch_verify([p.pedersen_proof for p in proofs], inputs, additional_data):
            return False
        claims = []
        try:
            params = ring.params
            cv = params.cv
            seed = cv.point_type(*cv.curve.params.auxiliary_points.accumulator_base)
            prefix = ring_root.verifier_transcript_prefix()
            fixed = ring_root.fixed_commitments()
            domain = params.domain
            replays = [replay_challenges(pr, pr.pedersen_proof.blinded_pk, params, prefix) for pr in proofs]
            # one modular inversion for the whole batch instead of three per proof
            dens = [d for rp in replays for d in zeta_denominators(rp[3], domain, params.prime)]
            invs = batch_inverse(dens, params.prime)
            for j, (proof, rp) in enumerate(zip(proofs, replays)):
                relation = proof.pedersen_proof.blinded_pk
                claims.extend(linear_pcs_verifications(proof, fixed, relation, seed + relation, seed, params, prefix, replay=rp,
                                                       inverses=invs[3 * j : 3 * j + 3], domain=domain))
        except (AssertionError, AttributeError, TypeError, ValueError):
            return False
        return bool(ring.params.pcs.batch_verify_linear_preconverted(claims))
