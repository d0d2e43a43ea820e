"""Pedersen VRF (dot_ring/vrf/pedersen/vrf.py:32-243).  Envelope: gamma || Y_bar || R || O_k || s || s_b."""
from __future__ import annotations

import os
from dataclasses import dataclass

from .. import _native, runtime
from ..curve import msm_groups, scalar_mul_batch
from .base import VRF
from .codec import dec_points, dec_scalar, dec_scalar_mod, enc_point, enc_scalar, point_len, scalar_len
from .primitives import (CHALLENGE_LEN, DomSep, VrfIo, challenge, nonce, point_to_hash, squeeze_transcript_bytes,
                         vrf_transcript)


@dataclass(frozen=True)
class PedersenVRF(VRF):
    output_point: object
    blinded_pk: object
    result_point: object
    ok: object
    s: int
    sb: int
    _blinding_factor: int = 0

    @classmethod
    def proof_len(cls) -> int:
        return 4 * point_len(cls.cv) + 2 * scalar_len(cls.cv)

    @classmethod
    def _blinding_base(cls):
        bb = cls.cv.curve.params.auxiliary_points.blinding_base
        if not bb:
            raise ValueError("Curve does not have a blinding base point for Pedersen VRF")
        return cls.cv.point_type(*bb)

    @classmethod
    def decode(cls, proof: bytes) -> "PedersenVRF":
        pl, sl = point_len(cls.cv), scalar_len(cls.cv)
        if len(proof) != cls.proof_len():
            raise ValueError(f"invalid Pedersen VRF proof length: expected {cls.proof_len()}, got {len(proof)}")
        try:
            out, blinded, r, ok = dec_points(cls.cv, [proof[pl * i : pl * (i + 1)] for i in range(4)])
        except ValueError as exc:
            raise ValueError("Invalid point in proof") from exc
        s = dec_scalar(cls.cv, proof[4 * pl : 4 * pl + sl])
        sb = dec_scalar(cls.cv, proof[4 * pl + sl :])
        return cls(output_point=out, blinded_pk=blinded, result_point=r, ok=ok, s=s, sb=sb)

    def encode(self) -> bytes:
        return (enc_point(self.output_point) + enc_point(self.blinded_pk) + enc_point(self.result_point)
                + enc_point(self.ok) + enc_scalar(self.cv, self.s) + enc_scalar(self.cv, self.sb))

    @classmethod
    def blinding_scalar(cls, secret_scalar: int, transcript) -> int:
        t = transcript.copy()
        t.absorb(bytes([DomSep.PEDERSEN_BLINDING]))
        return nonce(cls.cv, secret_scalar, t)

    @classmethod
    def _prove_gen(cls, alphas, secret_keys, additional_data, salts=None):
        """Generator form of prove_batch (see dot_ring_amd/pipeline.py): yields GPU callables, returns the proofs.
        Three device round trips for the whole batch (the transcript forces the three phases)."""
        cv = cls.cv
        count = len(alphas)
        salts = salts or [b""] * count
        gen, bb = cv.point_type.generator_point(), cls._blinding_base()
        order = cv.curve.params.subgroup_order
        xs = [dec_scalar_mod(cv, sk) for sk in secret_keys]
        tai = cv.curve.params.e2c == "tai"
        us = None if tai else cv.point_type.hash_to_field_pairs(alphas, salts)

        def first():
            inputs = cv.point_type.encode_to_curve_batch(alphas, salts) if tai else cv.point_type.encode_to_curve_from_field(us)
            return inputs, scalar_mul_batch(inputs, xs)                                  # I_i, O_i = x_i * I_i

        inputs, outs = yield first
        transcripts, blindings = [], []
        for i in range(count):
            t, _ = vrf_transcript(cv, DomSep.PEDERSEN_VRF, [VrfIo(inputs[i], outs[i])], additional_data[i])
            transcripts.append(t)
            blindings.append(cls.blinding_scalar(xs[i], t))
        # Y_bar_i = x_i*G + b_i*B  (= public key + b*B): one grouped 2-term MSM launch for the whole batch
        gb = [gen, bb] * count
        blind_scalars = [s for pair in zip(xs, blindings) for s in pair]
        blinded = yield (lambda: msm_groups(gb, blind_scalars, 2))
        ks, kbs = [], []
        for i in range(count):
            transcripts[i].absorb(enc_point(blinded[i]))
            ks.append(nonce(cv, xs[i], transcripts[i]))
            kbs.append(nonce(cv, blindings[i], transcripts[i]))
        # R_i = k_i*G + kb_i*B and Ok_i = k_i*I_i + 0*I_i in ONE grouped launch
        pts = gb + [p for inp in inputs for p in (inp, inp)]
        scs = [s for pair in zip(ks, kbs) for s in pair] + [s for k in ks for s in (k, 0)]
        third = yield (lambda: msm_groups(pts, scs, 2))
        proofs = []
        for i in range(count):
            result_point, ok = third[i], third[count + i]
            c = challenge(cv, [result_point, ok], transcripts[i])
            proofs.append(cls(output_point=outs[i], blinded_pk=blinded[i], result_point=result_point, ok=ok,
                              s=(ks[i] + c * xs[i]) % order, sb=(kbs[i] + c * blindings[i]) % order,
                              _blinding_factor=blindings[i]))
        return proofs

    @classmethod
    def _suite_struct(cls):
        sp = cls.cv.curve.params
        le = lambda v: int(v).to_bytes(32, "little")
        gen, bb = sp.generator, sp.auxiliary_points.blinding_base
        return _native.vrf_suite(sp.suite_id, sp.hash_fn, le(gen[0]) + le(gen[1]), le(bb[0]) + le(bb[1]), sp.curve_id)

    @classmethod
    def prove_batch(cls, alphas, secret_keys, additional_data, salts=None) -> list:
        """Additive API: element i equals prove(alphas[i], secret_keys[i], additional_data[i]).
        Default: one dr_pedersen_prove_batch call (transcripts on the library's worker threads);
        DOTRING_NATIVE_HOST=0 keeps the Python orchestration over the same kernels."""
        count = len(alphas)
        if not (len(secret_keys) == len(additional_data) == count) or (salts is not None and len(salts) != count):
            raise ValueError("batch arguments must have equal lengths")
        if count == 0:
            return []
        if (os.environ.get("DOTRING_NATIVE_HOST", "1") == "0" or not cls.cv.curve.params.auxiliary_points.blinding_base
                or cls.cv.point_type._WIDE):          # (Ed448: dr_pedersen_prove_batch carries 32-byte scalars)
            from ..pipeline import drive

            return drive(cls._prove_gen(alphas, secret_keys, additional_data, salts))
        cv = cls.cv
        order = cv.curve.params.subgroup_order
        le = lambda v: int(v).to_bytes(32, "little")
        sks = b"".join(bytes(sk) if len(sk) == 32 else le(int.from_bytes(sk, "little") % order) for sk in secret_keys)
        ctx = runtime.context()
        suite = cls._suite_struct()
        out, frm, mk = [], int.from_bytes, cv.point_type._trusted
        step, ab, plen, sof = 65536, _native.PEDERSEN_AUX_BYTES, cls.proof_len(), 4 * point_len(cv)
        for lo in range(0, count, step):
            hi = min(count, lo + step)
            raw, aux = ctx.pedersen_prove_batch(suite, [bytes(a) for a in alphas[lo:hi]], [bytes(a) for a in additional_data[lo:hi]],
                                                salts[lo:hi] if salts else None, sks[32 * lo : 32 * hi])
            for i in range(hi - lo):
                a, r = aux[ab * i : ab * i + ab], raw[plen * i : plen * i + plen]
                pts = [mk(frm(a[64 * k : 64 * k + 32], "little"), frm(a[64 * k + 32 : 64 * k + 64], "little")) for k in range(4)]
                out.append(cls(output_point=pts[0], blinded_pk=pts[1], result_point=pts[2], ok=pts[3], s=frm(r[sof : sof + 32], "little"),
                               sb=frm(r[sof + 32 : sof + 64], "little"), _blinding_factor=frm(a[256:288], "little")))
        return out

    @classmethod
    def prove(cls, alpha: bytes, secret_key: bytes, additional_data: bytes, salt: bytes = b"") -> "PedersenVRF":
        return cls.prove_batch([alpha], [secret_key], [additional_data], [salt])[0]

    def _challenge(self, input: bytes, additional_data: bytes, salt: bytes, input_point=None):
        cv = self.cv
        if input_point is None:
            input_point = cv.point_type.encode_to_curve(input, salt)
        transcript, merged = vrf_transcript(cv, DomSep.PEDERSEN_VRF, [VrfIo(input_point, self.output_point)], additional_data)
        transcript.absorb(enc_point(self.blinded_pk))
        return input_point, merged, challenge(cv, [self.result_point, self.ok], transcript)

    def verify(self, input: bytes, additional_data: bytes, salt: bytes = b"") -> bool:
        cv = self.cv
        sp = cv.curve.params
        if (sp.curve_id == _native.CURVE_BANDERSNATCH and sp.e2c != "tai" and sp.auxiliary_points.blinding_base
                and os.environ.get("DOTRING_NATIVE_HOST", "1") != "0" and os.environ.get("DOTRING_SMALL_HOST_MAX", "64") != "0"):
            # one proof: the library checks both relations on a host core (dr_pedersen_verify_batch with B = 1, csrc/hostsigma.hpp) — two
            # kernel launch chains otherwise
            try:
                blob = self.encode()
            except (AttributeError, TypeError, ValueError, OverflowError):
                return False
            return runtime.context().pedersen_verify_batch(self._suite_struct(), blob, [bytes(input)], [bytes(additional_data)], [bytes(salt)])
        _, merged, c = self._challenge(input, additional_data, salt)
        # the two checks  s*I - c*O == O_k  and  s*G + s_b*B - c*Y_bar == R  as ONE launch of two 3-term groups
        gen = cv.point_type.generator_point()
        lhs1, lhs2 = msm_groups([merged.input, merged.output, gen, gen, self._blinding_base(), self.blinded_pk],
                                [self.s, -c, 0, self.s, self.sb, -c], 3)
        return lhs1 == self.ok and lhs2 == self.result_point

    def verify_unblinding(self, public_key: bytes, blinding_factor: int) -> bool:
        from .codec import dec_point

        if not 0 <= blinding_factor < self.cv.curve.params.subgroup_order:
            return False
        return dec_point(self.cv, public_key) + self._blinding_base() * blinding_factor == self.blinded_pk

    @classmethod
    def proof_to_hash(cls, gamma, mul_cofactor: bool = False) -> bytes:
        if mul_cofactor:
            # gamma * cofactor (tiny.py:88, pedersen/vrf.py:167): 4 = two doublings on Bandersnatch, 8 = three on JubJub
            for _ in range(cls.cv.curve.params.cofactor.bit_length() - 1):
                gamma = gamma.double()
        return point_to_hash(cls.cv, gamma)

    @classmethod
    def batch_verify(cls, proofs, inputs, additional_data, salts=None) -> bool:
        """pedersen/vrf.py:171 — one (5B+2)-point MSM on the GPU instead of 2B small ones."""
        cv = cls.cv
        if salts is None:
            salts = [b""] * len(proofs)
        if (os.environ.get("DOTRING_NATIVE_HOST", "1") != "0" and cv.curve.params.auxiliary_points.blinding_base
                and not cv.point_type._WIDE):
            try:
                if not (len(proofs) == len(inputs) == len(additional_data) == len(salts)):
                    return False
                blobs = [p.encode() for p in proofs]
                if any(len(b) != cls.proof_len() for b in blobs):
                    return False
                ins, adl, sl = [bytes(x) for x in inputs], [bytes(x) for x in additional_data], [bytes(x) for x in salts]
            except (AttributeError, TypeError, ValueError):
                return False
            ctx, suite, step = runtime.context(), cls._suite_struct(), 65536
            return all(ctx.pedersen_verify_batch(suite, b"".join(blobs[lo : lo + step]), ins[lo : lo + step], adl[lo : lo + step], sl[lo : lo + step])
                       for lo in range(0, len(blobs), step))
        order = cv.curve.params.subgroup_order
        items, coeff_bytes = [], bytearray()
        try:
            if not (len(proofs) == len(inputs) == len(additional_data) == len(salts)):
                raise ValueError("batch arguments must have equal lengths")
            input_points = cv.point_type.encode_to_curve_batch(list(inputs), list(salts))      # one launch for all proofs
            for proof, input_value, ad, salt, ipt in zip(proofs, inputs, additional_data, salts, input_points):
                input_point, _, c = proof._challenge(input_value, ad, salt, ipt)
                items.append((proof, input_point, c))
                coeff_bytes += enc_scalar(cv, c) + enc_scalar(cv, proof.s) + enc_scalar(cv, proof.sb)
        except (AttributeError, TypeError, ValueError):
            return False
        if not items:
            return True
        absorbed = bytes(cv.curve.params.suite_id) + bytes([DomSep.BATCH_VERIFY]) + bytes(coeff_bytes)
        weights = squeeze_transcript_bytes(cv.curve.params.hash_fn, absorbed, 2 * CHALLENGE_LEN * len(items))
        points, scalars = [], []
        gen_scalar = blind_scalar = 0
        for index, (proof, input_point, c) in enumerate(items):
            off = 2 * CHALLENGE_LEN * index
            w_io = dec_scalar_mod(cv, weights[off : off + CHALLENGE_LEN])
            w_cm = dec_scalar_mod(cv, weights[off + CHALLENGE_LEN : off + 2 * CHALLENGE_LEN])
            points += [proof.ok, proof.output_point, input_point, proof.result_point, proof.blinded_pk]
            scalars += [w_io, w_io * c, -w_io * proof.s, w_cm, w_cm * c]
            gen_scalar = (gen_scalar - w_cm * proof.s) % order
            blind_scalar = (blind_scalar - w_cm * proof.sb) % order
        if gen_scalar:
            points.append(cv.point_type.generator_point())
            scalars.append(gen_scalar)
        if blind_scalar:
            points.append(cls._blinding_base())
            scalars.append(blind_scalar)
        return cv.point_type.msm(points, scalars).is_identity()
