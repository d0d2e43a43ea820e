// The ring protocol's shape, host only (plain C++): where the parts of an encoded Ring-VRF proof and of its auxiliary record lie, the
// order in which the batch verifier gathers a proof's G1 points, and the Fiat-Shamir schedule of the ring proof.  The batch prover and
// the batch verifier (capi_batch.hip) write and read through these names and run the one schedule below, so neither the layout nor
// the transcript can drift between them; tests/native/ring_fs_check.cpp checks the schedule against the Python reference's.
#pragma once
#include "hostproto.hpp"

namespace drh {
namespace ringfmt {
// ---- the encoded proof: the Pedersen VRF proof (pedersen/vrf.py:86-126, 32-byte points), then the ring proof's payload
// (proof_payload.py:68-117).  Offsets, each part behind the one before it:
constexpr size_t PED_POINTS = 0, PED_POINTS_BYTES = 4 * 32;          // O, Y_bar, R, O_k
constexpr size_t PED_SCALARS = PED_POINTS + PED_POINTS_BYTES;        // s, s_b
constexpr size_t COMMITS = PED_SCALARS + 2 * 32, COMMITS_BYTES = 4 * 48;     // C_b, C_accip, C_accx, C_accy compressed
constexpr size_t EVALS = COMMITS + COMMITS_BYTES, EVALS_BYTES = 7 * 32;      // px, py, s, b, accip, accx, accy at zeta
constexpr size_t CQ = EVALS + EVALS_BYTES;                           // C_q compressed
constexpr size_t L_ZW = CQ + 48;                                     // l(zeta * omega)
constexpr size_t OPENS = L_ZW + 32, OPENS_BYTES = 2 * 48;            // Phi_zeta, Phi_zeta_omega compressed
constexpr size_t PROOF_BYTES = OPENS + OPENS_BYTES;
static_assert(COMMITS == 192 && PROOF_BYTES == 784, "a Ring-VRF proof is 192 + 592 bytes");
// ---- the prover's auxiliary record (DR_RINGVRF_AUX_BYTES of dotring_hip.h): the four Pedersen points affine (4 x 64), the blinding
// factor, the seven G1 points serialised uncompressed (96 bytes each)
constexpr size_t AUX_BLIND = 4 * 64, AUX_COMMITS = AUX_BLIND + 32, AUX_CQ = AUX_COMMITS + 4 * 96, AUX_OPENS = AUX_CQ + 96;
constexpr size_t AUX_BYTES = AUX_OPENS + 2 * 96;
static_assert(AUX_BYTES == 960, "the auxiliary record is 288 + 7 * 96 bytes");
// ---- the verifier's G1 points of one proof in the order it gathers them (bases and scalars of both folds follow it); behind all
// proofs the G_FIXED points C_px, C_py, C_s and G1[0]
constexpr size_t G_COMMITS = 0, G_CQ = 4, G_OPENS = 5, G_PER_PROOF = 7, G_FIXED = 4;
static_assert(G_PER_PROOF * 48 == COMMITS_BYTES + 48 + OPENS_BYTES, "every G1 point of the payload is gathered");
// ---- per proof: the challenges of the three rounds, and dr_ring_prove_evals' record (the seven evaluations, then l(zeta * omega))
constexpr size_t ALPHAS_BYTES = 7 * 32, NUS_BYTES = 8 * 32, EVAL_REC = EVALS_BYTES + 32;
}  // namespace ringfmt

// The transcripts of proofs 4g .. 4g + 3 of a batch of B proofs through the ring proof's three rounds (phases.py:49
// derive_challenges_after_vk) — FsTranscript4: four Keccak states per vector instruction.  The last group repeats proof B - 1 in its
// spare slots, whose (identical) results land on the same bytes.  The prover runs a round between two GPU phases, the verifier all
// three in a row.  A proof's inputs come from the callers' records through functions of the proof's index — at(i): pointer to the
// bytes, ser(i, out): writes a serialize() form — and its challenges go to record i of the callers' arrays (32-byte values, LE).
struct RingFsGroup {
    FsTranscript4 t;
    size_t idx[4];
    RingFsGroup(const FsTranscript4& base, size_t g, size_t B) : t(base) {
        for (size_t k = 0; k < 4; k++) idx[k] = std::min(4 * g + k, B - 1);
    }
    static size_t groups(size_t B) { return (B + 3) / 4; }

    template <class Instance, class Cols>
    void round_alphas(Instance&& instance, Cols&& cols, uint8_t* alphas) {
        absorb("instance", 64, instance);
        absorb_ser<4 * 96>("committed_cols", cols);
        squeeze("constraints_aggregation", 7, alphas);
    }
    template <class Cq>
    void round_zeta(Cq&& cq, uint8_t* zetas) {
        absorb_ser<96>("quotient", cq);
        squeeze("evaluation_point", 1, zetas);
    }
    template <class Evals, class Lzw>
    void round_nus(Evals&& evals, Lzw&& l_zw, uint8_t* nus) {
        absorb("register_evaluations", ringfmt::EVALS_BYTES, evals);
        absorb("shifted_linearization_evaluation", 32, l_zw);
        squeeze("kzg_aggregation", 8, nus);
    }

  private:
    template <class At>
    void absorb(const char* label, size_t len, At&& at) {
        const uint8_t* in[4];
        for (int k = 0; k < 4; k++) in[k] = at(idx[k]);
        t.absorb_labeled(label, in, len);
    }
    template <size_t LEN, class Ser>
    void absorb_ser(const char* label, Ser&& ser) {
        uint8_t buf[4][LEN];
        const uint8_t* in[4];
        for (int k = 0; k < 4; k++) { ser(idx[k], buf[k]); in[k] = buf[k]; }
        t.absorb_labeled(label, in, LEN);
    }
    void squeeze(const char* label, int n, uint8_t* all) {      // n challenges per proof, to all + 32 n i
        uint8_t* out[4];
        for (int k = 0; k < 4; k++) out[k] = all + 32 * (size_t)n * idx[k];
        t.challenges(label, n, out);
    }
};

}  // namespace drh
