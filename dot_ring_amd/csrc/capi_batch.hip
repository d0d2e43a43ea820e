// libdotring_hip.so — C ABI, part 4 of 11: native batch orchestration.  Pedersen / IETF / Ring-VRF prove_batch and
// batch_verify run the whole protocol in the library: GPU phases through the entry points of the other parts, the hashing
// between them on worker threads (hosthash.hpp, hostproto.hpp).  The VRF transcripts are hostsigma.hpp's, the Ring-VRF proof's
// layout and the ring proof's Fiat-Shamir schedule hostring.hpp's: prover and verifier share one copy of each.
#include "capi_internal.hpp"
#include <atomic>
#include <condition_variable>
#include "hostsigma.hpp"
#include "verify_tree.hpp"

using namespace dri;
namespace rf = drh::ringfmt;
static_assert(rf::AUX_BYTES == DR_RINGVRF_AUX_BYTES, "hostring.hpp describes the auxiliary record of dotring_hip.h");

// The whole batch in one call: Pedersen VRF part (pedersen/vrf.py:86-126) then the ring proof
// (proof_builder.py:38-315) — GPU phases through the entry points above, the hashing between them on worker threads.
// Pedersen VRF prover for a batch (pedersen/vrf.py:86-126): head() = hash-to-curve, outputs, transcripts and blinding
// factors (what the ring proof needs); tail() = blinded keys, nonces, R / O_k, challenge, responses and the 192 encoded
// bytes.  The two halves may run on different contexts (streams) of the same GPU.
struct PedersenBatch {
    const drh::VrfSuite& su;
    size_t B;
    std::vector<uint8_t> xs, inputs, outs, blind, sc, ybar, ks, sc3, third;
    std::vector<uint8_t> outs_sw;            // SW suite: O in SW coordinates (its encoding and aux record)
    std::vector<drh::Bytes> tr;
    PedersenBatch(const drh::VrfSuite& s, size_t b) : su(s), B(b) {}
    ~PedersenBatch() {          // secret scalars, blinding factors and nonces (and the scalar vectors built from them) do not outlive the call
        for (std::vector<uint8_t>* v : {&xs, &blind, &ks, &sc, &sc3})
            if (!v->empty()) explicit_bzero(v->data(), v->size());
    }

    int head(dr_ctx* ctx, const uint8_t* alphas, const uint64_t* alpha_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts,
             const uint64_t* salt_off, const uint8_t* secret_scalars, PhaseTrace& tr_, const std::function<void()>* while_waiting = nullptr) {
        const drh::Mod256& mn = su.cv->n;
        // 1. secrets mod n
        xs.resize(B * 32);
        for (size_t i = 0; i < B; i++) {
            uint64_t x[4];
            mn.reduce_bytes(secret_scalars + 32 * i, 32, false, x);
            drh::store_le32(x, xs.data() + 32 * i);
        }
        // 2. I_i = encode_to_curve(salt || alpha), O_i = x_i * I_i
        inputs.resize(B * 64); outs.resize(B * 64);
        TRY(encode_and_mul(ctx, su, B, alphas, alpha_off, salts, salt_off, xs.data(), inputs.data(), outs.data(), while_waiting));
        tr_.mark("encode+x*I");
        // the SW suite encodes the SW images: (I_i, O_i) mapped pairwise, one inversion per proof
        std::vector<uint8_t> io_store;
        const uint8_t* io_c = nullptr;
        if (su.cv->sw) {
            std::vector<uint8_t> io(B * 128);
            for (size_t i = 0; i < B; i++) {
                std::memcpy(io.data() + 128 * i, inputs.data() + 64 * i, 64);
                std::memcpy(io.data() + 128 * i + 64, outs.data() + 64 * i, 64);
            }
            TRY(suite_coords(ctx, su, io.data(), 2 * B, 2, io_store, &io_c));
            outs_sw.resize(B * 64);
            for (size_t i = 0; i < B; i++) std::memcpy(outs_sw.data() + 64 * i, io_c + 128 * i + 64, 64);
        }
        // 3. transcripts, blinding factors
        tr.assign(B, drh::Bytes());
        blind.resize(B * 32); sc.resize(B * 64);
        std::vector<int> bad(B, 0);
        drh::parallel_for(B, [&](size_t i) {
            drh::Bytes& t = tr[i];
            uint8_t enc_i[drh::POINT_MAX], enc_o[drh::POINT_MAX];
            drh::enc_point(su, io_c ? io_c + 128 * i : inputs.data() + 64 * i, enc_i);
            drh::enc_point(su, io_c ? io_c + 128 * i + 64 : outs.data() + 64 * i, enc_o);
            drh::pedersen_transcript(su, su.point_len, enc_i, enc_o, drh::span_of(ads, ad_off, i), t);
            drh::Bytes tb = t;
            drh::put8(tb, 0x12);                                   // PEDERSEN_BLINDING
            uint64_t x[4], b[4];
            drh::load_le32(xs.data() + 32 * i, x);
            if (!drh::vrf_nonce(su, tb, x, b)) bad[i] = 1;
            drh::store_le32(b, blind.data() + 32 * i);
            std::memcpy(sc.data() + 64 * i, xs.data() + 32 * i, 32);
            std::memcpy(sc.data() + 64 * i + 32, blind.data() + 32 * i, 32);
        });
        for (size_t i = 0; i < B; i++) if (bad[i]) return fail(DR_ERR_INVALID, "nonce scalar is zero");
        tr_.mark("blinding");
        return DR_OK;
    }

    // out_proofs: 192 bytes per proof at `stride`; out_aux (nullable): O, Y_bar, R, O_k affine (4*64) + blinding (32) at aux_stride
    int tail(dr_ctx* actx, uint8_t* out_proofs, size_t stride, uint8_t* out_aux, size_t aux_stride) {
        // device copies of x, b, k, k_b (scalar uploads of the fixed-base and variable-base launches) do not outlive the call — on ANY exit path
        struct ScratchWipe {
            dr_ctx* c;
            bool armed = true;
            ~ScratchWipe() { if (armed) (void)ctx_wipe_scratch(c, true); }
        } scratch_wipe{actx};
        const drh::Mod256& mn = su.cv->n;
        const int cv = su.cv->id;
        ybar.resize(B * 64); ks.resize(B * 32); sc3.resize(B * 64); third.resize(2 * B * 64);
        // 4. blinded public keys  Y_bar_i = x_i*G + b_i*B: both bases are constants of the suite -> fixed-base window tables
        // (te_msm_groups, the variable-base launches, stays for callers with other bases)
        uint8_t gb[128];
        std::memcpy(gb, su.generator, 64);
        std::memcpy(gb + 64, su.blinding_base, 64);
        TRY(te_fixed_base_groups(actx, cv, gb, sc.data(), B, 2, ybar.data()));
        // 5. nonces
        const size_t pl = su.point_len;
        std::vector<uint8_t> ybar_store;
        const uint8_t* ybar_c = nullptr;
        TRY(suite_coords(actx, su, ybar.data(), B, 1, ybar_store, &ybar_c));
        std::vector<int> bad2(B, 0);
        drh::parallel_for(B, [&](size_t i) {
            uint8_t enc[drh::POINT_MAX];
            drh::enc_point(su, ybar_c + 64 * i, enc);
            drh::put(tr[i], enc, pl);
            uint64_t x[4], b[4], k[4], kb[4];
            drh::load_le32(xs.data() + 32 * i, x);
            drh::load_le32(blind.data() + 32 * i, b);
            if (!drh::vrf_nonce(su, tr[i], x, k) || !drh::vrf_nonce(su, tr[i], b, kb)) bad2[i] = 1;
            drh::store_le32(k, ks.data() + 32 * i);
            drh::store_le32(k, sc3.data() + 64 * i);                           // group i: k*G + kb*B
            drh::store_le32(kb, sc3.data() + 64 * i + 32);
        });
        for (size_t i = 0; i < B; i++) if (bad2[i]) return fail(DR_ERR_INVALID, "nonce scalar is zero");
        // R_i = k_i*G + kb_i*B from the tables; O_k,i = k_i * I_i is the one variable-base multiplication left
        TRY(te_fixed_base_groups(actx, cv, gb, sc3.data(), B, 2, third.data()));
        TRY(te_scalar_mul_batch(actx, cv, inputs.data(), ks.data(), B, third.data() + 64 * B));
        // 6. challenge, responses, the encoded proof (4 points, 2 scalars)
        std::vector<uint8_t> rk_store;
        const uint8_t* rk_c = nullptr;             // (R_i, O_k,i) pairs in the suite's coordinates
        if (su.cv->sw) {
            std::vector<uint8_t> rk(B * 128);
            for (size_t i = 0; i < B; i++) {
                std::memcpy(rk.data() + 128 * i, third.data() + 64 * i, 64);
                std::memcpy(rk.data() + 128 * i + 64, third.data() + 64 * (B + i), 64);
            }
            TRY(suite_coords(actx, su, rk.data(), 2 * B, 2, rk_store, &rk_c));
        }
        const uint8_t* outs_c = su.cv->sw ? outs_sw.data() : outs.data();
        // Curve25519: the identity has no encoding (the reference's point_to_string raises)
        if (drh::any_mont_identity(su, inputs.data(), B) || drh::any_mont_identity(su, outs.data(), B) || drh::any_mont_identity(su, ybar.data(), B) ||
            drh::any_mont_identity(su, third.data(), 2 * B))
            return fail(DR_ERR_INVALID, "cannot serialize the point at infinity");
        auto r_of = [&](size_t i) { return rk_c ? rk_c + 128 * i : third.data() + 64 * i; };
        auto ok_of = [&](size_t i) { return rk_c ? rk_c + 128 * i + 64 : third.data() + 64 * (B + i); };
        drh::parallel_for(B, [&](size_t i) {
            uint8_t* out = out_proofs + stride * i;
            drh::enc_point(su, outs_c + 64 * i, out);
            drh::enc_point(su, ybar_c + 64 * i, out + pl);
            drh::enc_point(su, r_of(i), out + 2 * pl);
            drh::enc_point(su, ok_of(i), out + 3 * pl);
            uint64_t c[4], x[4], b[4], k[4], kb[4], s[4], sb[4];
            drh::vrf_challenge(su, tr[i], out + 2 * pl, 2, c);
            drh::load_le32(xs.data() + 32 * i, x);
            drh::load_le32(blind.data() + 32 * i, b);
            drh::load_le32(ks.data() + 32 * i, k);
            drh::load_le32(sc3.data() + 64 * i + 32, kb);
            mn.mul(c, x, s);  mn.add(s, k, s);
            mn.mul(c, b, sb); mn.add(sb, kb, sb);
            drh::store_le32(s, out + 4 * pl);
            drh::store_le32(sb, out + 4 * pl + 32);
            if (out_aux) {                                   // (in the suite's coordinates)
                uint8_t* a = out_aux + aux_stride * i;
                std::memcpy(a, outs_c + 64 * i, 64);
                std::memcpy(a + 64, ybar_c + 64 * i, 64);
                std::memcpy(a + 128, r_of(i), 64);
                std::memcpy(a + 192, ok_of(i), 64);
                std::memcpy(a + rf::AUX_BLIND, blind.data() + 32 * i, 32);
            }
        });
        scratch_wipe.armed = false;                          // the success path reports the wipe's own status
        return ctx_wipe_scratch(actx, true);
    }
};

int ringvrf_prove_batch_impl(dr_ring_prover* p, const dr_vrf_suite* suite, size_t batch, const uint8_t* alphas, const uint64_t* alpha_off,
                                    const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts, const uint64_t* salt_off,
                                    const uint8_t* secret_scalars, const uint32_t* producer_index, const uint8_t* fs_prefix, size_t fs_prefix_len,
                                    const uint8_t* zk_random48, uint8_t* out_proofs, uint8_t* out_aux) {
    if (!p || !alpha_off || !ad_off || !secret_scalars || !producer_index || !fs_prefix || !out_proofs) return fail(DR_ERR_INVALID, "null argument");
    if (batch == 0) return DR_OK;
    if (batch > 4096) return fail(DR_ERR_INVALID, "batch must be at most 4096 per call");
    drh::VrfSuite su;
    TRY(load_suite(suite, su));
    if (su.cv->id != ring_prover_curve(p)) return fail(DR_ERR_INVALID, "VRF suite and ring prover are on different curves");
    TRY(offsets_ok(batch, {alpha_off, ad_off, salt_off}));
    dr_ctx* ctx = ring_prover_ctx(p);
    TRY(use_ctx(ctx));
    const size_t B = batch;
    PhaseTrace tr_("prove_batch");

    // hidden rows of the ring proof: 12 x 48 random bytes per proof reduced mod p — needs nothing from the GPU, so it runs on this
    // thread (and the pool) while the Elligator and x*I kernels of the Pedersen head are in flight
    std::vector<uint8_t> zk;
    const std::function<void()> reduce_zk = [&] {
        if (!zk_random48) return;
        zk.resize(B * 12 * 32);
        drh::parallel_for(B * 12, [&](size_t j) {
            uint64_t v[4];
            drh::mod_p().reduce_bytes(zk_random48 + 48 * j, 48, false, v);
            drh::store_le32(v, zk.data() + 32 * j);
        });
    };
    PedersenBatch ped(su, B);
    TRY(ped.head(ctx, alphas, alpha_off, ads, ad_off, salts, salt_off, secret_scalars, tr_, &reduce_zk));
    std::vector<uint8_t>& blind = ped.blind;
    // 4.-6. the rest of the Pedersen part needs nothing from the ring proof and the ring proof needs only the blinding
    // factors: it runs on a second stream (own context: scratch + stream) from a helper thread while this thread drives
    // the ring phases.  Its kernels are latency-bound (16..64 waves) and hide under the chip-filling MSMs.
    dr_ctx* actx = nullptr;
    TRY(ring_prover_aux_ctx(p, &actx));
    actx->prof = ctx->prof;
    int ped_rc = DR_OK;
    std::string ped_err;
    std::thread ped_thread([&] { run_guarded(ped_rc, ped_err, [&] { return ped.tail(actx, out_proofs, rf::PROOF_BYTES, out_aux, rf::AUX_BYTES); }); });
    struct WipeGuard {       // an exit before the last ring phase (which wipes on its own) still leaves no witness state in HBM
        dr_ring_prover* p;
        bool armed = true;
        ~WipeGuard() { if (armed) (void)dr_ring_prover_wipe(p); }
    } wipe_guard{p};
    ThreadJoiner joiner{ped_thread};          // every exit path below must wait for the helper before the buffers it uses go away

    // 7. ring proof: witness columns
    std::vector<uint8_t> relation(B * 64), wit(B * 4 * 96), cq(B * 96), evals(B * rf::EVAL_REC), opens(B * 192);
    std::vector<int> wit_inf(B * 4), cq_inf(B), open_inf(B * 2);
    tr_.mark("spawn+zk");
    TRY(dr_ring_prove_witness(p, B, producer_index, blind.data(), zk_random48 ? zk.data() : nullptr, relation.data(), wit.data(), wit_inf.data()));
    tr_.mark("witness");
    // transcripts in groups of four proofs (drh::RingFsGroup), one round of the schedule between two GPU phases
    drh::FsTranscript4 base;
    base.sh.update_same(fs_prefix, fs_prefix_len);
    const size_t G = drh::RingFsGroup::groups(B);
    std::vector<drh::RingFsGroup> fs;
    fs.reserve(G);
    for (size_t g = 0; g < G; g++) fs.emplace_back(base, g, B);
    std::vector<uint8_t> alphas7(B * rf::ALPHAS_BYTES), zetas(B * 32), nus(B * rf::NUS_BYTES);
    drh::parallel_for(G, [&](size_t g) {
        fs[g].round_alphas([&](size_t i) { return relation.data() + 64 * i; },
                           [&](size_t i, uint8_t* ser) {
                               for (int c = 0; c < 4; c++) drh::g1_serialized(wit.data() + 96 * (4 * i + c), wit_inf[4 * i + c], ser + 96 * c);
                           },
                           alphas7.data());
    }, 4);        // (an item is four proofs' sponges, 10 - 20 us: worth a thread from four items on)
    tr_.mark("fs1");
    TRY(dr_ring_prove_quotient(p, B, alphas7.data(), cq.data(), cq_inf.data()));
    tr_.mark("quotient");
    drh::parallel_for(G, [&](size_t g) {
        fs[g].round_zeta([&](size_t i, uint8_t* ser) { drh::g1_serialized(cq.data() + 96 * i, cq_inf[i], ser); }, zetas.data());
    }, 4);        // (an item is four proofs' sponges, 10 - 20 us: worth a thread from four items on)
    tr_.mark("fs2");
    TRY(dr_ring_prove_evals(p, B, zetas.data(), evals.data()));
    tr_.mark("evals");
    drh::parallel_for(G, [&](size_t g) {
        fs[g].round_nus([&](size_t i) { return evals.data() + rf::EVAL_REC * i; },
                        [&](size_t i) { return evals.data() + rf::EVAL_REC * i + rf::EVALS_BYTES; }, nus.data());
    }, 4);        // (an item is four proofs' sponges, 10 - 20 us: worth a thread from four items on)
    tr_.mark("fs3");
    TRY(dr_ring_prove_openings(p, B, nus.data(), opens.data(), open_inf.data()));
    wipe_guard.armed = false;        // (the openings phase ended with the wipe)
    tr_.mark("openings");
    // 8. payload: 4 compressed commitments, 7 evaluations, C_q, l(zeta*omega), 2 opening proofs  (proof_payload.py:68-117)
    std::vector<int> rc(B, DR_OK);
    drh::parallel_for(B, [&](size_t i) {
        uint8_t* out = out_proofs + rf::PROOF_BYTES * i;
        const uint8_t* ev = evals.data() + rf::EVAL_REC * i;
        int r = DR_OK;
        for (int c = 0; c < 4 && r == DR_OK; c++) r = dr_g1_compress(wit.data() + 96 * (4 * i + c), wit_inf[4 * i + c], out + rf::COMMITS + 48 * c);
        std::memcpy(out + rf::EVALS, ev, rf::EVALS_BYTES);
        if (r == DR_OK) r = dr_g1_compress(cq.data() + 96 * i, cq_inf[i], out + rf::CQ);
        std::memcpy(out + rf::L_ZW, ev + rf::EVALS_BYTES, 32);
        if (r == DR_OK) r = dr_g1_compress(opens.data() + 192 * i, open_inf[2 * i], out + rf::OPENS);
        if (r == DR_OK) r = dr_g1_compress(opens.data() + 192 * i + 96, open_inf[2 * i + 1], out + rf::OPENS + 48);
        rc[i] = r;
        if (out_aux) {
            uint8_t* a = out_aux + rf::AUX_BYTES * i;
            for (int c = 0; c < 4; c++) drh::g1_serialized(wit.data() + 96 * (4 * i + c), wit_inf[4 * i + c], a + rf::AUX_COMMITS + 96 * c);
            drh::g1_serialized(cq.data() + 96 * i, cq_inf[i], a + rf::AUX_CQ);
            drh::g1_serialized(opens.data() + 192 * i, open_inf[2 * i], a + rf::AUX_OPENS);
            drh::g1_serialized(opens.data() + 192 * i + 96, open_inf[2 * i + 1], a + rf::AUX_OPENS + 96);
        }
    });
    for (size_t i = 0; i < B; i++) if (rc[i] != DR_OK) return rc[i];
    tr_.mark("payload");
    if (ped_thread.joinable()) ped_thread.join();
    tr_.mark("join");
    if (ped_rc != DR_OK) return fail(ped_rc, ped_err.empty() ? "Pedersen part failed" : ped_err);
    return DR_OK;
}

// C++ exceptions (allocation failures of the host-side staging vectors, thread creation) must not cross the C ABI: abi_guard
int dr_ringvrf_prove_batch(dr_ring_prover* p, const dr_vrf_suite* suite, size_t batch, const uint8_t* alphas, const uint64_t* alpha_off,
                           const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts, const uint64_t* salt_off,
                           const uint8_t* secret_scalars, const uint32_t* producer_index, const uint8_t* fs_prefix, size_t fs_prefix_len,
                           const uint8_t* zk_random48, uint8_t* out_proofs, uint8_t* out_aux) {
    return abi_guard("native prover", [&] {
        return ringvrf_prove_batch_impl(p, suite, batch, alphas, alpha_off, ads, ad_off, salts, salt_off, secret_scalars, producer_index, fs_prefix,
                                        fs_prefix_len, zk_random48, out_proofs, out_aux);
    });
}

int dr_ringvrf_aux_take_blindings(uint8_t* aux, size_t batch, uint8_t* out_blind) {
    if (batch && (!aux || !out_blind)) return fail(DR_ERR_INVALID, "null buffer");
    for (size_t i = 0; i < batch; i++) {
        uint8_t* b = aux + rf::AUX_BYTES * i + rf::AUX_BLIND;
        std::memcpy(out_blind + 32 * i, b, 32);
        explicit_bzero(b, 32);
    }
    return DR_OK;
}

// Pedersen VRF batch verification core (pedersen/vrf.py:171-242) on decoded points: challenges, weights from one
// transcript over all (c, s, s_b), then ONE (5B+2)-point MSM that must be the identity.  proofs: 192 bytes per proof at
// `stride`; te_xy: the four decoded points of each proof (O, Y_bar, R, O_k affine); in_pts: encode_to_curve of the inputs.
int pedersen_verify_core(dr_ctx* actx, const drh::VrfSuite& su, size_t B, const uint8_t* proofs, size_t stride,
                                const std::vector<uint8_t>& te_xy, const std::vector<uint8_t>& in_pts, const uint8_t* ads,
                                const uint64_t* ad_off, int& ped_ok, const uint8_t* excluded = nullptr, uint8_t* each_ok = nullptr) {
    const drh::Mod256& mn = su.cv->n;
    const size_t pl = su.point_len;
    std::vector<uint8_t> in_store;
    const uint8_t* in_c = nullptr;
    TRY(suite_coords(actx, su, in_pts.data(), B, 1, in_store, &in_c));
    std::vector<uint8_t> cs(B * 32);
    drh::parallel_for(B, [&](size_t i) {
        if (excluded && excluded[i]) return;
        const uint8_t* pr = proofs + stride * i;
        uint8_t enc[drh::POINT_MAX];
        drh::enc_point(su, in_c + 64 * i, enc);
        drh::Bytes t;
        drh::pedersen_transcript(su, pl, enc, pr, drh::span_of(ads, ad_off, i), t);     // (the output point as encoded in the proof)
        drh::put(t, pr + pl, pl);                              // blinded public key
        uint64_t c[4];
        drh::vrf_challenge(su, t, pr + 2 * pl, 2, c);          // R, O_k
        drh::store_le32(c, cs.data() + 32 * i);
    });
    if (each_ok) {
        // a verdict per proof: the two equations of each proof as they stand, O_k = s*I - c*O and R = s*G + s_b*B - c*Y_bar — 2B groups of
        // three terms in ONE launch of the group kernel, compared on the host (an excluded proof rides along as 0 * G and is not compared)
        std::vector<uint8_t> pts(6 * B * 64), sc(6 * B * 32, 0), sums(2 * B * 64);
        drh::parallel_for(B, [&](size_t i) {
            uint8_t* p = pts.data() + 384 * i;
            if (excluded && excluded[i]) { for (int k = 0; k < 6; k++) std::memcpy(p + 64 * k, su.generator, 64); return; }
            const uint8_t* pr = proofs + stride * i;
            uint64_t c[4];
            drh::load_le32(cs.data() + 32 * i, c);
            mn.neg(c, c);
            uint8_t* k = sc.data() + 192 * i;
            std::memcpy(p, in_pts.data() + 64 * i, 64);                  std::memcpy(k, pr + 4 * pl, 32);            // s * I
            std::memcpy(p + 64, te_xy.data() + 64 * (4 * i), 64);        drh::store_le32(c, k + 32);                 // - c * O
            std::memcpy(p + 128, su.generator, 64);                                                                  // (0 * G: groups are of one size)
            std::memcpy(p + 192, su.generator, 64);                      std::memcpy(k + 96, pr + 4 * pl, 32);       // s * G
            std::memcpy(p + 256, su.blinding_base, 64);                  std::memcpy(k + 128, pr + 4 * pl + 32, 32); // s_b * B
            std::memcpy(p + 320, te_xy.data() + 64 * (4 * i + 1), 64);   drh::store_le32(c, k + 160);                // - c * Y_bar
        });
        TRY(te_msm_groups(actx, su.cv->id, pts.data(), sc.data(), 2 * B, 3, sums.data()));
        for (size_t i = 0; i < B; i++)
            each_ok[i] = !(excluded && excluded[i]) && std::memcmp(sums.data() + 128 * i, te_xy.data() + 64 * (4 * i + 3), 64) == 0 &&
                         std::memcmp(sums.data() + 128 * i + 64, te_xy.data() + 64 * (4 * i + 2), 64) == 0;
        return DR_OK;
    }
    {
        drh::Bytes absorbed = su.suite_id;
        drh::put8(absorbed, 0x50);                             // BATCH_VERIFY
        for (size_t i = 0; i < B; i++) {
            drh::put(absorbed, cs.data() + 32 * i, 32);
            drh::put(absorbed, proofs + stride * i + 4 * pl, 64);   // s, s_b
        }
        std::vector<uint8_t> weights(32 * B);
        drh::vrf_squeeze(su.xof, absorbed.data(), absorbed.size(), weights.data(), weights.size());
        std::vector<uint8_t> pts((5 * B + 2) * 64), sc((5 * B + 2) * 32);
        std::vector<uint64_t> gen_part(B * 4), blind_part(B * 4);
        drh::parallel_for(B, [&](size_t i) {
            const uint8_t* pr = proofs + stride * i;
            uint64_t w_io[4], w_cm[4], c[4], s[4], sb[4], t[4];
            mn.reduce_bytes(weights.data() + 32 * i, 16, false, w_io);
            mn.reduce_bytes(weights.data() + 32 * i + 16, 16, false, w_cm);
            drh::load_le32(cs.data() + 32 * i, c);
            drh::load_le32(pr + 4 * pl, s);
            drh::load_le32(pr + 4 * pl + 32, sb);
            uint8_t* p = pts.data() + 320 * i;
            uint8_t* k = sc.data() + 160 * i;
            std::memcpy(p, te_xy.data() + 64 * (4 * i + 3), 64);       drh::store_le32(w_io, k);                       // O_k
            std::memcpy(p + 64, te_xy.data() + 64 * (4 * i), 64);      mn.mul(w_io, c, t); drh::store_le32(t, k + 32);  // output
            std::memcpy(p + 128, in_pts.data() + 64 * i, 64);          mn.mul(w_io, s, t); mn.neg(t, t); drh::store_le32(t, k + 64);   // input
            std::memcpy(p + 192, te_xy.data() + 64 * (4 * i + 2), 64); drh::store_le32(w_cm, k + 96);                  // R
            std::memcpy(p + 256, te_xy.data() + 64 * (4 * i + 1), 64); mn.mul(w_cm, c, t); drh::store_le32(t, k + 128); // Y_bar
            mn.mul(w_cm, s, &gen_part[4 * i]);
            mn.mul(w_cm, sb, &blind_part[4 * i]);
        });
        uint64_t gs[4] = {0, 0, 0, 0}, bs[4] = {0, 0, 0, 0};
        for (size_t i = 0; i < B; i++) { mn.sub(gs, &gen_part[4 * i], gs); mn.sub(bs, &blind_part[4 * i], bs); }
        std::memcpy(pts.data() + 320 * B, su.generator, 64);           drh::store_le32(gs, sc.data() + 160 * B);
        std::memcpy(pts.data() + 320 * B + 64, su.blinding_base, 64);  drh::store_le32(bs, sc.data() + 160 * B + 32);
        uint8_t sum[64];
        TRY(te_msm(actx, su.cv->id, pts.data(), sc.data(), 5 * B + 2, sum));
        uint8_t ident[64];
        std::memset(ident, su.identity_fill, 64);
        if (!su.identity_fill) ident[32] = su.identity_y;   // (0, 1) on the twisted Edwards curves; 64 zero bytes on P-256 and secp256k1; 0xff bytes on Curve25519
        ped_ok = std::memcmp(sum, ident, 64) == 0 ? 1 : 0;
    }
    return DR_OK;
}

// a host fold's result as dr_pairing_check takes it: affine big-endian x || y (zeros and *is_inf for the point at infinity); `negate`: -P
static void g1_pair_operand(const drh::G1& pt, bool negate, uint8_t out[96], int* is_inf) {
    drh::Fq ax, ay;
    if (!drh::g1_to_affine(pt, ax, ay)) { std::memset(out, 0, 96); *is_inf = 1; return; }
    ax.store_be(out);
    (negate ? ay.neg() : ay).store_be(out + 48);
    *is_inf = 0;
}

// Up to eight proofs: every launch chain of the verifier's decoding and folds would be pure latency (0.7 - 2 ms each), so the points are
// decoded and the two G1 folds done on the host (hostsmall.hpp: ~80 us per point on the worker pool, ~0.4 ms per fold); the Pedersen side
// keeps its stream.  Measured at the end of round 4: 1.2 ms for one proof + 0.13 - 0.2 ms per further one (the host's load decides)
// against a flat 2.9 ms through the kernels.
static size_t verify_host_max() {
    static const size_t host_max = std::getenv("DOTRING_VERIFY_HOST_MAX") ? (size_t)std::atol(std::getenv("DOTRING_VERIFY_HOST_MAX")) : 8;
    return host_max;
}

// RingVRF.batch_verify over encoded proofs (vrf/ring/vrf.py:239-283, pedersen/vrf.py:171-242, ring_proof/verify.py:51-324,
// pcs/kzg.py:304-338): decode + validate every point, replay the transcripts on worker threads, fold all claims into one
// Bandersnatch MSM (5B+2 points, must be the identity) and two G1 MSMs + one pairing equation.  One call = one object; run() is the
// timeline, the phases are the methods below it in the order they run.  A phase that finds the batch malformed (a non-canonical
// scalar, a point that does not decode, a zeta inside the domain) sets `rejected`: the verdict is then 0 with DR_OK.
// run_each() (dr_ringvrf_verify_each, `each` set) goes through the same phases for a verdict PER PROOF: there such a phase marks the
// proof in `excluded` instead — verdict 0, its scalars zero, its undecodable points the identity — and the others are judged as if
// it were absent; the two G1 MSMs give way to the per-proof claim points and their sum tree, the pairing to the descent over it.
// The members are declared in the order the phases create them and each helper thread's joiner behind everything its thread
// touches, so that on ANY exit path a thread is joined before what it works on goes away.
struct RingVerifyBatch {
    dr_ctx* const ctx;
    const drh::VrfSuite& su;
    const dr_ring_verifier_key* const vk;
    const size_t B;
    const uint8_t *const proofs, *const inputs, *const ads, *const salts, *const seed32;
    const uint64_t *const in_off, *const ad_off, *const salt_off;
    const drh::Mod256& mp = drh::mod_p();
    const hipStream_t st;
    const size_t n_te, n_g1;                         // Bandersnatch points of the proofs; G1 points of both folds
    const bool small;
    bool rejected = false;
    // dr_ringvrf_verify_each: a malformed proof is excluded (verdict 0, scalars zero, undecodable points the identity) instead of
    // rejecting the call; ring and Pedersen verdicts per proof
    uint8_t* const verdicts;
    uint32_t* const stats;
    const bool each;
    std::vector<uint8_t> excluded, ped_each, ring_each, nodes_le;
    PhaseTrace tr_{verdicts ? "verify_each" : "verify_batch"};
    // gather
    std::vector<uint8_t> te_enc, g1_enc;
    // verifier randomness: two non-zero coefficients per proof (kzg.py:84-108) — they depend on the seed alone, and they are the only scalars of
    // the rhs fold (r1, r2 on the two opening proofs): drawn in the gather, so that that fold can start as soon as the points are decoded
    std::vector<uint8_t> rhs_sc;
    // the Pedersen side: helper thread on the second stream, held at a gate
    dr_ctx* actx = nullptr;
    std::vector<uint8_t> in_pts, te_xy;
    int side_rc = DR_OK, ped_ok = 0;
    std::string side_err;
    std::mutex gate_m;
    std::condition_variable gate_cv;
    int gate = -1;                                   // -1 closed, 0 give up, 1 go on
    std::thread side;
    ThreadJoiner side_joiner{side, [this] { open_gate(0); }};
    // decoded G1 points: the context's resident device buffer (kernel route) or the host route's bases, and their standard-form copy
    Scratch& g1_bases;
    std::vector<uint8_t> g1_le;
    std::vector<drh::G1AffineHost> host_bases;
    // the rhs fold and its Miller loop: helper thread on the third stream
    std::vector<uint8_t> rhs_full;
    uint8_t pair_g1[2 * 96];
    int pair_inf[2] = {0, 0};
    drh::Fq12 f_rhs = drh::Fq12::one();
    int rhs_rc = DR_OK;
    std::string rhs_err;
    std::thread rhs_thread;
    ThreadJoiner rhs_joiner{rhs_thread};             // (declared after everything the thread touches: joined before any of it goes away)
    // challenges of every proof (replay) and the lhs fold's scalars (claim scalars)
    std::vector<uint8_t> al_all, zeta_all, nus_all, lhs_sc;
    std::vector<uint64_t> fixed_part;                   // per proof: r1*nu0, r1*nu1, r1*nu2, r1*agg + r2*l_zw

    RingVerifyBatch(dr_ctx* c, const drh::VrfSuite& s, const dr_ring_verifier_key* k, size_t batch, const uint8_t* pr, const uint8_t* in,
                    const uint64_t* ino, const uint8_t* ad, const uint64_t* ado, const uint8_t* sa, const uint64_t* sao, const uint8_t* seed, uint8_t* verdicts_out = nullptr,
                    uint32_t* stats_out = nullptr)
        : ctx(c), su(s), vk(k), B(batch), proofs(pr), inputs(in), ads(ad), salts(sa), seed32(seed), in_off(ino), ad_off(ado), salt_off(sao),
          st(c->stream), n_te(4 * batch), n_g1(rf::G_PER_PROOF * batch + rf::G_FIXED), small(batch <= verify_host_max()), verdicts(verdicts_out),
          stats(stats_out), each(verdicts_out != nullptr), excluded(each ? batch : 0, 0), g1_bases(c->vfy_bases) {}

    int run(int* ok) {
        gather();
        if (rejected) return DR_OK;
        tr_.mark("gather");
        TRY(start_pedersen_side());
        TRY(small ? decode_host() : decode_kernels());
        if (rejected) return DR_OK;
        tr_.mark("decode");
        TRY(start_rhs_fold());
        // (the Pedersen helper may go on only once the two host passes below have their slices of the worker pool: its challenge hashing
        //  queued first would be drained first — the pool serves the oldest job — and the critical path would wait behind it)
        replay();
        tr_.mark("replay");
        claim_scalars();
        open_gate(1);                // Pedersen part: te_xy has been complete since the decode; its hashing and MSM run beside the G1 folds and the pairing
        if (rejected) return DR_OK;
        tr_.mark("transcripts");
        TRY(lhs_fold());
        tr_.mark("g1 msms");
        int pok = 0;
        TRY(pairing(pok));
        tr_.mark("pairing");
        TRY(join());
        *ok = pok && ped_ok;
        return DR_OK;
    }

    void open_gate(int v) {
        { std::lock_guard<std::mutex> lk(gate_m); if (gate < 0) gate = v; }
        gate_cv.notify_all();
    }

    // ---- 1. canonical scalars; gather encoded points; the verifier randomness
    void gather() {
        const drh::Mod256& mn = su.cv->n;
        te_enc.resize(B * rf::PED_POINTS_BYTES); g1_enc.resize(B * rf::G_PER_PROOF * 48);
        rhs_sc.resize(2 * B * 32);
        std::atomic<bool> canonical{true};
        drh::parallel_for(B, [&](size_t i) {
            const uint8_t* pr = proofs + rf::PROOF_BYTES * i;
            for (int k = 0; k < 2; k++) {
                uint64_t r[4];
                drh::ring_verifier_randomness(seed32, i, k, r);
                drh::store_le32(r, rhs_sc.data() + 64 * i + 32 * k);
            }
            std::memcpy(te_enc.data() + rf::PED_POINTS_BYTES * i, pr + rf::PED_POINTS, rf::PED_POINTS_BYTES);
            uint64_t v[4];
            bool ok_i = true;
            for (int k = 0; k < 2; k++) { drh::load_le32(pr + rf::PED_SCALARS + 32 * k, v); if (drh::Mod256::geq(v, mn.m)) ok_i = false; }      // dec_scalar
            for (int k = 0; k < 7; k++) { drh::load_le32(pr + rf::EVALS + 32 * k, v); if (drh::Mod256::geq(v, mp.m)) ok_i = false; }
            drh::load_le32(pr + rf::L_ZW, v); if (drh::Mod256::geq(v, mp.m)) ok_i = false;
            if (!ok_i) { if (each) excluded[i] = 1; else canonical.store(false, std::memory_order_relaxed); }
            uint8_t* g = g1_enc.data() + rf::G_PER_PROOF * 48 * i;
            std::memcpy(g + 48 * rf::G_COMMITS, pr + rf::COMMITS, rf::COMMITS_BYTES);      // C_b, C_accip, C_accx, C_accy
            std::memcpy(g + 48 * rf::G_CQ, pr + rf::CQ, 48);                               // C_q
            std::memcpy(g + 48 * rf::G_OPENS, pr + rf::OPENS, rf::OPENS_BYTES);            // Phi_zeta, Phi_zeta_omega
        });
        if (!canonical.load()) rejected = true;
    }

    // ---- 2. decode + validate the 4B Bandersnatch points, decompress the 7B G1 points (on the host or through the kernels); meanwhile
    // a helper thread hashes the inputs to the curve on a second stream (all three kernels are latency-bound: a few dozen waves).
    // One helper thread for the whole Pedersen side (second stream): hash the inputs to the curve right away, then wait at a
    // gate until this thread has decoded and validated the proof points, then the challenges and the (5B+2)-point MSM.  The main
    // thread never waits for the Elligator kernels (they took the decode phase from 2.2 to 3.1 ms when it joined them there).
    int start_pedersen_side() {
        if (!ctx->aux) TRY(ctx_create_role(ctx->device, 1, &ctx->aux));
        actx = ctx->aux;
        actx->prof = ctx->prof;
        in_pts.resize(B * 64); te_xy.resize(n_te * 64);
        side = std::thread([this] {
            run_guarded(side_rc, side_err, [&]() -> int {
                TRY(encode_to_curve_msgs(actx, su, B, inputs, in_off, salts, salt_off, in_pts.data()));
                {
                    std::unique_lock<std::mutex> lk(gate_m);
                    gate_cv.wait(lk, [&] { return gate >= 0; });
                    if (gate == 0) return DR_OK;
                }
                if (each) ped_each.assign(B, 0);
                return pedersen_verify_core(actx, su, B, proofs, rf::PROOF_BYTES, te_xy, in_pts, ads, ad_off, ped_ok, each ? excluded.data() : nullptr,
                                            each ? ped_each.data() : nullptr);
            });
        });
        return DR_OK;
    }

    // small batches (verify_host_max): every point decoded on the worker pool, the G1 bases kept for the host folds
    int decode_host() {
        const size_t n_dec = rf::G_PER_PROOF * B;
        g1_le.resize(n_dec * 96);
        std::vector<int> good(n_te + n_dec, 0);
        auto decode_one = [&](size_t j) {
            if (j < n_te) {
                good[j] = drh::te_decode_checked(*su.cv, te_enc.data() + 32 * j, te_xy.data() + 64 * j) ? 1 : 0;
                return;
            }
            const size_t k = j - n_te;
            uint8_t be[96];
            int inf = 0;
            if (dr_g1_decompress(g1_enc.data() + 48 * k, be, &inf) != DR_OK) return;
            uint8_t* le = g1_le.data() + 96 * k;
            if (inf) std::memset(le, 0, 96);
            else for (int q = 0; q < 48; q++) { le[q] = be[47 - q]; le[48 + q] = be[95 - q]; }
            good[j] = 1;
        };
        // 4B + 7B decodings of 35 - 80 us each, one per item of the worker pool (its threads are already there: starting seven of our
        // own cost more than a decoding)
        drh::parallel_for(n_te + n_dec, decode_one, 1);
        for (size_t j = 0; j < good.size(); j++)
            if (!good[j]) {                                                  // malformed / invalid point: ok = 0
                if (!each) { rejected = true; return DR_OK; }
                excluded[j < n_te ? j / 4 : (j - n_te) / rf::G_PER_PROOF] = 1;      // (an undecoded G1 record stays zero: the identity)
            }
        host_bases.resize(n_g1);
        for (size_t k = 0; k < n_dec; k++) {
            const uint8_t* le = g1_le.data() + 96 * k;
            bool inf = true;
            for (int q = 0; q < 96; q++) if (le[q]) { inf = false; break; }
            host_bases[k].inf = inf;
            if (!inf && (!drh::Fq::load_le(host_bases[k].x, le) || !drh::Fq::load_le(host_bases[k].y, le + 48))) {
                if (!each) { rejected = true; return DR_OK; }
                excluded[k / rf::G_PER_PROOF] = 1;
                host_bases[k].inf = true;
            }
        }
        for (size_t k = 0; k < rf::G_FIXED; k++) {
            const uint8_t* be = k < 3 ? vk->fixed_commitments + 96 * k : vk->g1_generator;
            drh::G1AffineHost& hb = host_bases[n_dec + k];
            hb.inf = (be[0] & 0x40) != 0;
            if (!hb.inf) {
                if (be[0] & 0xe0) return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
                if (!drh::Fq::load_be(hb.x, be) || !drh::Fq::load_be(hb.y, be + 48) || !drh::g1_on_curve(hb.x, hb.y))
                    return fail(DR_ERR_INVALID, "invalid BLS12-381 G1 encoding");
            }
        }
        return DR_OK;
    }

    // larger batches: both decoders as kernels, side by side on two streams
    int decode_kernels() {
        const size_t n_dec = rf::G_PER_PROOF * B;
        g1_le.resize(n_dec * 96);
        Scratch &te_in = ctx->vfy_te_in, &te_out = ctx->vfy_te_out, &vflags = ctx->vfy_flags, &g1_in = ctx->vfy_in, &g1_std = ctx->vfy_std;
        TRY(te_in.reserve(n_te * 32));
        TRY(te_out.reserve(n_te * 64));
        TRY(vflags.reserve(n_te * 4 + n_g1 * 4));
        // the third stream (G1 decompression, below) writes its verdicts behind this stream's: it starts when this stream is done with
        // whatever an earlier call left in it, but not behind the decoding kernel launched next
        hipEvent_t scratch_ready;
        HIP_TRY(hipEventCreateWithFlags(&scratch_ready, hipEventDisableTiming));
        struct EventGuard { hipEvent_t e; ~EventGuard() { (void)hipEventDestroy(e); } } scratch_ready_guard{scratch_ready};
        HIP_TRY(hipEventRecord(scratch_ready, st));
        HIP_TRY(hipMemcpyAsync(te_in.p, te_enc.data(), n_te * 32, hipMemcpyHostToDevice, st));
        uint32_t* d_ok = vflags.as<uint32_t>();
        TRY(launch(ctx, "k_bsn_decode_points", [&] {
            launch_decode_points(ctx, st, su.cv->id, false, te_in.as<uint32_t>(), te_out.as<uint32_t>(), d_ok, n_te);
        }));
        std::vector<uint32_t> flags(n_te + n_g1);
        // G1: bases buffer = 7B decompressed points followed by C_px, C_py, C_s and G1[0]
        TRY(g1_bases.reserve(n_g1 * 96));
        TRY(g1_in.reserve(n_dec * 48));
        TRY(g1_std.reserve(n_g1 * 96));
        // the G1 decompression (a 380-squaring chain on ~100 waves) runs next to the Bandersnatch decoding (~1 ms on 128 waves) on
        // the third stream; an event brings it back into this stream before anything reads the bases
        if (!ctx->aux2) TRY(ctx_create_role(ctx->device, 2, &ctx->aux2));
        dr_ctx* dctx = ctx->aux2;
        hipStream_t st2 = dctx->stream;
        ctx->aux2->prof = ctx->prof;
        if (st2 != st) HIP_TRY(hipStreamWaitEvent(st2, scratch_ready, 0));
        HIP_TRY(hipMemcpyAsync(g1_in.p, g1_enc.data(), n_dec * 48, hipMemcpyHostToDevice, st2));
        TRY(launch(dctx, "k_g1_decompress", [&] {
            g1_launch_decompress(st2, g1_in.as<uint8_t>(), g1_bases.as<uint32_t>(), d_ok + n_te, n_dec);
        }));
        // only now the copy back of the decoded Bandersnatch points: into pageable memory it blocks this thread until the decoding
        // kernel is done, and issued before the G1 launch (as it was until round 3) it kept the two decoders from running side by
        // side — 1.06 + 0.96 ms in a row instead of 1.06
        HIP_TRY(hipMemcpyAsync(te_xy.data(), te_out.p, n_te * 64, hipMemcpyDeviceToHost, st));
        {
            hipEvent_t done;
            HIP_TRY(hipEventCreateWithFlags(&done, hipEventDisableTiming));
            hipError_t e1 = hipEventRecord(done, st2), e2 = e1 == hipSuccess ? hipStreamWaitEvent(st, done, 0) : e1;
            (void)hipEventDestroy(done);
            HIP_TRY(e2);
        }
        {
            uint8_t tail_be[4 * 96];
            std::memcpy(tail_be, vk->fixed_commitments, 3 * 96);
            std::memcpy(tail_be + 288, vk->g1_generator, 96);
            for (int k = 0; k < 3; k++) if (tail_be[96 * k] & 0x40) std::memset(tail_be + 96 * k, 0, 96);       // serialised infinity
            std::vector<uint8_t> le;
            TRY(g1_be_to_le_limbs(tail_be, 4, le, true));
            HIP_TRY(hipMemcpyAsync(g1_bases.as<uint32_t>() + n_dec * 24, le.data(), 4 * 96, hipMemcpyHostToDevice, st));
            HIP_TRY(hipStreamSynchronize(st));          // `le` is a stack-lifetime staging buffer
            tr_.mark("decode kernels");
            g1_launch_bases_to_mont(st, g1_bases.as<uint32_t>() + n_dec * 24, 4);
        }
        g1_launch_bases_from_mont(st, g1_bases.as<uint32_t>(), g1_std.as<uint32_t>(), n_dec);
        HIP_TRY(hipMemcpyAsync(g1_le.data(), g1_std.p, n_dec * 96, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(flags.data(), d_ok, (n_te + n_dec) * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        for (size_t i = 0; i < n_te + n_dec; i++)
            if (!flags[i]) {                                                 // malformed / invalid point: ok = 0
                if (!each) { rejected = true; return DR_OK; }
                excluded[i < n_te ? i / 4 : (i - n_te) / rf::G_PER_PROOF] = 1;      // (k_g1_decompress wrote the identity in its place)
            }
        return DR_OK;
    }

    // ---- 3a. the rhs fold — r1, r2 on the two opening proofs of every proof, zero scalars (no digits, no cost) on everything else — needs
    // nothing from the transcripts: it starts now, on the third stream from a helper thread, and runs under the two host passes that follow;
    // the thread then takes the Miller loop of its pair (-rhs, G2[1]) as well, so that after the lhs fold only one loop, one product in
    // Fq12 and the final exponentiation are left (the two loops' product is what the joint loop of dr_pairing_check computes).
    int start_rhs_fold() {
        rhs_full.assign(n_g1 * 32, 0);
        for (size_t i = 0; i < B; i++) std::memcpy(rhs_full.data() + 32 * (rf::G_PER_PROOF * i + rf::G_OPENS), rhs_sc.data() + 64 * i, 64);
        if (small) {
            // one or two proofs: the same on the host (hostsmall.hpp: ~0.3 ms for the 2B live terms)
            rhs_thread = std::thread([this] {
                run_guarded(rhs_rc, rhs_err, [&]() -> int {
                    const drh::G1 rhs_pt = drh::g1_msm_small(host_bases.data(), rhs_full.data(), n_g1, 1);
                    g1_pair_operand(rhs_pt, true, pair_g1 + 96, pair_inf + 1);
                    return pairing_miller(pair_g1 + 96, vk->g2 + 192, 1, f_rhs);
                });
            });
            return DR_OK;
        }
        if (!ctx->aux2) TRY(ctx_create_role(ctx->device, 2, &ctx->aux2));
        dr_ctx* bctx = ctx->aux2;
        bctx->prof = ctx->prof;
        rhs_thread = std::thread([this, bctx] {
            run_guarded(rhs_rc, rhs_err, [&]() -> int {
                TRY(use_ctx(bctx));
                TRY(bctx->scalars.reserve(n_g1 * 32));
                HIP_TRY(hipMemcpyAsync(bctx->scalars.p, rhs_full.data(), n_g1 * 32, hipMemcpyHostToDevice, bctx->stream));
                TRY(msm_to_bytes(bctx, g1_bases.as<uint32_t>(), bctx->scalars.as<uint32_t>(), n_g1, 1, pair_g1 + 96, pair_inf + 1));
                // (a vanishing rhs can only come from r1 = r2 = 0 or infinity openings: its pair then contributes 1 and the equation demands lhs = O)
                if (!pair_inf[1]) {                                              // e(lhs, G2[0]) * e(-rhs, G2[1]) == 1
                    drh::Fq y;
                    if (!drh::Fq::load_be(y, pair_g1 + 144)) return fail(DR_ERR_DEVICE, "MSM result out of range");
                    y.neg().store_be(pair_g1 + 144);
                }
                return pairing_miller(pair_g1 + 96, vk->g2 + 192, 1, f_rhs);
            });
        });
        return DR_OK;
    }

    // ---- 4. ring proofs: transcript replay, four proofs per sponge group (drh::RingFsGroup: all three rounds of the schedule)
    void replay() {
        drh::FsTranscript4 base;
        base.sh.update_same(vk->fs_prefix, vk->fs_prefix_len);
        auto be_rec = [&](size_t idx, uint8_t out[96]) {     // device LE limbs -> serialize() form
            const uint8_t* s = g1_le.data() + 96 * idx;
            bool inf = true;
            for (int j = 0; j < 96; j++) if (s[j]) { inf = false; break; }
            if (inf) { std::memset(out, 0, 96); out[0] = 0x40; return; }
            for (int j = 0; j < 48; j++) { out[j] = s[47 - j]; out[48 + j] = s[95 - j]; }
        };
        al_all.resize(B * rf::ALPHAS_BYTES); zeta_all.resize(B * 32); nus_all.resize(B * rf::NUS_BYTES);
        drh::parallel_for(drh::RingFsGroup::groups(B), [&](size_t g) {
            drh::RingFsGroup t(base, g, B);
            t.round_alphas([&](size_t i) { return te_xy.data() + 64 * (4 * i + 1); },                    // blinded public key
                           [&](size_t i, uint8_t* ser) {
                               for (size_t c = 0; c < 4; c++) be_rec(rf::G_PER_PROOF * i + rf::G_COMMITS + c, ser + 96 * c);
                           },
                           al_all.data());
            t.round_zeta([&](size_t i, uint8_t* ser) { be_rec(rf::G_PER_PROOF * i + rf::G_CQ, ser); }, zeta_all.data());
            t.round_nus([&](size_t i) { return proofs + rf::PROOF_BYTES * i + rf::EVALS; },
                        [&](size_t i) { return proofs + rf::PROOF_BYTES * i + rf::L_ZW; }, nus_all.data());
        }, 4);        // (an item is four proofs' sponges, 10 - 20 us: worth a thread from four items on)
    }

    // ---- the verifier scalar pass per proof and the random linear combination of all claims: the lhs fold's scalars
    void claim_scalars() {
        drh::RingVerifierDomain dm;
        dm.init(vk->log2n, vk->omega_n, vk->seed_xy);
        lhs_sc.resize(n_g1 * 32);
        fixed_part.resize(B * 16);
        std::vector<int> bad(B, 0);
        // Every proof needs two field inversions (seed + relation in affine form; the Lagrange / vanishing denominators at zeta) — at 7 us
        // each they were two thirds of this pass.  Sixteen proofs share ONE (Montgomery's trick, drh::batch_inv): both halves of the
        // arithmetic are split around their inversion.
        constexpr size_t VS = 16;
        drh::parallel_for((B + VS - 1) / VS, [&](size_t slice) {
            const size_t lo = slice * VS, hi = std::min(B, lo + VS);
            drh::TeAddPending ta[VS];
            drh::RingTermsPending rt[VS];
            uint64_t den[2 * VS][4];
            for (size_t i = lo; i < hi; i++) {
                const size_t k = i - lo;
                if (each && excluded[i]) { bad[i] = 1; std::memset(den[2 * k], 0, 64); continue; }
                drh::te_add_affine_prep(*su.cv, vk->seed_xy, te_xy.data() + 64 * (4 * i + 1), ta[k]);
                std::memcpy(den[2 * k], ta[k].den, 32);
                if (drh::ring_verifier_terms_prep(dm, zeta_all.data() + 32 * i, rt[k])) std::memcpy(den[2 * k + 1], rt[k].prod, 32);
                else { bad[i] = 1; std::memset(den[2 * k + 1], 0, 32); }
            }
            drh::batch_inv(mp, den, 2 * (hi - lo));
            for (size_t i = lo; i < hi; i++) {
                if (bad[i]) continue;
                const size_t k = i - lo;
                const uint8_t* pr = proofs + rf::PROOF_BYTES * i;
                uint8_t result_seed[64];
                drh::te_add_affine_finish(ta[k], den[2 * k], result_seed);          // seed + blinded public key
                drh::RingClaimScalars cl;
                drh::ring_verifier_terms_finish(*su.cv, dm, al_all.data() + rf::ALPHAS_BYTES * i, nus_all.data() + rf::NUS_BYTES * i,
                                                zeta_all.data() + 32 * i, pr + rf::EVALS, pr + rf::L_ZW, result_seed, rt[k], den[2 * k + 1], cl);
                uint64_t r[2][4];                                                    // this proof's verifier randomness (drawn in the gather)
                for (int j = 0; j < 2; j++) drh::load_le32(rhs_sc.data() + 64 * i + 32 * j, r[j]);
                drh::ring_claim_fold(cl, r[0], r[1], lhs_sc.data() + 32 * rf::G_PER_PROOF * i, &fixed_part[16 * i]);
            }
        }, 1);
        for (size_t i = 0; i < B; i++)
            if (bad[i]) { if (each) excluded[i] = 1; else rejected = true; }
    }

    // two MSMs over the decompressed bases (already resident): lhs over all 7B+4 points here, rhs (started above) over the 2B opening
    // proofs.  Two single MSMs rather than a batch of two: the final 255-doubling window combination of a single MSM runs on the host
    // (0.2 ms), a batch leaves it to one GPU lane per MSM (4 ms).
    int lhs_fold() {
        {
            uint64_t acc[4][4] = {{0}};
            for (size_t i = 0; i < B; i++)
                for (int k = 0; k < 4; k++) mp.add(acc[k], &fixed_part[16 * i + 4 * k], acc[k]);
            mp.neg(acc[3], acc[3]);                                                   // - sum_v on G1[0]
            for (int k = 0; k < 4; k++) drh::store_le32(acc[k], lhs_sc.data() + 32 * (rf::G_PER_PROOF * B + k));
        }
        if (small) {
            // the lhs fold on the host, three or four points per worker thread (the rhs has been running since the decode)
            const drh::G1 lhs_pt = drh::g1_msm_small(host_bases.data(), lhs_sc.data(), n_g1, (unsigned)std::min<size_t>(8, std::max<size_t>(2, n_g1 / 3)));
            g1_pair_operand(lhs_pt, false, pair_g1, pair_inf);
            return DR_OK;
        }
        TRY(use_ctx(ctx));           // from here on the context's scratch is used: behind a pending wipe of it
        TRY(ctx->scalars.reserve(n_g1 * 32));
        HIP_TRY(hipMemcpyAsync(ctx->scalars.p, lhs_sc.data(), n_g1 * 32, hipMemcpyHostToDevice, st));
        return msm_to_bytes(ctx, g1_bases.as<uint32_t>(), ctx->scalars.as<uint32_t>(), n_g1, 1, pair_g1, pair_inf);
    }

    // e(lhs, G2[0]) * e(-rhs, G2[1]) == 1: the second loop comes with the rhs fold — joined only now: with one proof that thread (fold +
    // loop, ~0.45 ms from the decode on) ends after this one's lhs fold, and this loop needs nothing from it
    int pairing(int& pok) {
        drh::Fq12 f_lhs;
        TRY(pairing_miller(pair_g1, vk->g2, 1, f_lhs));
        rhs_thread.join();
        if (rhs_rc != DR_OK) return fail(rhs_rc, rhs_err.empty() ? "rhs fold failed" : rhs_err);
        pok = pairing_product_is_one(f_lhs * f_rhs) ? 1 : 0;
        return DR_OK;
    }

    int join() {
        side.join();
        tr_.mark("pedersen join");
        if (side_rc != DR_OK) return fail(side_rc, side_err.empty() ? "Pedersen part failed" : side_err);
        return DR_OK;
    }

    // ---- dr_ringvrf_verify_each: the same phases, the proofs kept apart.  The coefficients r1, r2 are drawn per proof, so the sum of
    // (L_i, R_i) over ANY subset of proofs is a sound combination of its own: the tree of these sums is built once (kernels_g1_claims.hip.h,
    // or on the host for the small route) and pairings are spent only where a subtree fails (verify_tree.hpp).
    int run_each() {
        gather();
        tr_.mark("gather");
        TRY(start_pedersen_side());
        TRY(small ? decode_host() : decode_kernels());
        tr_.mark("decode");
        replay();
        tr_.mark("replay");
        claim_scalars();
        size_t n_excluded = 0;
        for (size_t i = 0; i < B; i++) n_excluded += excluded[i];
        open_gate(1);                // (`excluded` is final from here on: the Pedersen helper reads it)
        tr_.mark("transcripts");
        const drh::VerifyTreeShape shape(B);
        TRY(small ? claim_nodes_host(shape) : claim_nodes_device(shape));
        tr_.mark("claim tree");
        size_t tested = 0;
        TRY(descend(shape, tested));
        tr_.mark("pairings");
        TRY(join());
        for (size_t i = 0; i < B; i++) verdicts[i] = (!excluded[i] && ring_each[i] && ped_each[i]) ? 1 : 0;
        if (stats) { stats[0] = (uint32_t)tested; stats[1] = (uint32_t)n_excluded; stats[2] = (uint32_t)shape.depth; stats[3] = 0; }
        return DR_OK;
    }

    // the 13 terms of proof i: its seven claim scalars on its own points, f_{i,0..3} on C_px, C_py, C_s, G1[0] (the last negated), then
    // r1, r2 on its opening proofs; all zero for an excluded proof
    static constexpr size_t CLAIM_TERMS = rf::G_PER_PROOF + rf::G_FIXED + 2, CLAIM_L = rf::G_PER_PROOF + rf::G_FIXED;
    void claim_terms(std::vector<uint32_t>& idx, std::vector<uint8_t>& sc) const {
        idx.resize(B * CLAIM_TERMS);
        sc.assign(B * CLAIM_TERMS * 32, 0);
        for (size_t i = 0; i < B; i++) {
            uint32_t* ix = &idx[CLAIM_TERMS * i];
            uint8_t* k = sc.data() + 32 * CLAIM_TERMS * i;
            for (size_t j = 0; j < rf::G_PER_PROOF; j++) ix[j] = (uint32_t)(rf::G_PER_PROOF * i + j);
            for (size_t j = 0; j < rf::G_FIXED; j++) ix[rf::G_PER_PROOF + j] = (uint32_t)(rf::G_PER_PROOF * B + j);
            ix[CLAIM_L] = (uint32_t)(rf::G_PER_PROOF * i + rf::G_OPENS);
            ix[CLAIM_L + 1] = ix[CLAIM_L] + 1;
            if (excluded[i]) continue;
            std::memcpy(k, lhs_sc.data() + 32 * rf::G_PER_PROOF * i, 32 * rf::G_PER_PROOF);
            for (size_t j = 0; j < rf::G_FIXED; j++) {
                uint64_t f[4];
                std::memcpy(f, &fixed_part[16 * i + 4 * j], 32);
                if (j == 3) mp.neg(f, f);
                drh::store_le32(f, k + 32 * (rf::G_PER_PROOF + j));
            }
            std::memcpy(k + 32 * CLAIM_L, rhs_sc.data() + 64 * i, 64);
        }
    }

    // nodes_le: the L tree then the R tree, 2 * Bp - 1 nodes each in heap order, affine standard-form little-endian x || y (zeros: identity)
    int claim_nodes_device(const drh::VerifyTreeShape& shape) {
        std::vector<uint32_t> idx;
        std::vector<uint8_t> sc;
        claim_terms(idx, sc);
        nodes_le.resize(2 * shape.nodes() * 96);
        TRY(use_ctx(ctx));           // from here on the context's scratch is used: behind a pending wipe of it
        const uint32_t off[2] = {0, (uint32_t)CLAIM_L}, m[2] = {(uint32_t)CLAIM_L, 2};
        return g1_claim_tree(ctx, g1_bases.as<uint32_t>(), idx.data(), sc.data(), B, CLAIM_TERMS, 2, off, m, nodes_le.data());
    }

    int claim_nodes_host(const drh::VerifyTreeShape& shape) {
        std::vector<uint32_t> idx;
        std::vector<uint8_t> sc;
        claim_terms(idx, sc);
        const size_t N = shape.nodes();
        std::vector<drh::G1> tree(2 * N, drh::G1::inf());
        drh::parallel_for(2 * B, [&](size_t job) {
            const size_t i = job >> 1, c = job & 1, first = CLAIM_TERMS * i + (c ? CLAIM_L : 0), m = c ? 2 : CLAIM_L;
            drh::G1AffineHost pts[CLAIM_L];
            for (size_t j = 0; j < m; j++) pts[j] = host_bases[idx[first + j]];
            tree[c * N + shape.padded - 1 + i] = drh::g1_msm_small(pts, sc.data() + 32 * first, m, 1);
        }, 1);
        for (size_t c = 0; c < 2; c++)
            for (size_t k = shape.padded - 1; k-- > 0;) tree[c * N + k] = drh::g1_add(tree[c * N + 2 * k + 1], tree[c * N + 2 * k + 2]);
        nodes_le.assign(2 * N * 96, 0);
        drh::parallel_for(2 * N, [&](size_t k) {
            drh::Fq ax, ay;
            if (!drh::g1_to_affine(tree[k], ax, ay)) return;
            ax.store_le(nodes_le.data() + 96 * k);
            ay.store_le(nodes_le.data() + 96 * k + 48);
        }, 4);
        return DR_OK;
    }

    // e(L, G2[0]) * e(-R, G2[1]) == 1 at the nodes the descent asks for, the tests of one request side by side on the worker pool
    int descend(const drh::VerifyTreeShape& shape, size_t& tested) {
        const size_t N = shape.nodes();
        std::atomic<int> rc{DR_OK};
        std::mutex err_m;
        std::string err;
        auto operand = [&](size_t node, bool negate, uint8_t out[96]) {
            const uint8_t* le = nodes_le.data() + 96 * node;
            std::memset(out, 0, 96);
            drh::Fq x, y;
            bool inf = true;
            for (int q = 0; q < 96; q++) if (le[q]) { inf = false; break; }
            if (inf || !drh::Fq::load_le(x, le) || !drh::Fq::load_le(y, le + 48)) return;
            x.store_be(out);
            (negate ? y.neg() : y).store_be(out + 48);
        };
        auto test = [&](const std::vector<size_t>& ask, std::vector<uint8_t>& pass) {
            drh::parallel_for(ask.size(), [&](size_t j) {
                uint8_t pair[2 * 96];
                operand(ask[j], false, pair);
                operand(N + ask[j], true, pair + 96);
                drh::Fq12 f;
                const int r = pairing_miller(pair, vk->g2, 2, f);
                if (r != DR_OK) {
                    std::lock_guard<std::mutex> lk(err_m);
                    if (rc.exchange(r) == DR_OK) err = dr_last_error();
                    return;
                }
                pass[j] = pairing_product_is_one(f) ? 1 : 0;
            }, 1);
        };
        ring_each.assign(B, 0);
        tested = drh::verify_tree_descend(shape, test, ring_each.data());
        if (rc.load() != DR_OK) return fail(rc.load(), err.empty() ? "pairing failed" : err);
        return DR_OK;
    }
};

int ringvrf_verify_batch_impl(dr_ctx* ctx, const dr_vrf_suite* suite, const dr_ring_verifier_key* vk, size_t batch, const uint8_t* proofs,
                                     const uint8_t* inputs, const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts,
                                     const uint64_t* salt_off, const uint8_t seed32[32], int* ok) {
    // (not use_ctx: a prover that ran on this context may have left the zeroing of its buffers on the wipe stream; the decoding phase
    //  works in verifier-owned buffers and runs beside it, the MSM phase — the first to touch the context's scratch — joins it)
    if (!ctx) return fail(DR_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    if (!vk || !proofs || !in_off || !ad_off || !seed32 || !ok || !vk->fs_prefix) return fail(DR_ERR_INVALID, "null argument");
    *ok = 0;
    if (batch == 0) { *ok = 1; return DR_OK; }
    if (batch > 4096) return fail(DR_ERR_INVALID, "batch must be at most 4096 per call");
    if (vk->log2n < 9 || vk->log2n > 16) return fail(DR_ERR_INVALID, "bad domain size");
    drh::VrfSuite su;
    TRY(load_suite(suite, su));
    TRY(offsets_ok(batch, {in_off, ad_off, salt_off}));
    RingVerifyBatch v(ctx, su, vk, batch, proofs, inputs, in_off, ads, ad_off, salts, salt_off, seed32);
    return v.run(ok);
}

// ... with a verdict per proof: the same refusals, the same phases (RingVerifyBatch::run_each)
int ringvrf_verify_each_impl(dr_ctx* ctx, const dr_vrf_suite* suite, const dr_ring_verifier_key* vk, size_t batch, const uint8_t* proofs,
                             const uint8_t* inputs, const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts,
                             const uint64_t* salt_off, const uint8_t seed32[32], uint8_t* verdicts, uint32_t* stats) {
    if (!ctx) return fail(DR_ERR_INVALID, "null context");
    HIP_TRY(hipSetDevice(ctx->device));
    if (!vk || !proofs || !in_off || !ad_off || !seed32 || !vk->fs_prefix || (batch && !verdicts)) return fail(DR_ERR_INVALID, "null argument");
    if (stats) std::memset(stats, 0, 4 * sizeof(uint32_t));
    if (batch == 0) return DR_OK;
    if (batch > 4096) return fail(DR_ERR_INVALID, "batch must be at most 4096 per call");
    std::memset(verdicts, 0, batch);
    if (vk->log2n < 9 || vk->log2n > 16) return fail(DR_ERR_INVALID, "bad domain size");
    drh::VrfSuite su;
    TRY(load_suite(suite, su));
    TRY(offsets_ok(batch, {in_off, ad_off, salt_off}));
    RingVerifyBatch v(ctx, su, vk, batch, proofs, inputs, in_off, ads, ad_off, salts, salt_off, seed32, verdicts, stats);
    return v.run_each();
}

int dr_ringvrf_verify_each(dr_ctx* ctx, const dr_vrf_suite* suite, const dr_ring_verifier_key* vk, size_t batch, const uint8_t* proofs,
                           const uint8_t* inputs, const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts,
                           const uint64_t* salt_off, const uint8_t seed32[32], uint8_t* verdicts, uint32_t* stats) {
    return abi_guard("native verifier", [&] {
        return ringvrf_verify_each_impl(ctx, suite, vk, batch, proofs, inputs, in_off, ads, ad_off, salts, salt_off, seed32, verdicts, stats);
    });
}

int dr_ringvrf_verify_batch(dr_ctx* ctx, const dr_vrf_suite* suite, const dr_ring_verifier_key* vk, size_t batch, const uint8_t* proofs,
                            const uint8_t* inputs, const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts,
                            const uint64_t* salt_off, const uint8_t seed32[32], int* ok) {
    return abi_guard("native verifier", [&] {
        return ringvrf_verify_batch_impl(ctx, suite, vk, batch, proofs, inputs, in_off, ads, ad_off, salts, salt_off, seed32, ok);
    });
}

// PedersenVRF.prove for a batch (pedersen/vrf.py:86-126): 192 bytes per proof; same code as the Pedersen part of
// dr_ringvrf_prove_batch.  out_aux (nullable): per proof O, Y_bar, R, O_k affine (4*64) and the blinding factor (32).
int dr_pedersen_prove_batch(dr_ctx* ctx, const dr_vrf_suite* suite, size_t batch, const uint8_t* alphas, const uint64_t* alpha_off,
                            const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts, const uint64_t* salt_off,
                            const uint8_t* secret_scalars, uint8_t* out_proofs, uint8_t* out_aux) {
    return abi_guard("native prover", [&]() -> int {
        TRY(use_ctx(ctx));
        if (!alpha_off || !ad_off || !secret_scalars || !out_proofs) return fail(DR_ERR_INVALID, "null argument");
        if (batch == 0) return DR_OK;
        if (batch > 65536) return fail(DR_ERR_INVALID, "batch must be at most 65536 per call");
        drh::VrfSuite su;
        TRY(load_suite(suite, su, true));
        TRY(offsets_ok(batch, {alpha_off, ad_off, salt_off}));
        PhaseTrace tr_("pedersen_prove_batch");
        if (drh::small_host_serves(su, batch)) {
            // a handful of proofs: the whole protocol on host cores (hostsigma.hpp), one proof per worker thread
            const auto tables = drh::te_suite_tables(su);
            if (!tables) return fail(DR_ERR_INVALID, "suite base point out of range");
            std::vector<int> rcs(batch, 0);
            drh::parallel_for(batch, [&](size_t i) {
                rcs[i] = drh::pedersen_prove_one(su, *tables, drh::span_of(alphas, alpha_off, i), drh::span_of(ads, ad_off, i),
                                                 drh::span_of(salts, salt_off, i), secret_scalars + 32 * i, out_proofs + 192 * i,
                                                 out_aux ? out_aux + DR_PEDERSEN_AUX_BYTES * i : nullptr);
            }, 1);
            tr_.mark("host");
            for (size_t i = 0; i < batch; i++)
                if (rcs[i]) return fail(rcs[i] == 2 ? DR_ERR_INVALID : DR_ERR_DEVICE, rcs[i] == 2 ? "nonce scalar is zero" : "hash to curve on the host: field element out of range");
            return DR_OK;
        }
        PedersenBatch ped(su, batch);
        TRY(ped.head(ctx, alphas, alpha_off, ads, ad_off, salts, salt_off, secret_scalars, tr_));
        TRY(ped.tail(ctx, out_proofs, 4 * su.point_len + 64, out_aux, DR_PEDERSEN_AUX_BYTES));
        tr_.mark("tail");
        return DR_OK;
    });
}

// PedersenVRF.batch_verify (pedersen/vrf.py:171-242) over ENCODED proofs (192 bytes each): point decoding + subgroup
// checks and hash-to-curve on the GPU, challenges on worker threads, one (5B+2)-point MSM.  *ok = 1 iff all verify.
int dr_pedersen_verify_batch(dr_ctx* ctx, const dr_vrf_suite* suite, size_t batch, const uint8_t* proofs, const uint8_t* inputs,
                             const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts, const uint64_t* salt_off,
                             int* ok) {
    return abi_guard("native verifier", [&]() -> int {
        TRY(use_ctx(ctx));
        if (!proofs || !in_off || !ad_off || !ok) return fail(DR_ERR_INVALID, "null argument");
        *ok = 0;
        if (batch == 0) { *ok = 1; return DR_OK; }
        if (batch > 65536) return fail(DR_ERR_INVALID, "batch must be at most 65536 per call");
        drh::VrfSuite su;
        TRY(load_suite(suite, su, true));
        const size_t B = batch, pl = su.point_len, plen = 4 * pl + 64;
        const drh::Mod256& mn = su.cv->n;
        TRY(offsets_ok(B, {in_off, ad_off, salt_off}));
        if (drh::small_host_serves(su, B)) {
            // a handful of proofs: decoding, hash-to-curve and both relations of every proof on host cores (hostsigma.hpp)
            const auto tables = drh::te_suite_tables(su);
            if (!tables) return fail(DR_ERR_INVALID, "suite base point out of range");
            std::vector<int> verdict(B, 0);
            drh::parallel_for(B, [&](size_t i) {
                verdict[i] = drh::pedersen_verify_one(su, *tables, proofs + 192 * i, drh::span_of(inputs, in_off, i), drh::span_of(ads, ad_off, i),
                                                      drh::span_of(salts, salt_off, i), B <= 2);
            }, 1);
            int all = 1;
            for (size_t i = 0; i < B; i++) all &= verdict[i] == drh::SIGMA_OK ? 1 : 0;
            *ok = all;
            return DR_OK;
        }
        std::vector<uint8_t> te_enc(B * 4 * pl), te_xy(B * 256), flags(B * 4), in_pts(B * 64);
        for (size_t i = 0; i < B; i++) {
            std::memcpy(te_enc.data() + 4 * pl * i, proofs + plen * i, 4 * pl);
            uint64_t v[4];
            for (int k = 0; k < 2; k++) { drh::load_le32(proofs + plen * i + 4 * pl + 32 * k, v); if (drh::Mod256::geq(v, mn.m)) return DR_OK; }   // dec_scalar
        }
        TRY(te_decode_points(ctx, su.cv->id, false, te_enc.data(), 4 * B, te_xy.data(), flags.data()));     // (TE images for the SW suite)
        for (size_t i = 0; i < 4 * B; i++) if (!flags[i]) return DR_OK;
        TRY(encode_to_curve_msgs(ctx, su, B, inputs, in_off, salts, salt_off, in_pts.data()));
        int ped_ok = 0;
        TRY(pedersen_verify_core(ctx, su, B, proofs, plen, te_xy, in_pts, ads, ad_off, ped_ok));
        *ok = ped_ok;
        return DR_OK;
    });
}

// TinyVRF.prove / ThinVRF.prove for a batch (vrf/ietf/tiny.py:53-70, thin.py): I = encode_to_curve, pk = x G, O = x I;
// transcript over the two (input, output) pairs (G, pk), (I, O); delinearised input M = G + z I; k = nonce; R = k M;
// c = challenge(R); s = k + c x.  Tiny proof = O || c (16) || s (80 bytes), Thin proof = O || R || s (96 bytes).
int dr_ietf_prove_batch(dr_ctx* ctx, const dr_vrf_suite* suite, int thin, size_t batch, const uint8_t* alphas, const uint64_t* alpha_off,
                        const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts, const uint64_t* salt_off,
                        const uint8_t* secret_scalars, uint8_t* out_proofs, uint8_t* out_aux) {
    return abi_guard("native prover", [&]() -> int {
        TRY(use_ctx(ctx));
        if (!alpha_off || !ad_off || !secret_scalars || !out_proofs) return fail(DR_ERR_INVALID, "null argument");
        if (batch == 0) return DR_OK;
        if (batch > 65536) return fail(DR_ERR_INVALID, "batch must be at most 65536 per call");
        drh::VrfSuite su;
        TRY(load_suite(suite, su, true));
        const size_t B = batch, pl = su.point_len, plen = thin ? 2 * pl + 32 : pl + 48;
        const drh::Mod256& mn = su.cv->n;
        const int cv = su.cv->id;
        TRY(offsets_ok(B, {alpha_off, ad_off, salt_off}));
        if (drh::small_host_serves(su, B)) {
            // a handful of proofs: the whole protocol on host cores (hostsigma.hpp), one proof per worker thread
            const auto tables = drh::te_suite_tables(su);
            if (!tables) return fail(DR_ERR_INVALID, "suite base point out of range");
            std::vector<int> rcs(B, 0);
            drh::parallel_for(B, [&](size_t i) {
                rcs[i] = drh::ietf_prove_one(su, *tables, thin != 0, drh::span_of(alphas, alpha_off, i), drh::span_of(ads, ad_off, i),
                                             drh::span_of(salts, salt_off, i), secret_scalars + 32 * i, out_proofs + plen * i,
                                             out_aux ? out_aux + 128 * i : nullptr);
            }, 1);
            for (size_t i = 0; i < B; i++)
                if (rcs[i]) return fail(rcs[i] == 2 ? DR_ERR_INVALID : DR_ERR_DEVICE, rcs[i] == 2 ? "nonce scalar is zero" : "hash to curve on the host: field element out of range");
            return DR_OK;
        }
        std::vector<uint8_t> xs(B * 32), inputs(B * 64), firsts(2 * B * 64), ks(B * 32);
        struct SecretGuard {         // secret scalars and nonces, on the host and in the context's scratch, do not outlive the call
            std::vector<uint8_t>*a, *b;
            dr_ctx* ctx;
            ~SecretGuard() {
                for (std::vector<uint8_t>* v : {a, b})
                    if (!v->empty()) explicit_bzero(v->data(), v->size());
                (void)ctx_wipe_scratch(ctx);
            }
        } secret_guard{&xs, &ks, ctx};
        for (size_t i = 0; i < B; i++) {
            uint64_t x[4];
            mn.reduce_bytes(secret_scalars + 32 * i, 32, false, x);
            drh::store_le32(x, xs.data() + 32 * i);
        }
        TRY(encode_to_curve_msgs(ctx, su, B, alphas, alpha_off, salts, salt_off, inputs.data()));
        // pk = x G from the generator's window table; O = x I is variable-base
        TRY(te_fixed_base_groups(ctx, cv, su.generator, xs.data(), B, 1, firsts.data()));
        TRY(te_scalar_mul_batch(ctx, cv, inputs.data(), xs.data(), B, firsts.data() + 64 * B));
        const uint8_t* pks = firsts.data();
        const uint8_t* outs = firsts.data() + 64 * B;
        // Curve25519: the identity has no encoding (the reference's point_to_string raises)
        if (drh::any_mont_identity(su, inputs.data(), B) || drh::any_mont_identity(su, firsts.data(), 2 * B))
            return fail(DR_ERR_INVALID, "cannot serialize the point at infinity");
        // the SW suite encodes the SW images: (pk_i, I_i, O_i) mapped together, one inversion per proof
        std::vector<uint8_t> pio_store;
        const uint8_t* pio = nullptr;
        if (su.cv->sw) {
            std::vector<uint8_t> t3(B * 192);
            for (size_t i = 0; i < B; i++) {
                std::memcpy(t3.data() + 192 * i, pks + 64 * i, 64);
                std::memcpy(t3.data() + 192 * i + 64, inputs.data() + 64 * i, 64);
                std::memcpy(t3.data() + 192 * i + 128, outs + 64 * i, 64);
            }
            TRY(suite_coords(ctx, su, t3.data(), 3 * B, 3, pio_store, &pio));
        }
        auto pk_c = [&](size_t i) { return pio ? pio + 192 * i : pks + 64 * i; };
        auto in_c = [&](size_t i) { return pio ? pio + 192 * i + 64 : inputs.data() + 64 * i; };
        auto out_c = [&](size_t i) { return pio ? pio + 192 * i + 128 : outs + 64 * i; };
        // transcripts, delinearisation scalar z, nonces
        std::vector<drh::Bytes> tr(B);
        std::vector<uint8_t> gpts(B * 128), gsc(B * 64);
        std::vector<int> bad(B, 0);
        uint8_t enc_g[drh::POINT_MAX];
        drh::enc_point(su, su.cv->sw ? su.generator_sw : su.generator, enc_g);
        drh::parallel_for(B, [&](size_t i) {
            uint8_t enc_pk[drh::POINT_MAX], enc_i[drh::POINT_MAX], enc_o[drh::POINT_MAX];
            drh::enc_point(su, pk_c(i), enc_pk);
            drh::enc_point(su, in_c(i), enc_i);
            drh::enc_point(su, out_c(i), enc_o);
            uint64_t z[4], x[4], k[4], one[4] = {1, 0, 0, 0};
            drh::ietf_transcript(su, thin != 0, pl, enc_g, enc_pk, enc_i, enc_o, drh::span_of(ads, ad_off, i), tr[i], z);
            std::memcpy(gpts.data() + 128 * i, su.generator, 64);
            std::memcpy(gpts.data() + 128 * i + 64, inputs.data() + 64 * i, 64);
            drh::store_le32(one, gsc.data() + 64 * i);
            drh::store_le32(z, gsc.data() + 64 * i + 32);
            drh::load_le32(xs.data() + 32 * i, x);
            if (!drh::vrf_nonce(su, tr[i], x, k)) bad[i] = 1;
            drh::store_le32(k, ks.data() + 32 * i);
        });
        for (size_t i = 0; i < B; i++) if (bad[i]) return fail(DR_ERR_INVALID, "nonce scalar is zero");
        std::vector<uint8_t> merged(B * 64), rs(B * 64);
        TRY(te_msm_groups(ctx, cv, gpts.data(), gsc.data(), B, 2, merged.data()));
        TRY(te_scalar_mul_batch(ctx, cv, merged.data(), ks.data(), B, rs.data()));
        std::vector<uint8_t> rs_store;
        const uint8_t* rs_c = nullptr;
        TRY(suite_coords(ctx, su, rs.data(), B, 1, rs_store, &rs_c));
        if (drh::any_mont_identity(su, rs.data(), B)) return fail(DR_ERR_INVALID, "cannot serialize the point at infinity");
        drh::parallel_for(B, [&](size_t i) {
            uint8_t* out = out_proofs + plen * i;
            uint8_t enc_r[drh::POINT_MAX];
            drh::enc_point(su, out_c(i), out);
            drh::enc_point(su, rs_c + 64 * i, enc_r);
            uint64_t c[4], x[4], k[4], s[4];
            drh::vrf_challenge(su, tr[i], enc_r, 1, c);
            drh::load_le32(xs.data() + 32 * i, x);
            drh::load_le32(ks.data() + 32 * i, k);
            mn.mul(c, x, s);
            mn.add(s, k, s);
            if (out_aux) {                                   // (in the suite's coordinates)
                std::memcpy(out_aux + 128 * i, out_c(i), 64);
                std::memcpy(out_aux + 128 * i + 64, rs_c + 64 * i, 64);
            }
            if (thin) {
                std::memcpy(out + pl, enc_r, pl);
                drh::store_le32(s, out + 2 * pl);
            } else {
                uint8_t cb[32];
                drh::store_le32(c, cb);
                std::memcpy(out + pl, cb, 16);
                drh::store_le32(s, out + pl + 16);
            }
        });
        return DR_OK;
    });
}


// TinyVRF.verify / ThinVRF.verify (vrf/ietf/tiny.py:72-88, thin.py:96-118) for `batch` ENCODED proofs (80 / 96 bytes each), each under its
// own compressed public key: verdict[i] = 1 verifies, 0 does not, 2 the public key is not a valid point, 3 the proof is malformed (a
// point that does not decode to a prime-order point, a non-canonical scalar) — the cases the reference raises ValueError for.  Every
// proof is checked on its own (no random linear combination), one proof per worker thread, on host cores: this is the single-proof
// entry point — one proof costs ~0.6 ms here against three kernel launch chains (2.5 ms); ThinVRF.batch_verify of many proofs is the
// one MSM on the GPU (dr_te_msm).  Elligator suites of Bandersnatch only (DR_ERR_INVALID otherwise).
int dr_ietf_verify_batch(dr_ctx* ctx, const dr_vrf_suite* suite, int thin, size_t batch, const uint8_t* proofs, const uint8_t* public_keys,
                         const uint8_t* inputs, const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts,
                         const uint64_t* salt_off, uint8_t* verdict) {
    return abi_guard("native verifier", [&]() -> int {
        if (!ctx) return fail(DR_ERR_INVALID, "null context");
        if (batch == 0) return DR_OK;
        if (!proofs || !public_keys || !in_off || !ad_off || !verdict) return fail(DR_ERR_INVALID, "null argument");
        drh::VrfSuite su;
        TRY(load_suite(suite, su));
        if (su.cv->id != 0 || su.cv->tai) return fail(DR_ERR_INVALID, "dr_ietf_verify_batch serves the Elligator suites of Bandersnatch");
        TRY(offsets_ok(batch, {in_off, ad_off, salt_off}));
        const auto tables = drh::te_suite_tables(su);
        if (!tables) return fail(DR_ERR_INVALID, "suite base point out of range");
        const size_t plen = thin ? 96 : 80;
        drh::parallel_for(batch, [&](size_t i) {
            verdict[i] = (uint8_t)drh::ietf_verify_one(su, *tables, thin != 0, proofs + plen * i, public_keys + 32 * i, drh::span_of(inputs, in_off, i),
                                                       drh::span_of(ads, ad_off, i), drh::span_of(salts, salt_off, i), batch <= 2);
        }, 1);
        return DR_OK;
    });
}

// ---- ONE batch over several GPUs of this process (SURVEY 8(b)'s additive row, 8(e) first mode; the reference's process-sharded bench,
// tests/benchmark/bench_ring_proof.py:168-182, hands index ranges out and takes every result back the same way).  Proofs are
// independent units: device g takes proofs [g B / G, (g + 1) B / G) — sizes differ by at most one, empty shards are fine — on a host
// thread of its own, and writes its 784-byte proofs straight into the caller's buffer, so the "gather" is the memory the caller
// already holds.  No collective, nothing exchanged between the devices.
namespace {
struct Shard {
    size_t lo, hi;
};
Shard shard_of(size_t n, size_t g, size_t G) {
    const size_t base = n / G, rem = n % G;
    const size_t lo = g * base + std::min(g, rem);
    return {lo, lo + base + (g < rem ? 1 : 0)};
}
// run f(g) for g < G on G threads (the calling thread takes shard 0); first failure by shard order wins
template <class F>
int run_shards(size_t G, F&& f) {
    std::vector<int> rc(G, DR_OK);
    std::vector<std::string> err(G);
    std::vector<std::thread> th;
    th.reserve(G);
    for (size_t g = 1; g < G; g++) th.emplace_back([&, g] { run_guarded(rc[g], err[g], [&] { return f(g); }); });
    run_guarded(rc[0], err[0], [&] { return f(0); });
    for (auto& t : th) t.join();
    for (size_t g = 0; g < G; g++)
        if (rc[g] != DR_OK) return fail(rc[g], "device shard " + std::to_string(g) + ": " + err[g]);
    return DR_OK;
}
}  // namespace

int dr_ringvrf_prove_batch_multi(dr_ring_prover* const* provers, size_t n_provers, const dr_vrf_suite* suite, size_t batch, const uint8_t* alphas,
                                 const uint64_t* alpha_off, const uint8_t* ads, const uint64_t* ad_off, const uint8_t* salts, const uint64_t* salt_off,
                                 const uint8_t* secret_scalars, const uint32_t* producer_index, const uint8_t* fs_prefix, size_t fs_prefix_len,
                                 const uint8_t* zk_random48, uint8_t* out_proofs, uint8_t* out_aux) {
    return abi_guard("native prover", [&]() -> int {
        if (!provers || n_provers == 0 || n_provers > 64) return fail(DR_ERR_INVALID, "1..64 provers");
        if (!alpha_off || !ad_off || !secret_scalars || !producer_index || !fs_prefix || !out_proofs) return fail(DR_ERR_INVALID, "null argument");
        for (size_t g = 0; g < n_provers; g++) {
            if (!provers[g]) return fail(DR_ERR_INVALID, "null prover");
            for (size_t h = 0; h < g; h++)
                if (provers[h] == provers[g] || ring_prover_ctx(provers[h]) == ring_prover_ctx(provers[g]))
                    return fail(DR_ERR_INVALID, "every shard needs a prover and a context of its own");
        }
        if (batch == 0) return DR_OK;
        return run_shards(n_provers, [&](size_t g) -> int {
            const Shard sh = shard_of(batch, g, n_provers);
            for (size_t lo = sh.lo; lo < sh.hi; lo += 4096) {                 // (one native call proves at most 4096 proofs)
                const size_t n = std::min<size_t>(4096, sh.hi - lo);
                TRY(ringvrf_prove_batch_impl(provers[g], suite, n, alphas, alpha_off + lo, ads, ad_off + lo, salts, salt_off ? salt_off + lo : nullptr,
                                             secret_scalars + 32 * lo, producer_index + lo, fs_prefix, fs_prefix_len,
                                             zk_random48 ? zk_random48 + 576 * lo : nullptr, out_proofs + rf::PROOF_BYTES * lo,
                                             out_aux ? out_aux + rf::AUX_BYTES * lo : nullptr));
            }
            return DR_OK;
        });
    });
}

int dr_ringvrf_verify_batch_multi(dr_ctx* const* ctxs, size_t n_ctxs, const dr_vrf_suite* suite, const dr_ring_verifier_key* vk, size_t batch,
                                  const uint8_t* proofs, const uint8_t* inputs, const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off,
                                  const uint8_t* salts, const uint64_t* salt_off, const uint8_t seed32[32], int* ok) {
    return abi_guard("native verifier", [&]() -> int {
        if (!ctxs || n_ctxs == 0 || n_ctxs > 64) return fail(DR_ERR_INVALID, "1..64 contexts");
        if (!vk || !proofs || !in_off || !ad_off || !seed32 || !ok) return fail(DR_ERR_INVALID, "null argument");
        for (size_t g = 0; g < n_ctxs; g++) {
            if (!ctxs[g]) return fail(DR_ERR_INVALID, "null context");
            for (size_t h = 0; h < g; h++)
                if (ctxs[h] == ctxs[g]) return fail(DR_ERR_INVALID, "every shard needs a context of its own");
        }
        *ok = 0;
        if (batch == 0) { *ok = 1; return DR_OK; }
        std::vector<int> verdict(n_ctxs, 1);
        TRY(run_shards(n_ctxs, [&](size_t g) -> int {
            const Shard sh = shard_of(batch, g, n_ctxs);
            for (size_t lo = sh.lo; lo < sh.hi && verdict[g]; lo += 4096) {
                const size_t n = std::min<size_t>(4096, sh.hi - lo);
                // every shard (and chunk) folds its claims with randomness of its own: SHAKE256(seed || LE64(first proof))
                uint8_t mix[40], sub[32];
                std::memcpy(mix, seed32, 32);
                for (int k = 0; k < 8; k++) mix[32 + k] = (uint8_t)((uint64_t)lo >> (8 * k));
                drh::Shake256 sh256;
                sh256.update(mix, 40);
                sh256.digest(sub, 32);
                int one = 0;
                TRY(ringvrf_verify_batch_impl(ctxs[g], suite, vk, n, proofs + rf::PROOF_BYTES * lo, inputs, in_off + lo, ads, ad_off + lo, salts,
                                              salt_off ? salt_off + lo : nullptr, sub, &one));
                verdict[g] = one;
            }
            return DR_OK;
        }));
        int all = 1;
        for (size_t g = 0; g < n_ctxs; g++) all &= verdict[g];
        *ok = all;
        return DR_OK;
    });
}

// every shard writes its slice of `verdicts`; the statistics are summed, the depth is the deepest tree's
int dr_ringvrf_verify_each_multi(dr_ctx* const* ctxs, size_t n_ctxs, const dr_vrf_suite* suite, const dr_ring_verifier_key* vk, size_t batch,
                                 const uint8_t* proofs, const uint8_t* inputs, const uint64_t* in_off, const uint8_t* ads, const uint64_t* ad_off,
                                 const uint8_t* salts, const uint64_t* salt_off, const uint8_t seed32[32], uint8_t* verdicts, uint32_t* stats) {
    return abi_guard("native verifier", [&]() -> int {
        if (!ctxs || n_ctxs == 0 || n_ctxs > 64) return fail(DR_ERR_INVALID, "1..64 contexts");
        if (!vk || !proofs || !in_off || !ad_off || !seed32 || (batch && !verdicts)) return fail(DR_ERR_INVALID, "null argument");
        for (size_t g = 0; g < n_ctxs; g++) {
            if (!ctxs[g]) return fail(DR_ERR_INVALID, "null context");
            for (size_t h = 0; h < g; h++)
                if (ctxs[h] == ctxs[g]) return fail(DR_ERR_INVALID, "every shard needs a context of its own");
        }
        if (stats) std::memset(stats, 0, 4 * sizeof(uint32_t));
        if (batch == 0) return DR_OK;
        std::vector<uint32_t> shard_stats(4 * n_ctxs, 0);
        TRY(run_shards(n_ctxs, [&](size_t g) -> int {
            const Shard sh = shard_of(batch, g, n_ctxs);
            for (size_t lo = sh.lo; lo < sh.hi; lo += 4096) {
                const size_t n = std::min<size_t>(4096, sh.hi - lo);
                // every shard (and chunk) folds its claims with randomness of its own: SHAKE256(seed || LE64(first proof))
                uint8_t mix[40], sub[32];
                std::memcpy(mix, seed32, 32);
                for (int k = 0; k < 8; k++) mix[32 + k] = (uint8_t)((uint64_t)lo >> (8 * k));
                drh::Shake256 sh256;
                sh256.update(mix, 40);
                sh256.digest(sub, 32);
                uint32_t one[4] = {0, 0, 0, 0};
                TRY(ringvrf_verify_each_impl(ctxs[g], suite, vk, n, proofs + rf::PROOF_BYTES * lo, inputs, in_off + lo, ads, ad_off + lo, salts,
                                             salt_off ? salt_off + lo : nullptr, sub, verdicts + lo, one));
                uint32_t* s = &shard_stats[4 * g];
                s[0] += one[0]; s[1] += one[1]; s[2] = std::max(s[2], one[2]);
            }
            return DR_OK;
        }));
        if (stats)
            for (size_t g = 0; g < n_ctxs; g++) {
                stats[0] += shard_stats[4 * g]; stats[1] += shard_stats[4 * g + 1]; stats[2] = std::max(stats[2], shard_stats[4 * g + 2]);
            }
        return DR_OK;
    });
}
