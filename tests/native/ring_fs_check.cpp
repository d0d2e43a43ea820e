// Command-line harness around dot_ring_amd/csrc/hostring.hpp (the ring proof's Fiat-Shamir schedule in groups of four proofs) and the
// verifier arithmetic beside RingClaimScalars in hostproto.hpp, plain g++, no GPU: tests/test_ring_fs_cpu.py compares it with the
// oracle and with Python integers.  One command per line on stdin, fields in hex:
//   schedule <fs prefix> <B> <relations B*64> <cols B*384> <cq B*96> <evals B*224> <l_zw B*32>
//                                          -> "challenges <alphas B*224> <zetas B*32> <nus B*256>" | "error <why>"
//       run twice: a round at a time over all groups (as the prover does between its GPU phases) and group by group through all three
//       rounds (the verifier's replay); the two must agree
//   random <seed32> <i> <k>                -> "scalar <le32>"
//   fold <claim scalars 15*32: nus[8] k_ip k_x k_y zeta zeta_omega agg_zeta l_zw> <r1> <r2>
//                                          -> "fold <lhs 7*32> <fixed 4*32>"
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>

#include "hostring.hpp"

using namespace drh;
namespace rf = drh::ringfmt;

static Bytes unhex(const std::string& s) {
    Bytes out;
    if (s == "-") return out;
    for (size_t i = 0; i + 1 < s.size(); i += 2) out.push_back((uint8_t)std::stoul(s.substr(i, 2), nullptr, 16));
    return out;
}
static std::string hex(const uint8_t* p, size_t n) {
    static const char* d = "0123456789abcdef";
    std::string s;
    for (size_t i = 0; i < n; i++) { s.push_back(d[p[i] >> 4]); s.push_back(d[p[i] & 15]); }
    return s;
}

struct ScheduleInput {
    size_t B;
    Bytes prefix, rel, cols, cq, evals, lzw;
};
struct Challenges {
    Bytes alphas, zetas, nus;
    explicit Challenges(size_t B) : alphas(B * rf::ALPHAS_BYTES), zetas(B * 32), nus(B * rf::NUS_BYTES) {}
    bool operator==(const Challenges& o) const { return alphas == o.alphas && zetas == o.zetas && nus == o.nus; }
};

static void round1(RingFsGroup& t, const ScheduleInput& in, Challenges& c) {
    t.round_alphas([&](size_t i) { return in.rel.data() + 64 * i; }, [&](size_t i, uint8_t* ser) { std::memcpy(ser, in.cols.data() + 384 * i, 384); },
                   c.alphas.data());
}
static void round2(RingFsGroup& t, const ScheduleInput& in, Challenges& c) {
    t.round_zeta([&](size_t i, uint8_t* ser) { std::memcpy(ser, in.cq.data() + 96 * i, 96); }, c.zetas.data());
}
static void round3(RingFsGroup& t, const ScheduleInput& in, Challenges& c) {
    t.round_nus([&](size_t i) { return in.evals.data() + 224 * i; }, [&](size_t i) { return in.lzw.data() + 32 * i; }, c.nus.data());
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "schedule") {
            std::string prefix, rel, cols, cq, evals, lzw;
            ScheduleInput s;
            in >> prefix >> s.B >> rel >> cols >> cq >> evals >> lzw;
            s.prefix = unhex(prefix); s.rel = unhex(rel); s.cols = unhex(cols); s.cq = unhex(cq); s.evals = unhex(evals); s.lzw = unhex(lzw);
            const size_t B = s.B;
            if (B == 0 || s.rel.size() != 64 * B || s.cols.size() != 384 * B || s.cq.size() != 96 * B || s.evals.size() != 224 * B || s.lzw.size() != 32 * B) {
                std::puts("error bad lengths");
                std::fflush(stdout);
                continue;
            }
            FsTranscript4 base;
            base.sh.update_same(s.prefix.data(), s.prefix.size());
            const size_t G = RingFsGroup::groups(B);
            Challenges by_round(B), by_group(B);
            {
                std::vector<RingFsGroup> fs;
                fs.reserve(G);
                for (size_t g = 0; g < G; g++) fs.emplace_back(base, g, B);
                for (size_t g = 0; g < G; g++) round1(fs[g], s, by_round);
                for (size_t g = 0; g < G; g++) round2(fs[g], s, by_round);
                for (size_t g = 0; g < G; g++) round3(fs[g], s, by_round);
            }
            for (size_t g = 0; g < G; g++) {
                RingFsGroup t(base, g, B);
                round1(t, s, by_group);
                round2(t, s, by_group);
                round3(t, s, by_group);
            }
            if (!(by_round == by_group)) std::puts("error the prover's and the verifier's use of the schedule disagree");
            else std::printf("challenges %s %s %s\n", hex(by_round.alphas.data(), by_round.alphas.size()).c_str(),
                             hex(by_round.zetas.data(), by_round.zetas.size()).c_str(), hex(by_round.nus.data(), by_round.nus.size()).c_str());
        } else if (cmd == "random") {
            std::string seed;
            unsigned long long i = 0;
            int k = 0;
            in >> seed >> i >> k;
            Bytes sb = unhex(seed);
            if (sb.size() != 32) { std::puts("error bad seed"); std::fflush(stdout); continue; }
            uint64_t r[4];
            uint8_t out[32];
            ring_verifier_randomness(sb.data(), i, k, r);
            store_le32(r, out);
            std::printf("scalar %s\n", hex(out, 32).c_str());
        } else if (cmd == "fold") {
            std::string cl_hex, r1_hex, r2_hex;
            in >> cl_hex >> r1_hex >> r2_hex;
            Bytes cb = unhex(cl_hex), r1b = unhex(r1_hex), r2b = unhex(r2_hex);
            if (cb.size() != 15 * 32 || r1b.size() != 32 || r2b.size() != 32) { std::puts("error bad lengths"); std::fflush(stdout); continue; }
            RingClaimScalars cl;
            uint64_t* fields[15] = {cl.nus[0], cl.nus[1], cl.nus[2], cl.nus[3], cl.nus[4], cl.nus[5], cl.nus[6], cl.nus[7],
                                    cl.k_ip, cl.k_x, cl.k_y, cl.zeta, cl.zeta_omega, cl.agg_zeta, cl.l_zw};
            for (int j = 0; j < 15; j++) load_le32(cb.data() + 32 * j, fields[j]);
            uint64_t r1[4], r2[4], fixed[16];
            load_le32(r1b.data(), r1);
            load_le32(r2b.data(), r2);
            uint8_t lhs[7 * 32], fx[4 * 32];
            ring_claim_fold(cl, r1, r2, lhs, fixed);
            for (int j = 0; j < 4; j++) store_le32(fixed + 4 * j, fx + 32 * j);
            std::printf("fold %s %s\n", hex(lhs, sizeof lhs).c_str(), hex(fx, sizeof fx).c_str());
        } else if (!cmd.empty()) {
            std::puts("error unknown command");
        }
        std::fflush(stdout);
    }
    return 0;
}
