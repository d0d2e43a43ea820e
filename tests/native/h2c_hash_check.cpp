// Host build of dot_ring_amd/csrc/hosth2c.hpp and hostproto.hpp's hash_to_field_xmd for tests/test_h2c_hash_cpu.py.  Each input line is
//   <suite> <variant> <hex(salt)> <hex(msg)>      suite: blsg1 | blsg2 | ed448 | secp256k1 | ed25519, variant: ro | nu, "-" an empty string
//   reduce64 <hex of 64 bytes>                     fq_reduce_be64
//   reduce84 <hex of 84 bytes>                     fe_reduce_be84
// and each output line holds the field elements of hash_to_field(salt || msg) (for blsg2 the components c0 c1 of each), or the reduced
// value, as big-endian hexadecimal numbers separated by blanks.  The wide suites hash through hash_to_field_fq / hash_to_field_fe448 with
// the salt as the prefix; the 256-bit ones through hash_to_field_xmd over the joined string, as the library calls them.  The tags are
// the RFC's (the library's units choose theirs by variant; tests/test_h2c_hash_cpu.py compares those through the library itself).
// Built with -fsanitize=address,undefined -fno-sanitize-recover=all: a read past a message, a digest or a chunk ends the program.
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include <vector>

#include "hostproto.hpp"

static bool unhex(const std::string& s, std::vector<uint8_t>& out) {
    out.clear();
    if (s == "-") return true;
    if (s.size() % 2) return false;
    for (size_t i = 0; i < s.size(); i += 2) {
        unsigned v;
        if (std::sscanf(s.c_str() + i, "%2x", &v) != 1) return false;
        out.push_back((uint8_t)v);
    }
    return true;
}
static void print_le(const uint8_t* p, size_t n) {
    for (size_t i = n; i-- > 0;) std::printf("%02x", p[i]);
}

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        if (line.empty()) continue;
        std::istringstream in(line);
        std::string suite, a, b, c;
        in >> suite >> a;
        std::vector<uint8_t> salt, msg;
        if (suite == "reduce64" || suite == "reduce84") {
            const bool fq = suite == "reduce64";
            if (!unhex(a, msg) || msg.size() != (fq ? 64u : 84u)) return 2;
            std::vector<uint8_t> out(fq ? 48 : 56);            // (exact sizes on the heap: the sanitizer sees an overrun of either side)
            if (fq) drh::fq_reduce_be64(msg.data(), out.data()); else drh::fe_reduce_be84(msg.data(), out.data());
            print_le(out.data(), out.size());
            std::printf("\n");
            continue;
        }
        in >> b >> c;
        if ((a != "ro" && a != "nu") || !unhex(b, salt) || !unhex(c, msg)) return 2;
        const bool nu = a == "nu";
        const unsigned count = nu ? 1 : 2;
        const std::string tag = nu ? "NU_" : "RO_";
        size_t elem = 32, parts = count;
        std::vector<uint8_t> out;
        if (suite == "blsg1" || suite == "blsg2") {
            const std::string dst = "QUUX-V01-CS02-with-BLS12381G" + std::string(suite == "blsg1" ? "1" : "2") + "_XMD:SHA-256_SSWU_" + tag;
            elem = 48;
            parts = suite == "blsg1" ? count : 2 * count;
            out.resize(elem * parts);
            drh::hash_to_field_fq(dst.data(), dst.size(), (unsigned)parts, salt.data(), salt.size(), msg.data(), msg.size(), out.data());
        } else if (suite == "ed448") {
            const std::string dst = "QUUX-V01-CS02-with-edwards448_XOF:SHAKE256_ELL2_" + tag;
            elem = 56;
            out.resize(elem * parts);
            drh::hash_to_field_fe448(dst.data(), dst.size(), count, salt.data(), salt.size(), msg.data(), msg.size(), out.data());
        } else if (suite == "secp256k1" || suite == "ed25519") {
            const bool k1 = suite == "secp256k1";
            const std::string name = (k1 ? "QUUX-V01-CS02-with-secp256k1_XMD:SHA-256_SSWU_" : "QUUX-V01-CS02-with-edwards25519_XMD:SHA-512_ELL2_") + tag;
            const drh::Bytes dst(name.begin(), name.end());
            std::vector<uint8_t> joined(salt);
            joined.insert(joined.end(), msg.begin(), msg.end());
            out.resize(elem * parts);
            if (k1) drh::hash_to_field_xmd_sha256(dst, drh::mod_psecp256k1(), joined.data(), joined.size(), count, out.data());
            else drh::hash_to_field_xmd_sha512(dst, drh::mod_p25519(), joined.data(), joined.size(), count, out.data());
        } else {
            return 2;
        }
        for (size_t k = 0; k < parts; k++) {
            if (k) std::printf(" ");
            print_le(out.data() + elem * k, elem);
        }
        std::printf("\n");
    }
    return 0;
}
