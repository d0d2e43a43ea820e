// Host-only shaping of what the single-launch entry points upload (capi_suite.hpp): zero-padded decoder records, and the identities of a
// flagged suite (Curve25519, Curve448) as flag words beside cleaned points.  No HIP include: tests/native/io_records_check.cpp builds this header
// stand-alone under the address and undefined-behaviour sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace drh {

// n inputs of enc_bytes each as records of rec_bytes (>= enc_bytes), the tail of every record zero
inline std::vector<uint8_t> pad_records(const uint8_t* in, size_t n, size_t enc_bytes, size_t rec_bytes) {
    std::vector<uint8_t> rec(n * rec_bytes, 0);
    for (size_t i = 0; i < n; i++) std::memcpy(rec.data() + rec_bytes * i, in + enc_bytes * i, enc_bytes);
    return rec;
}

inline bool all_ff(const uint8_t* p, size_t bytes) {
    for (size_t i = 0; i < bytes; i++) if (p[i] != 0xff) return false;
    return true;
}

// The identities among n points of pt_bytes each as flag words (1 = the identity).  `given`: the caller spells them out, one byte per
// point in `marks` (null: none is the identity); otherwise the identity travels inside the point, as pt_bytes of 0xff.  `clean` stays
// empty when no point is the identity, and else holds the points with the identities' bytes zeroed (a flagged point's bytes are ignored).
inline void split_identities(const uint8_t* pts, size_t n, size_t pt_bytes, bool given, const uint8_t* marks, std::vector<uint8_t>& clean,
                             std::vector<uint32_t>& flags) {
    flags.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
        if (!(given ? marks && marks[i] : all_ff(pts + pt_bytes * i, pt_bytes))) continue;
        if (clean.empty()) clean.assign(pts, pts + n * pt_bytes);
        std::memset(clean.data() + pt_bytes * i, 0, pt_bytes);
        flags[i] = 1;
    }
}

}  // namespace drh
