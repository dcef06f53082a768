// rpt_segments_host.hpp — the part of the segment pass (rpt_set_segments / rpt_render_segments) that needs no device: the
// set's validation, the largest object index it names, the options' validation and the count x pieces limit.  Plain C++17, no HIP:
// rpt_api.hip includes it, and tests/native/segments_host_main.cpp compiles it alone (under the address and undefined-behaviour
// sanitizers).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rpt.h"
#include "rpt_particles_host.hpp"

namespace rptg {

// count x pieces: one piece adds to any one accumulator word at most 4 times (§22, rule S4), each add at most 2^40 after star_add's
// clamp, and 2^21 x 4 x 2^40 = 2^63 < 2^64: the 64-bit sums cannot wrap
constexpr long long kMaxPieces = 1ll << 21;
constexpr int kDefaultPieces = 16;

// "" = count x pieces is within the limit
inline std::string load_fault(int count, int pieces) {
    if ((long long)count * (long long)pieces > kMaxPieces)
        return "count * pieces is " + std::to_string((long long)count * (long long)pieces) + " (" + std::to_string(count) + " segments, pieces " +
               std::to_string(pieces) + "); the limit is 2^21 (2097152)";
    return "";
}

// "" = the set is acceptable with `pieces` in force; otherwise what rpt_set_segments refuses it for (entry index and field)
inline std::string set_fault(const rpt_segment *segments, int count, int pieces) {
    if (count < 0) return "count is negative";
    const std::string load = load_fault(count, pieces);
    if (!load.empty()) return load;
    if (count > 0 && !segments) return "a null set with count > 0";
    for (int i = 0; i < count; i++) {
        const rpt_segment &s = segments[i];
        const std::string which = "entry " + std::to_string(i) + ": ";
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(s.a[k]) || !std::isfinite(s.b[k]) || !std::isfinite(s.rgb[k])) return which + "every component of a, b and rgb must be finite";
            if (s.rgb[k] < 0.0f) return which + "a colour channel is negative";
        }
        if (s.object < 0) return which + "object is negative";
    }
    return "";
}

inline int largest_object(const rpt_segment *segments, int count) { return rptp::largest_object_of(segments, count); }

// The set as the device reads it, in the caller's order: ends, indices and colours copied, padding zero
inline void prepare_set(const rpt_segment *segments, int count, rpt_segment *out) {
    for (int i = 0; i < count; i++) {
        rpt_segment s;
        std::memset(&s, 0, sizeof s);
        for (int k = 0; k < 3; k++) {
            s.a[k] = segments[i].a[k];
            s.b[k] = segments[i].b[k];
            s.rgb[k] = segments[i].rgb[k];
        }
        s.object = segments[i].object;
        out[i] = s;
    }
}

// "" = the options are acceptable for a set of `count` segments; otherwise what rpt_set_segment_options refuses them for
inline std::string options_fault(int flags, float depth_bias, int pieces, int count) {
    if (flags & ~RPT_SEGMENTS_INVERSE_SQUARE) return "unknown flag bits (RPT_SEGMENTS_INVERSE_SQUARE is the only one)";
    if (!std::isfinite(depth_bias) || depth_bias < 0.0f) return "depth_bias must be finite and >= 0";
    if (pieces < 1 || pieces > 64 || (pieces & (pieces - 1)) != 0) return "pieces is one of 1, 2, 4, 8, 16, 32, 64, not " + std::to_string(pieces);
    return load_fault(count, pieces);
}

}  // namespace rptg
