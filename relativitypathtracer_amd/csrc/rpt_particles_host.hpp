// rpt_particles_host.hpp — the part of the particle pass (rpt_set_particles / rpt_render_particles) that needs no device:
// the set's validation, the largest object index it names, and the options' validation.  Plain C++17, no HIP: rpt_api.hip includes it,
// and tests/native/particles_host_main.cpp compiles it alone (under the address and undefined-behaviour sanitizers).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rpt.h"

namespace rptp {

constexpr int kMaxParticles = 1 << 22;  // 2^22 particles x 2^40 per tap cannot overflow a 64-bit accumulator (as rpts::kMaxStars)

// "" = the set is acceptable; otherwise what rpt_set_particles refuses it for (entry index and field)
inline std::string set_fault(const rpt_particle *particles, int count) {
    if (count < 0 || count > kMaxParticles) return "count is 0 .. 2^22 (4194304)";
    if (count > 0 && !particles) return "a null set with count > 0";
    for (int i = 0; i < count; i++) {
        const rpt_particle &p = particles[i];
        const std::string which = "entry " + std::to_string(i) + ": ";
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(p.pos[k]) || !std::isfinite(p.rgb[k])) return which + "every component of pos and rgb must be finite";
            if (p.rgb[k] < 0.0f) return which + "a colour channel is negative";
        }
        if (p.object < 0) return which + "object is negative";
    }
    return "";
}

// the largest object index of a set that has passed its set_fault; -1 for an empty one.  For every record that names an object: the
// particles here, and the ballistic records, the rockets and the segments (rptb, rptr, rptg::largest_object)
template <typename Record>
int largest_object_of(const Record *records, int count) {
    int largest = -1;
    for (int i = 0; i < count; i++)
        if (records[i].object > largest) largest = records[i].object;
    return largest;
}
inline int largest_object(const rpt_particle *particles, int count) { return largest_object_of(particles, count); }

// The set as the device reads it, in the caller's order: positions, indices and colours copied, padding zero
inline void prepare_set(const rpt_particle *particles, int count, rpt_particle *out) {
    for (int i = 0; i < count; i++) {
        rpt_particle p;
        std::memset(&p, 0, sizeof p);
        for (int k = 0; k < 3; k++) {
            p.pos[k] = particles[i].pos[k];
            p.rgb[k] = particles[i].rgb[k];
        }
        p.object = particles[i].object;
        out[i] = p;
    }
}

// "" = the options are acceptable; otherwise what rpt_set_particle_options refuses them for
inline std::string options_fault(int flags, float depth_bias) {
    if (flags & ~RPT_PARTICLES_INVERSE_SQUARE) return "unknown flag bits (RPT_PARTICLES_INVERSE_SQUARE is the only one)";
    if (!std::isfinite(depth_bias) || depth_bias < 0.0f) return "depth_bias must be finite and >= 0";
    return "";
}

}  // namespace rptp
