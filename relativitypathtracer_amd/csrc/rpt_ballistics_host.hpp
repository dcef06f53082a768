// rpt_ballistics_host.hpp — the part of the ballistic pass (rpt_set_ballistics / rpt_render_ballistics) that needs no
// device: the set's validation, the largest object index it names, and the copy the device reads.  The options are the particle pass's
// (rptp::options_fault).  Plain C++17, no HIP: rpt_api.hip includes it, and tests/native/ballistics_host_main.cpp compiles it alone
// (under the address and undefined-behaviour sanitizers).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rpt.h"
#include "rpt_particles_host.hpp"

namespace rptb {

constexpr int kMaxBallistics = 1 << 22;     // 2^22 records x 2^40 per tap cannot overflow a 64-bit accumulator (as rptp::kMaxParticles)
constexpr float kMaxProperVelocity = 1000.0f;     // per component: gamma <= 1733, and u.u, 1 + u.u and a * a stay far from overflow

// "" = the set is acceptable; otherwise what rpt_set_ballistics refuses it for (entry index and field)
inline std::string set_fault(const rpt_ballistic *records, int count) {
    if (count < 0 || count > kMaxBallistics) return "count is 0 .. 2^22 (4194304)";
    if (count > 0 && !records) return "a null set with count > 0";
    for (int i = 0; i < count; i++) {
        const rpt_ballistic &p = records[i];
        const std::string which = "entry " + std::to_string(i) + ": ";
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(p.pos[k]) || !std::isfinite(p.rgb[k]) || !std::isfinite(p.u[k])) return which + "every component of pos, rgb and u must be finite";
            if (std::fabs(p.u[k]) > kMaxProperVelocity) return which + "a component of u (gamma * beta) is beyond 1000";
            if (p.rgb[k] < 0.0f) return which + "a colour channel is negative";
        }
        if (p.object < 0) return which + "object is negative";
        if (std::isnan(p.t0) || std::isnan(p.t1)) return which + "t0 or t1 is not a number";
        if (!(p.t0 < p.t1)) return which + "the window [t0, t1) is empty (t0 >= t1)";
    }
    return "";
}

inline int largest_object(const rpt_ballistic *records, int count) { return rptp::largest_object_of(records, count); }

// The set as the device reads it, in the caller's order: the record has no padding, every field is copied
inline void prepare_set(const rpt_ballistic *records, int count, rpt_ballistic *out) {
    for (int i = 0; i < count; i++) {
        rpt_ballistic p;
        std::memset(&p, 0, sizeof p);
        for (int k = 0; k < 3; k++) {
            p.pos[k] = records[i].pos[k];
            p.rgb[k] = records[i].rgb[k];
            p.u[k] = records[i].u[k];
        }
        p.object = records[i].object;
        p.t0 = records[i].t0;
        p.t1 = records[i].t1;
        out[i] = p;
    }
}

}  // namespace rptb
