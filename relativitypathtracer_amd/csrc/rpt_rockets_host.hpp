// rpt_rockets_host.hpp — the part of the rocket pass (rpt_set_rockets / rpt_render_rockets) that needs no device: the
// set's validation, the largest object index it names, and the copy the device reads.  The options are the particle pass's
// (rptp::options_fault).  Plain C++17, no HIP: rpt_api.hip includes it, and tests/native/rockets_host_main.cpp compiles it alone
// (under the address and undefined-behaviour sanitizers).
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "../../include/rpt.h"
#include "rpt_particles_host.hpp"

namespace rptr {

constexpr int kMaxRockets = 1 << 22;              // 2^22 records x 2^40 per tap cannot overflow a 64-bit accumulator (as rptb::kMaxBallistics)
constexpr float kMaxProperVelocity = 1000.0f;     // per component, as rptb::kMaxProperVelocity
constexpr float kMaxAcceleration = 1000.0f;       // per component: acc.acc <= 3e6, and (acc.acc T) T stays finite for every |T| < 1e15

// "" = the set is acceptable; otherwise what rpt_set_rockets refuses it for (entry index and field)
inline std::string set_fault(const rpt_rocket *records, int count) {
    if (count < 0 || count > kMaxRockets) return "count is 0 .. 2^22 (4194304)";
    if (count > 0 && !records) return "a null set with count > 0";
    for (int i = 0; i < count; i++) {
        const rpt_rocket &p = records[i];
        const std::string which = "entry " + std::to_string(i) + ": ";
        for (int k = 0; k < 3; k++) {
            if (!std::isfinite(p.pos[k]) || !std::isfinite(p.rgb[k]) || !std::isfinite(p.u[k]) || !std::isfinite(p.acc[k]))
                return which + "every component of pos, rgb, u and acc must be finite";
            if (std::fabs(p.u[k]) > kMaxProperVelocity) return which + "a component of u (gamma * beta) is beyond 1000";
            if (std::fabs(p.acc[k]) > kMaxAcceleration) return which + "a component of acc (the proper acceleration) is beyond 1000";
            if (p.rgb[k] < 0.0f) return which + "a colour channel is negative";
        }
        if (p.object < 0) return which + "object is negative";
        if (std::isnan(p.t0) || std::isnan(p.t1)) return which + "t0 or t1 is not a number";
        if (!(p.t0 < p.t1)) return which + "the window [t0, t1) is empty (t0 >= t1)";
        if (p.reserved != 0.0f) return which + "reserved must be 0";      // (a NaN is not 0 either)
    }
    return "";
}

inline int largest_object(const rpt_rocket *records, int count) { return rptp::largest_object_of(records, count); }

// The set as the device reads it, in the caller's order: the record has no padding, every field is copied
inline void prepare_set(const rpt_rocket *records, int count, rpt_rocket *out) {
    for (int i = 0; i < count; i++) {
        rpt_rocket p;
        std::memset(&p, 0, sizeof p);
        for (int k = 0; k < 3; k++) {
            p.pos[k] = records[i].pos[k];
            p.rgb[k] = records[i].rgb[k];
            p.u[k] = records[i].u[k];
            p.acc[k] = records[i].acc[k];
        }
        p.object = records[i].object;
        p.t0 = records[i].t0;
        p.t1 = records[i].t1;
        out[i] = p;
    }
}

}  // namespace rptr
