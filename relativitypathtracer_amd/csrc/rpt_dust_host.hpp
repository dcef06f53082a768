// rpt_dust_host.hpp — the part of the lit particles (rpt_set_particle_lighting) that needs no device: the flags'
// validation, the launch's two refusals of its own as predicates, and the choice of the splat kernel.  Plain C++17, no HIP: rpt_api.hip
// includes it, and tests/native/dust_host_main.cpp compiles it alone (under the address and undefined-behaviour sanitizers).
#pragma once

#include <string>

#include "../../include/rpt.h"

namespace rptl {

constexpr int kAllFlags = RPT_PARTICLES_LIT | RPT_PARTICLES_SHADOWED | RPT_PARTICLES_AMBIENT;

// "" = the flags are acceptable; otherwise what rpt_set_particle_lighting refuses them for
inline std::string lighting_fault(int flags) {
    if (flags & ~kAllFlags) return "unknown flag bits (RPT_PARTICLES_LIT, RPT_PARTICLES_SHADOWED and RPT_PARTICLES_AMBIENT are the three)";
    if ((flags & RPT_PARTICLES_SHADOWED) && !(flags & RPT_PARTICLES_LIT)) return "RPT_PARTICLES_SHADOWED needs RPT_PARTICLES_LIT";
    if ((flags & RPT_PARTICLES_AMBIENT) && !(flags & RPT_PARTICLES_LIT)) return "RPT_PARTICLES_AMBIENT needs RPT_PARTICLES_LIT";
    return "";
}

// What rpt_render_particles refuses a lit pass for: the code it returns (RPT_OK = the pass may be launched) and the message.
// thermal_count: the temperatures set (rpt_set_particle_temperatures) — an argument of the caller's, RPT_ERR_ARG; derived_layout: the
// scene's octrees have the derived layout the shadow ray's walk reads — a state of the uploaded scene, RPT_ERR_STATE, as
// rpt_probe_object answers it.
struct LaunchFault {
    int code;
    std::string message;
};
inline LaunchFault launch_fault(int flags, int thermal_count, bool derived_layout) {
    if (!(flags & RPT_PARTICLES_LIT)) return {RPT_OK, ""};
    if (thermal_count != 0)
        return {RPT_ERR_ARG, "RPT_PARTICLES_LIT with particle temperatures set (rpt_set_particle_temperatures): a scattered spectrum is not the grain's blackbody"};
    if ((flags & RPT_PARTICLES_SHADOWED) && !derived_layout)
        return {RPT_ERR_STATE, "RPT_PARTICLES_SHADOWED on a scene whose octree has no derived layout (children not consecutive)"};
    return {RPT_OK, ""};
}

// The splat kernel of a pass: 1130 plain (1132 with temperatures), 1134 lit, 1135 lit and shadowed, 1136 the same with time windows.
// With interval 0 the lit pass is the plain one (rule D0) and launches it.
inline int splat_kernel(int flags, int interval, int thermal_count, bool windows) {
    if (!(flags & RPT_PARTICLES_LIT) || interval == 0) return thermal_count != 0 ? 1132 : 1130;
    if (!(flags & RPT_PARTICLES_SHADOWED)) return 1134;
    return windows ? 1136 : 1135;
}

}  // namespace rptl
