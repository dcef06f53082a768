// rpt_ballistics.hip.h — the ballistic pass (rpt_set_ballistics / rpt_render_ballistics; not in the reference): point
// sources with a velocity of their own.  A record gives a straight worldline in the rest frame of one object — where the particle is at
// that frame's time 0, and its proper velocity u = gamma * beta there — and the window of that frame's time in which it shines.  The
// particle does not ride the object: the object is the frame the worldline is written in.  The pass solves, in closed form, for the
// event of the worldline on the camera's past light cone (or, with light delay off, on its simultaneity slice), and from there on is the
// particle pass (§20): InvLorentz into the camera's frame, the point-source Doppler law with the distance r' the camera has in the
// PARTICLE's rest frame in place of r, project_to_frame, four depth-tested taps into the star pass's accumulator (kernels 1150 and 1152,
// scatters), which kernel 1131 resolves.  With u = 0 the rules are §20's operation for operation.  tests/native/ballistics_oracle.c restates
// every rule in C.
#pragma once

#include "rpt_particles.hip.h"

#pragma clang fp contract(off)

namespace rptd {

// Rules 1-6 for one record written in the frame of object L: false = the particle is skipped.  THERMAL as in particle_place.
//   1  g = sqrt(1 + u.u), beta = u / g
//   2  w0 = (pos + beta * cam.x) - cam.yzw: the particle's place at the camera's time, from the camera.  a = u.w0,
//      r' = sqrt(w0.w0 + a * a) = gamma * (r + beta.w): the camera's distance in the particle's rest frame
//   3  tau, the emission time less the camera's: on the light cone g * (a - r') for an approaching particle (a <= 0: both terms have
//      one sign), -g * (w0.w0) / (a + r') for a receding one (the same root, without the cancellation); on the slice
//      -(i0.yzw.w0) / (i0.x + i0.yzw.beta)
//   4  w = w0 + beta * tau; the emission time cam.x + tau is held against [t0, t1)
//   5  k = inv * (tau, w), dist = |k.yzw|, n = k.yzw / dist
//   6  D = dist / r', S_f or T_f, / D^2 with beaming, / r'^2 with the inverse square
template <bool THERMAL>
RPT_DEV bool ballistic_place(const ParticleArgs &a, const rpt_float4 *inv, f4 cam, f3 pos, f3 u, float t0, float t1, f3 rgb, float xg, float &X, float &Y, float &dist, f3 &c) {
    const float g = __builtin_sqrtf(1.0f + dot(u, u));
    const f3 beta = u / g;
    const f3 w0 = (pos + beta * cam.x) - yzw(cam);
    const float ww = dot(w0, w0);
    const float al = dot(u, w0);
    const float rp = __builtin_sqrtf(ww + al * al);
    if (!(rp > 0.0f) || !(rp <= 3.402823466e38f)) return false;
    float tau;
    if (a.interval == 0) {
        const f4 i0 = ld4(inv[0]);
        tau = -(i0.y * w0.x + i0.z * w0.y + i0.w * w0.z) / (i0.x + (i0.y * beta.x + i0.z * beta.y + i0.w * beta.z));
    } else if (al <= 0.0f) {
        tau = g * (al - rp);
    } else {
        tau = -((g * ww) / (al + rp));
    }
    const f3 w = w0 + beta * tau;
    const float t = cam.x + tau;
    if (t < t0 || t >= t1) return false;
    const f4 k = transformPoint4D(inv, mk4(tau, w.x, w.y, w.z));
    const f3 s = yzw(k);
    dist = __builtin_sqrtf(dot(s, s));
    if (!(dist > 0.0f) || !(dist <= 3.402823466e38f)) return false;
    const f3 n = s / dist;
    c = rgb;
    if (a.doppler != 0) {
        const float D = dist / rp;
        if (!(D > 0.0f) || !(D <= 3.402823466e38f)) return false;
        if constexpr (THERMAL) c = thermal_colour(a.doppler, D, rgb, xg);
        else c = doppler_colour(a.doppler, D, rgb);
        if (a.doppler & 2) c = c / (D * D);              // a point source also loses solid angle by D^2
    }
    if (a.inverse_square) c = c / (rp * rp);
    return project_to_frame(a, n, X, Y);                 // §19 rule 4, as star_place has it
}

// The ballistic record: pos.xyz, object | rgb.rgb, t0 | u.xyz, t1 (48 B a lane, a wave's records 3 KiB in a row).  The object's time
// window is not looked at (ParticleArgs::dobjs is null and is not read): the record brings its own.
struct BallisticSource {
    static constexpr int kQuads = 3;
    template <bool THERMAL>
    static RPT_DEV bool place(const ParticleArgs &a, const rpt_float4 *inv, f4 cam, int, const float4 *q, float xg, float &X, float &Y, float &dist, f3 &c) {
        return ballistic_place<THERMAL>(a, inv, cam, mk3(q[0].x, q[0].y, q[0].z), mk3(q[2].x, q[2].y, q[2].z), q[1].w, q[2].w, mk3(q[1].x, q[1].y, q[1].z), xg, X, Y, dist, c);
    }
};

// 1150: one lane per record (point_splat, rpt_particles.hip.h), rules 1-6
__global__ __launch_bounds__(256) void rpt_ballistics_splat_kernel(const ParticleArgs a) {
    splat_and_count(a.counts, [&](int i) { return point_splat<BallisticSource, false>(a, nullptr, i); });
}

// 1152: T_f for S_f with xg[count] as 1132 reads it
__global__ __launch_bounds__(256) void rpt_ballistics_thermal_splat_kernel(const ParticleArgs a, const float *xg) {
    splat_and_count(a.counts, [&](int i) { return point_splat<BallisticSource, true>(a, xg, i); });
}

}  // namespace rptd
