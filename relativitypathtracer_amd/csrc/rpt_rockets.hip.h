// rpt_rockets.hip.h — the rocket pass (rpt_set_rockets / rpt_render_rockets; not in the reference): point sources under
// constant proper acceleration.  A record gives a hyperbolic worldline in the rest frame of one object — where the rocket is at that
// frame's time 0, its proper velocity u = gamma * beta there, and the proper acceleration its crew feels — and the window of that
// frame's time in which it shines.  The rocket does not ride the object: the object is the frame the worldline is written in.  In the
// half-angle variable z = (2 / alpha) tanh(alpha s / 2) the worldline is rational, so the event on the camera's past light cone (or,
// with light delay off, on its simultaneity slice) is the root of a quadratic: + - * / and sqrt, no sinh, cosh or log.  From that event
// on the pass is the ballistic pass (§24): InvLorentz into the camera's frame, the point-source Doppler law with the distance r' the
// camera has in the ROCKET's rest frame at emission, project_to_frame, four depth-tested taps into the star pass's accumulator (kernels
// 1160 and 1162, scatters), which kernel 1131 resolves.  tests/native/rockets_oracle.c restates every rule in C.
#pragma once

#include "rpt_ballistics.hip.h"

#pragma clang fp contract(off)

namespace rptd {

// Rules 1-6 for one record written in the frame of object L: false = the rocket is skipped.  THERMAL as in particle_place.  al2 = acc.acc.
//   1  g = sqrt(1 + u.u); a0 = u.acc; av = acc + u * (a0 / (g + 1)): the 4-velocity (g, u) and the 4-acceleration (a0, av) at time 0
//   2  with d = 1 - al2 z^2 / 4: sinh(alpha s) / alpha = z / d, (cosh(alpha s) - 1) / al2 = z^2 / (2 d), cosh = 1 + al2 z^2 / (2 d)
//   3  the state at the camera's time T = cam.x.  G = sqrt((g g + (2 a0) T) + (al2 T) T) is gamma there; z0 = 2 T / (g + G) and
//      d0 = 2 D0 / (g + G)^2 with D0 = g (g + G) + a0 T, so S0 = z0 / d0 = T (g + G) / D0 and C0 = z0^2 / (2 d0) = T T / D0 without the
//      difference d0; skipped unless D0 > 0.  p = (pos + u S0) + av C0, u1 = u ch0 + av S0, a01 = g sh0 + a0 ch0, a1 = u sh0 + av ch0
//      with ch0 = 1 + al2 C0 and sh0 = al2 S0
//   4  w0 = p - cam.yzw, ww = w0.w0, n = u1.w0, m = a1.w0, Aq = (m - 1) - (ww al2) / 4, r' = sqrt(n n - Aq ww): the camera's distance
//      in the rocket's rest frame at emission.  Skipped unless 0 < r' <= FLT_MAX
//   5  the past root of Aq z^2 + 2 n z + ww = 0: -(ww / (n + r')) where n > 0, (r' - n) / Aq where n <= 0 and Aq < 0, none elsewhere; on
//      the slice the root of (R / 2 - P al2 / 4) z^2 + Q z + P = 0 that is -P / Q at al2 = 0, with P = i0.yzw.w0, Q = i0.x G + i0.yzw.u1,
//      R = i0.x a01 + i0.yzw.a1.  d = 1 - ((al2 z) z) / 4; skipped unless d > 0: the horizon
//   6  S = z / d, C = (z S) / 2; tau = G S + a01 C, w = (w0 + u1 S) + a1 C; the emission time cam.x + tau is held against [t0, t1);
//      then §24 rules 5-6 unchanged: k = inv * (tau, w), dist = |k.yzw|, n = k.yzw / dist, D = dist / r', S_f or T_f, / D^2 with
//      beaming, / r'^2 with the inverse square
template <bool THERMAL>
RPT_DEV bool rocket_place(const ParticleArgs &a, const rpt_float4 *inv, f4 cam, f3 pos, f3 u, f3 acc, float t0, float t1, f3 rgb, float xg, float &X, float &Y,
                          float &dist, f3 &c) {
    const float al2 = dot(acc, acc);
    const float g = __builtin_sqrtf(1.0f + dot(u, u));
    const float a0 = dot(u, acc);
    const f3 av = acc + u * (a0 / (g + 1.0f));
    const float T = cam.x;
    const float G = __builtin_sqrtf((g * g + (2.0f * a0) * T) + (al2 * T) * T);
    const float gG = g + G;
    const float D0 = g * gG + a0 * T;
    if (!(D0 > 0.0f)) return false;
    const float S0 = (T * gG) / D0;
    const float C0 = (T * T) / D0;
    const float ch0 = 1.0f + al2 * C0;
    const float sh0 = al2 * S0;
    const f3 p = (pos + u * S0) + av * C0;
    const f3 u1 = u * ch0 + av * S0;
    const float a01 = g * sh0 + a0 * ch0;
    const f3 a1 = u * sh0 + av * ch0;
    const f3 w0 = p - yzw(cam);
    const float ww = dot(w0, w0);
    const float n1 = dot(u1, w0);
    const float m = dot(a1, w0);
    const float Aq = (m - 1.0f) - (ww * al2) * 0.25f;
    const float rp = __builtin_sqrtf(n1 * n1 - Aq * ww);
    if (!(rp > 0.0f) || !(rp <= 3.402823466e38f)) return false;
    float z;
    if (a.interval == 0) {
        const f4 i0 = ld4(inv[0]);
        const float P = i0.y * w0.x + i0.z * w0.y + i0.w * w0.z;
        const float Q = i0.x * G + (i0.y * u1.x + i0.z * u1.y + i0.w * u1.z);
        const float R = i0.x * a01 + (i0.y * a1.x + i0.z * a1.y + i0.w * a1.z);
        const float As = 0.5f * R - (P * al2) * 0.25f;
        z = -((2.0f * P) / (Q + __builtin_sqrtf(Q * Q - (4.0f * As) * P)));
    } else if (n1 > 0.0f) {
        z = -(ww / (n1 + rp));
    } else if (Aq < 0.0f) {
        z = (rp - n1) / Aq;
    } else {
        return false;
    }
    const float d = 1.0f - ((al2 * z) * z) * 0.25f;
    if (!(d > 0.0f)) return false;
    const float S = z / d;
    const float C = (z * S) * 0.5f;
    const float tau = G * S + a01 * C;
    const f3 w = (w0 + u1 * S) + a1 * C;
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

// The rocket's record: the ballistic record and a fourth quad, acc.xyz, reserved (64 B a lane, a wave's records 4 KiB in a row).  The
// object's time window is not looked at (ParticleArgs::dobjs is null and is not read).
struct RocketSource {
    static constexpr int kQuads = 4;
    template <bool THERMAL>
    static RPT_DEV bool place(const ParticleArgs &a, const rpt_float4 *inv, f4 cam, int, const float4 *q, float xg, float &X, float &Y, float &dist, f3 &c) {
        return rocket_place<THERMAL>(a, inv, cam, mk3(q[0].x, q[0].y, q[0].z), mk3(q[2].x, q[2].y, q[2].z), mk3(q[3].x, q[3].y, q[3].z), q[1].w, q[2].w, mk3(q[1].x, q[1].y, q[1].z), xg,
                                     X, Y, dist, c);
    }
};

// 1160: one lane per record (point_splat, rpt_particles.hip.h), rules 1-6
__global__ __launch_bounds__(256) void rpt_rockets_splat_kernel(const ParticleArgs a) {
    splat_and_count(a.counts, [&](int i) { return point_splat<RocketSource, false>(a, nullptr, i); });
}

// 1162: T_f for S_f with xg[count] as 1152 reads it
__global__ __launch_bounds__(256) void rpt_rockets_thermal_splat_kernel(const ParticleArgs a, const float *xg) {
    splat_and_count(a.counts, [&](int i) { return point_splat<RocketSource, true>(a, xg, i); });
}

}  // namespace rptd
