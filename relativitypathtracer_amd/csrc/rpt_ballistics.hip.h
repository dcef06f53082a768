// rpt_ballistics.hip.h — the ballistic pass (rpt_set_ballistics / rpt_render_ballistics; not in the reference): point
// sources with a velocity of their own.  A record gives a straight worldline in the rest frame of one object — where the particle is at
// that frame's time 0, and its proper velocity u = gamma * beta there — and the window of that frame's time in which it shines.  The
// particle does not ride the object: the object is the frame the worldline is written in.  The pass solves, in closed form, for the
// event of the worldline on the camera's past light cone (or, with light delay off, on its simultaneity slice), and from there on is the
// particle pass (§20): InvLorentz into the camera's frame, the point-source Doppler law with the distance r' the camera has in the
// PARTICLE's rest frame in place of r, project_to_frame, four depth-tested taps into the star pass's accumulator (kernels 1150 and 1152,
// scatters), which kernel 1131 resolves.  With u = 0 the rules are §20's operation for operation.  Included by rpt_api.hip behind every
// other splat pass, so that the kernels before it keep their place in the translation unit.  tests/native/ballistics_oracle.c restates
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

// The body of 1150 and 1152: kernel 1130's, lane for lane.  One lane per record: three 16-byte loads of it (48 B a lane, a wave's
// records 3 KiB in a row) and, THERMAL, four bytes of xg; then the five rpt_float4 of the object the worldline is written in, InvLorentz
// and stationaryCam, 80 consecutive bytes at byte 192 of Object[object].  The index is held against object_count before anything
// follows it (the host has refused a set that names a larger one; this keeps the kernel inside Object[] whatever it is handed).  The
// object's time window is not looked at (ParticleArgs::dobjs is null and is not read): the record brings its own.  Rules 1-6 in
// registers, then per tap one 8-byte read of the pixel's record (object, dist) and, where the tap passes, three 8-byte integer atomic
// adds that return nothing.  Every tap is tested against the frame after the wrap and BEFORE its record is read, so no record, whatever
// its numbers, addresses an event record or a word outside the frame.  The records are not written and the sums are integers: the frame
// does not depend on the order of arrival.  true = a tap of this lane's record passed.
template <bool THERMAL>
RPT_DEV bool ballistic_splat(const ParticleArgs &a, const float *xg, int i) {
    bool seen = false;
    if (i < a.count) {
        const float4 *record = reinterpret_cast<const float4 *>(reinterpret_cast<const rpt_ballistic *>(a.particles) + i);
        const float4 lo = record[0], mid = record[1], hi = record[2];      // pos.xyz, object | rgb.rgb, t0 | u.xyz, t1
        float x_green = 0.0f;
        if constexpr (THERMAL) x_green = xg[i];
        const int object = __float_as_int(lo.w);
        if (object >= 0 && object < a.object_count) {
            const rpt_object *L = a.objects + object;
            rpt_float4 inv[4];
            for (int k = 0; k < 4; k++) inv[k] = L->InvLorentz[k];
            const f4 cam = ld4(L->stationaryCam);
            float X, Y, dist;
            f3 c;
            if (ballistic_place<THERMAL>(a, inv, cam, mk3(lo.x, lo.y, lo.z), mk3(hi.x, hi.y, hi.z), mid.w, hi.w, mk3(mid.x, mid.y, mid.z), x_green, X, Y, dist, c)) {
                const float xf = __builtin_floorf(X), yf = __builtin_floorf(Y);
                const int x0 = (int)xf, y0 = (int)yf;    // |X|, |Y| < 1e9: in range
                const float fx = X - xf, fy = Y - yf;
                const float depth = dist - a.depth_bias;
                for (int k = 0; k < 4; k++) {
                    int x = x0 + (k & 1);
                    const int y = y0 + (k >> 1);
                    if (a.wrap) x = x < 0 ? x + a.width : (x >= a.width ? x - a.width : x);
                    if (x < 0 || x >= a.width || y < 0 || y >= a.height) continue;
                    const size_t p = (size_t)y * (size_t)a.width + (size_t)x;
                    const uint2 head = *reinterpret_cast<const uint2 *>(a.events + p);       // object, dist
                    if (!((int)head.x < 0 || depth < __uint_as_float(head.y))) continue;
                    seen = true;
                    const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
                    unsigned long long *word = a.acc + p * 3;
                    star_add(word + 0, c.x * w);
                    star_add(word + 1, c.y * w);
                    star_add(word + 2, c.z * w);
                }
            }
        }
    }
    return seen;
}

// 1150: ballistic_splat<false>.  Particles seen: a ballot per wave, LDS, one global atomic per workgroup, as 1130.
__global__ __launch_bounds__(256) void rpt_ballistics_splat_kernel(const ParticleArgs a) {
    __shared__ unsigned int block_seen;
    const int t = (int)threadIdx.x;
    if (t == 0) block_seen = 0u;
    __syncthreads();
    const bool seen = ballistic_splat<false>(a, nullptr, (int)blockIdx.x * 256 + t);
    const unsigned long long set = __ballot(seen);
    if ((t & 63) == 0 && set) atomicAdd(&block_seen, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && block_seen) atomicAdd(a.counts, (unsigned long long)block_seen);
}

// 1152: ballistic_splat<true>, T_f for S_f with xg[count] as 1132 reads it (the host has refused a count that is not the set's)
__global__ __launch_bounds__(256) void rpt_ballistics_thermal_splat_kernel(const ParticleArgs a, const float *xg) {
    __shared__ unsigned int block_seen;
    const int t = (int)threadIdx.x;
    if (t == 0) block_seen = 0u;
    __syncthreads();
    const bool seen = ballistic_splat<true>(a, xg, (int)blockIdx.x * 256 + t);
    const unsigned long long set = __ballot(seen);
    if ((t & 63) == 0 && set) atomicAdd(&block_seen, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && block_seen) atomicAdd(a.counts, (unsigned long long)block_seen);
}

}  // namespace rptd
