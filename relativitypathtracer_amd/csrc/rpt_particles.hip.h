// rpt_particles.hip.h — the particle pass (rpt_set_particles / rpt_render_particles; not in the reference): point sources
// at a finite distance, each at rest in the rest frame of one object, put on the camera's past light cone (or, with light delay off, on
// its simultaneity slice), taken into the camera's frame by that object's InvLorentz, Doppler-shifted and beamed as point sources,
// depth-tested tap by tap against the event records and splatted bilinearly into the star pass's per-pixel integer accumulator (kernel
// 1130, a scatter), which kernel 1131 adds to the pixels of a rendered frame, hit or miss.  A sibling of the star-field pass: included by
// rpt_api.hip behind rpt_stars.hip.h, whose star_add, clamp, fixed point and projection (§19 rule 4, project_to_frame) it uses as
// they are.  tests/native/particles_oracle.c restates every rule in C.
#pragma once

#include "rpt_stars.hip.h"

#pragma clang fp contract(off)

namespace rptd {

struct ParticleArgs {
    const rpt_particle *particles;      // [count] rest-frame positions, object indices and colours, 32 B each
    const rpt_object *objects;          // [object_count] the Object[] the frames of this view were rendered with
    const DObj *dobjs;                  // [object_count] for win_t0 / win_t1, or null: the context has no time windows
    const rpt_event *events;            // [height][width] records of the same view: read only, the first 8 bytes of a tap's
    unsigned long long *acc;            // [height * width * 3] the star pass's accumulator; all zero outside a pass
    unsigned long long *counts;         // [0]: particles seen, one atomic add per workgroup that has any
    int count, object_count;
    int width, height;
    int interval;                       // -1 or 0 (the host refuses another)
    int doppler;                        // RPT_DOPPLER_* as the rules use them: 0 when Doppler is off or interval == 0
    int camera;                         // RPT_STARS_EQUIRECT or 0
    int wrap;                           // equirect: h_fov is the full circle
    int inverse_square;                 // RPT_PARTICLES_INVERSE_SQUARE
    float depth_bias;
    float plane_x, plane_y;             // pinhole: s * aspect and s (s = 1.0f without a lens)
    float h_fov, v_fov, yaw;            // equirect
};

struct ParticleResolveArgs {
    unsigned long long *acc;
    rpt_pixel *out16;                   // the framebuffer: only the dword at byte 8 of a pixel is read and written
    unsigned long long *counts;         // [1]: pixels whose bytes changed
    unsigned long long pixels;          // width * height
    float hable_wp[3];
};

// Rules 1-4 for one particle of object L: false = the particle is skipped.  THERMAL: the colour rule is T_f with the
// particle's xg (kernel 1132); without it xg is not looked at and the rule is S_f (kernel 1130).
template <bool THERMAL>
RPT_DEV bool particle_place(const ParticleArgs &a, const rpt_float4 *inv, f4 cam, const DObj *window, f3 pos, f3 rgb, float xg, float &X, float &Y, float &dist, f3 &c) {
    const f3 w = pos - yzw(cam);
    const float r = __builtin_sqrtf(dot(w, w));
    if (!(r > 0.0f) || !(r <= 3.402823466e38f)) return false;
    float tau = -r;
    if (a.interval == 0) {
        const f4 i0 = ld4(inv[0]);
        tau = -(i0.y * w.x + i0.z * w.y + i0.w * w.z) / i0.x;
    }
    const f4 k = transformPoint4D(inv, mk4(tau, w.x, w.y, w.z));
    const f3 s = yzw(k);
    dist = __builtin_sqrtf(dot(s, s));
    if (!(dist > 0.0f) || !(dist <= 3.402823466e38f)) return false;
    const f3 n = s / dist;
    if (window && !window_accepts(*window, cam.x + tau)) return false;
    c = rgb;
    if (a.doppler != 0) {
        const float D = dist / r;
        if (!(D > 0.0f) || !(D <= 3.402823466e38f)) return false;
        if constexpr (THERMAL) c = thermal_colour(a.doppler, D, rgb, xg);
        else c = doppler_colour(a.doppler, D, rgb);
        if (a.doppler & 2) c = c / (D * D);              // a point source also loses solid angle by D^2
    }
    if (a.inverse_square) c = c / (r * r);
    return project_to_frame(a, n, X, Y);                 // §19 rule 4, as star_place has it
}

// The four depth-tested taps of a point at (X, Y), `dist` from the camera, colour c: per tap one 8-byte read of the pixel's record
// (object, dist) and, where the tap passes, three 8-byte integer atomic adds that return nothing.  Every tap is tested against the
// frame after the wrap and BEFORE its record is read, so no source, whatever its numbers, addresses a record or a word outside the
// frame.  The records are not written and the sums are integers: the frame does not depend on the order of arrival.  true = a tap
// passed.  (The lit kernels, rpt_dust.hip.h, test the taps and add to them in two phases with the light loop between: not this.)
RPT_DEV bool splat_taps(const ParticleArgs &a, float X, float Y, float dist, f3 c) {
    const float xf = __builtin_floorf(X), yf = __builtin_floorf(Y);
    const int x0 = (int)xf, y0 = (int)yf;                // |X|, |Y| < 1e9 (+ a segment's 2 pi W / h_fov + 1024): in range
    const float fx = X - xf, fy = Y - yf;
    const float depth = dist - a.depth_bias;
    bool seen = false;
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
    return seen;
}

// One lane of a point-source splat: source i of SOURCE's records.  kQuads 16-byte loads of its record (a.particles read as that
// record, 16 * kQuads bytes each) and, THERMAL, four bytes of xg (the host has refused a count that is not the set's); then the five
// rpt_float4 of the object the record names — InvLorentz and stationaryCam, 80 consecutive bytes at byte 192 of Object[object];
// neighbouring sources usually name the same object, so a wave's loads fall on one or two lines.  The index is held against
// object_count before anything follows it (the host has refused a set that names a larger one; this keeps the kernel inside Object[]
// whatever it is handed).  SOURCE::place — the pass's rules, in registers — then splat_taps.  true = a tap of this source passed.
template <class SOURCE, bool THERMAL>
RPT_DEV bool point_splat(const ParticleArgs &a, const float *xg, int i) {
    if (i >= a.count) return false;
    const float4 *record = reinterpret_cast<const float4 *>(a.particles) + (size_t)i * SOURCE::kQuads;
    float4 q[SOURCE::kQuads];
    for (int k = 0; k < SOURCE::kQuads; k++) q[k] = record[k];
    float x_green = 0.0f;
    if constexpr (THERMAL) x_green = xg[i];
    const int object = __float_as_int(q[0].w);
    if (object < 0 || object >= a.object_count) return false;
    const rpt_object *L = a.objects + object;
    rpt_float4 inv[4];
    for (int k = 0; k < 4; k++) inv[k] = L->InvLorentz[k];
    const f4 cam = ld4(L->stationaryCam);
    float X, Y, dist;
    f3 c;
    if (!SOURCE::template place<THERMAL>(a, inv, cam, object, q, x_green, X, Y, dist, c)) return false;
    return splat_taps(a, X, Y, dist, c);
}

// The particle that rides its object: pos.xyz, object | rgb.rgb, padding; with time windows, the two floats of its object's DObj
struct ParticleSource {
    static constexpr int kQuads = 2;
    template <bool THERMAL>
    static RPT_DEV bool place(const ParticleArgs &a, const rpt_float4 *inv, f4 cam, int object, const float4 *q, float xg, float &X, float &Y, float &dist, f3 &c) {
        return particle_place<THERMAL>(a, inv, cam, a.dobjs ? a.dobjs + object : nullptr, mk3(q[0].x, q[0].y, q[0].z), mk3(q[1].x, q[1].y, q[1].z), xg, X, Y, dist, c);
    }
};

// 1130: one lane per particle, rules 1-4.  Kernel 1132 (rpt_thermal.hip.h, behind T_f's definition) is the same with THERMAL.
__global__ __launch_bounds__(256) void rpt_particles_splat_kernel(const ParticleArgs a) {
    splat_and_count(a.counts, [&](int i) { return point_splat<ParticleSource, false>(a, nullptr, i); });
}

// 1131: kernel 1121 without the record read — one lane per pixel, pixels in memory order.  Where a pixel's three sums are all zero
// nothing else is read.  Elsewhere the zeros go back (the accumulator is clean again for the next pass, a star pass included), and the
// sums are tonemapped on their own and added to the pixel's R, G, B bytes, saturating, whether the record is a hit or a miss: the depth
// test has already been made, tap by tap, in 1130.
__global__ __launch_bounds__(256) void rpt_particles_resolve_kernel(const ParticleResolveArgs a) {
    __shared__ unsigned int block_changed;
    const int t = (int)threadIdx.x;
    if (t == 0) block_changed = 0u;
    __syncthreads();
    const unsigned long long p = (unsigned long long)blockIdx.x * 256ull + (unsigned long long)t;
    bool changed = false;
    if (p < a.pixels) {
        unsigned long long *word = a.acc + p * 3ull;
        const unsigned long long sum[3] = {word[0], word[1], word[2]};
        if ((sum[0] | sum[1] | sum[2]) != 0ull) {
            word[0] = 0ull;
            word[1] = 0ull;
            word[2] = 0ull;
            uint32_t *rgba = reinterpret_cast<uint32_t *>(a.out16 + p) + 2;
            const uint32_t before = *rgba;
            uint32_t now = before & 0xff000000u;
            for (int k = 0; k < 3; k++) {
                const float S = (float)sum[k] * (1.0f / RPT_STARS_ONE);
                const uint32_t add = to_u8(cl_min(hable1(S) / a.hable_wp[k], 1.0f));
                const uint32_t byte = ((before >> (8 * k)) & 255u) + add;
                now |= (byte > 255u ? 255u : byte) << (8 * k);
            }
            changed = now != before;
            if (changed) *rgba = now;
        }
    }
    const unsigned long long set = __ballot(changed);
    if ((t & 63) == 0 && set) atomicAdd(&block_changed, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && block_changed) atomicAdd(a.counts + 1, (unsigned long long)block_changed);
}

}  // namespace rptd
