// rpt_stars.hip.h — the star-field pass (rpt_set_stars / rpt_render_stars; not in the reference): point sources in the
// sky's rest frame, aberrated into the camera's, Doppler-shifted and beamed as point sources, splatted bilinearly into a per-pixel
// integer accumulator (kernel 1120, a scatter) and added to the miss pixels of a rendered frame (kernel 1121).  A sibling of the overlay
// and the readout pass: it reads the event records and the framebuffer's packed colour, and writes that colour's R, G, B.  Included by
// rpt_api.hip behind rpt_kernels.hip.h, whose helpers (transformPoint4D, normalize, doppler_colour, rpt_atan2f, rpt_asinf, hable1, to_u8)
// it uses as they are.  tests/native/stars_oracle.c restates every rule in C.
#pragma once

#include "rpt_kernels.hip.h"

#pragma clang fp contract(off)

namespace rptd {

#define RPT_STARS_EQUIRECT 1            /* StarArgs::camera: 0 = the pinhole (with or without a lens) */
#define RPT_STARS_CLAMP 65536.0f        /* a tap's contribution per channel, before the fixed point */
#define RPT_STARS_ONE 16777216.0f       /* 2^24: the accumulator's unit */

struct StarArgs {
    const rpt_star *stars;              // [count] unit directions in the sky's rest frame and colours, 32 B each
    unsigned long long *acc;            // [height * width * 3] fixed-point sums, R, G, B per pixel; all zero outside a pass
    unsigned long long *counts;         // [0]: stars with a tap inside the frame, one atomic add per workgroup that has any
    rpt_float4 G[4];                    // sky -> camera, rows t, x, y, z (rule 1)
    int count;
    int width, height;
    int interval;
    int doppler;                        // RPT_DOPPLER_* as the rules use them: 0 when Doppler is off or interval == 0
    int camera;                         // RPT_STARS_EQUIRECT or 0
    int wrap;                           // equirect: h_fov is the full circle, a column tap left of column 0 lands on column width - 1 and back
    float plane_x, plane_y;             // pinhole: s * aspect and s (s = 1.0f without a lens)
    float h_fov, v_fov, yaw;            // equirect
};

struct StarResolveArgs {
    unsigned long long *acc;
    const rpt_event *events;            // [height][width] records of the same view
    rpt_pixel *out16;                   // the framebuffer: only the dword at byte 8 of a pixel is read and written
    unsigned long long *counts;         // [1]: pixels whose bytes changed
    unsigned long long pixels;          // width * height
    float hable_wp[3];
};

// T_f of rpt_thermal.hip.h, which rpt_api.hip includes behind this header: S_f where xg == 0, Planck's law elsewhere
RPT_DEV f3 thermal_colour(int flags, float D, f3 c, float xg);

// Rule 4 for a unit direction n in the camera's frame, for StarArgs and ParticleArgs alike (the view's fields have the same names in
// both): the equirect or the pinhole projection to (X, Y).  false = behind the pinhole, or no finite position.
template <typename Args>
RPT_DEV bool project_to_frame(const Args &a, f3 n, float &X, float &Y) {
    if (a.camera == RPT_STARS_EQUIRECT) {
        const float pi = (float)RPT_PI_D, two_pi = (float)(2.0 * RPT_PI_D);
        float lambda = rpt_atan2f(n.x, n.z) - a.yaw;
        lambda = lambda - two_pi * __builtin_floorf((lambda + pi) / two_pi);
        const float ny = n.y < -1.0f ? -1.0f : (n.y > 1.0f ? 1.0f : n.y);
        const float phi = rpt_asinf(ny);
        X = (float)a.width * (lambda / a.h_fov + 0.5f) - 0.5f;
        Y = (float)a.height * (phi / a.v_fov + 0.5f) - 0.5f;
    } else {
        if (!(n.z > 0.0f)) return false;
        X = (float)a.width * (0.5f + ((0.5f * n.x) / n.z) / a.plane_x);
        Y = (float)a.height * (0.5f + ((0.5f * n.y) / n.z) / a.plane_y);
    }
    return fabsf(X) < 1e9f && fabsf(Y) < 1e9f;           // (a NaN fails both)
}

// Rules 1-4 for one star: false = the star is skipped (D not finite or not > 0, behind the pinhole, no finite position).
// THERMAL: the colour rule is T_f with the star's xg (kernel 1122); without it xg is not looked at and the rule is S_f (kernel 1120).
template <bool THERMAL>
RPT_DEV bool star_place(const StarArgs &a, f3 s, f3 rgb, float xg, float &X, float &Y, f3 &c) {
    const f4 q = transformPoint4D(a.G, mk4((float)a.interval, s.x, s.y, s.z));
    c = rgb;
    if (a.interval != 0) {
        const float D = q.x / (float)a.interval;
        if (!(D > 0.0f) || !(D <= 3.402823466e38f)) return false;
        if (a.doppler != 0) {
            if constexpr (THERMAL) c = thermal_colour(a.doppler, D, rgb, xg);
            else c = doppler_colour(a.doppler, D, rgb);
        }
        if (a.doppler & 2) c = c / (D * D);              // a point source also loses solid angle by D^2
    }
    return project_to_frame(a, normalize(yzw(q)), X, Y);
}

// one channel of one tap into the accumulator: nothing for p <= 0 or NaN, the clamp, the fixed point, a fire-and-forget integer add
RPT_DEV void star_add(unsigned long long *word, float p) {
    if (!(p > 0.0f)) return;
    if (p > RPT_STARS_CLAMP) p = RPT_STARS_CLAMP;
    const unsigned long long q = (unsigned long long)(p * RPT_STARS_ONE);
    if (q != 0ull) (void)__hip_atomic_fetch_add(word, q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// A splat kernel's frame: `lane` is handed this lane's global index and says whether its source left a tap; the lanes that did are
// counted by a ballot per wave, the four waves' counts added in LDS, one global atomic per workgroup that has any.  Every lane reaches
// both barriers: a lane function returns early, the frame does not.
template <typename Lane>
RPT_DEV void splat_and_count(unsigned long long *counts, Lane lane) {
    __shared__ unsigned int block_seen;
    const int t = (int)threadIdx.x;
    if (t == 0) block_seen = 0u;
    __syncthreads();
    const bool seen = lane((int)blockIdx.x * 256 + t);
    const unsigned long long set = __ballot(seen);
    if ((t & 63) == 0 && set) atomicAdd(&block_seen, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && block_seen) atomicAdd(counts, (unsigned long long)block_seen);
}

// One lane of 1120 and 1122: one star.  Two 16-byte loads of its record and, THERMAL, xg[i] — one float per star in the catalogue's
// order, a wave 256 consecutive bytes; the host launches 1122 only with an array of exactly a.count entries (enqueue_stars refuses
// another), so i < a.count keeps the load inside it.  Rules 1-4 in registers (G and the camera are kernel arguments: scalar loads), then
// up to twelve 8-byte integer atomic adds that return nothing — the four pixels around (X, Y), three channels each, a pixel's three
// words 24 consecutive bytes and a row's two pixels 48.  Every tap is tested against the frame after the wrap, so no star, whatever its
// numbers, addresses a word outside the width * height * 3 of `acc`.  Integer sums do not depend on the order of arrival.  The taps
// have no depth test and read no record: they are not splat_taps (rpt_particles.hip.h).  true = a tap is inside the frame.
template <bool THERMAL>
RPT_DEV bool star_splat(const StarArgs &a, const float *xg, int i) {
    if (i >= a.count) return false;
    const float4 *record = reinterpret_cast<const float4 *>(a.stars + i);
    const float4 lo = record[0], hi = record[1];         // dir.xyz, rgb.r | rgb.g, rgb.b, padding
    float x_green = 0.0f;
    if constexpr (THERMAL) x_green = xg[i];
    float X, Y;
    f3 c;
    if (!star_place<THERMAL>(a, mk3(lo.x, lo.y, lo.z), mk3(lo.w, hi.x, hi.y), x_green, X, Y, c)) return false;
    const float xf = __builtin_floorf(X), yf = __builtin_floorf(Y);
    const int x0 = (int)xf, y0 = (int)yf;                // |X|, |Y| < 1e9: in range
    const float fx = X - xf, fy = Y - yf;
    bool inside = false;
    for (int k = 0; k < 4; k++) {
        int x = x0 + (k & 1);
        const int y = y0 + (k >> 1);
        if (a.wrap) x = x < 0 ? x + a.width : (x >= a.width ? x - a.width : x);
        if (x < 0 || x >= a.width || y < 0 || y >= a.height) continue;
        inside = true;
        const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
        unsigned long long *word = a.acc + ((size_t)y * (size_t)a.width + (size_t)x) * 3;
        star_add(word + 0, c.x * w);
        star_add(word + 1, c.y * w);
        star_add(word + 2, c.z * w);
    }
    return inside;
}

// 1120: star_splat<false> under the frame.  Kernel 1122 (rpt_thermal.hip.h, behind T_f's definition) is star_splat<true>.
__global__ __launch_bounds__(256) void rpt_stars_splat_kernel(const StarArgs a) {
    splat_and_count(a.counts, [&](int i) { return star_splat<false>(a, nullptr, i); });
}

// 1121: one lane per pixel, pixels in memory order (a wave reads 1536 consecutive bytes of the accumulator).  Where a pixel's three sums
// are all zero — nearly everywhere — nothing else is read.  Elsewhere the zeros go back (the accumulator is clean again for the next
// pass: no memset per frame), and where the record is a miss the sums are tonemapped on their own and added to the pixel's R, G, B bytes,
// saturating.  Changed pixels are counted as 1100 counts them.
__global__ __launch_bounds__(256) void rpt_stars_resolve_kernel(const StarResolveArgs a) {
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
            const int object = *reinterpret_cast<const int *>(a.events + p);
            if (object < 0) {
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
    }
    const unsigned long long set = __ballot(changed);
    if ((t & 63) == 0 && set) atomicAdd(&block_changed, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && block_changed) atomicAdd(a.counts + 1, (unsigned long long)block_changed);
}

}  // namespace rptd
