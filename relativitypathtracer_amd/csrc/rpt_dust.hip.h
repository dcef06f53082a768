// rpt_dust.hip.h — lit particles (rpt_set_particle_lighting; not in the reference): dust.  A particle's rgb is an albedo and
// its colour at rest is what it scatters from the scene's lights: trace()'s light loop with the normal taken out, light delay on the
// light -> grain leg as on the grain -> camera leg, the light's Doppler factor, its time window and, optionally, the renderer's own shadow
// ray (sample_light_occluded).  Kernels 1134 (lit), 1135 (lit + shadowed) and 1136 (lit + shadowed, time windows) keep 1130's shape —
// 256 lanes, one lane per particle, particle_place as it stands, the taps tested, THEN the light loop for the particles that have a tap
// to add to, then 1130's atomic adds; kernel 1131 resolves.  Included last by rpt_api.hip: every kernel before it keeps its place and
// its code.  tests/native/dust_oracle.c restates rules D0-D7 in C.
#pragma once

#include "rpt_particles.hip.h"

#pragma clang fp contract(off)

namespace rptd {

struct DustArgs {
    ParticleArgs p;                     // as the plain pass fills it; p.counts has four words: seen, changed pixels, pairs lit, pairs shadowed
    float ambient;                      // rpt_set_params
    int add_ambient;                    // RPT_PARTICLES_AMBIENT
};

struct DustNoShadow {};                 // 1134: no KernelArgs, no shadow ray

// Rules D1-D6 for one particle of object L whose event lies tau before the camera event: the colour at rest it scatters.
// SHADOW: DustNoShadow, or the policy sample_light_occluded is instantiated with (k is then the scene, as probe_kernel_args fills it).
// Every index followed here is i < object_count into Object[] and DObj[]; the shadow ray follows what the colour kernels' shadow rays
// follow, validated at upload.
template <class SHADOW>
RPT_DEV f3 dust_scattered(const DustArgs &a, const KernelArgs *k, const rpt_object *L, const rpt_float4 *inv, f4 cam, float tau, f3 pos, f3 rgb,
                          unsigned int &lit, unsigned int &shadowed) {
    const float interval = (float)a.p.interval;
    const f4 hitPos = transformPoint4D(inv, mk4(cam.x + tau, pos.x, pos.y, pos.z));                 // D1
    f3 sum = a.add_ambient ? rgb * a.ambient : mk3(0.0f, 0.0f, 0.0f);                               // D2
    for (int i = 0; i < a.p.object_count; i++) {
        const rpt_object &lo = a.p.objects[i];
        if (!lo.light) continue;
        const f4 P = transformPoint4D(lo.Lorentz, hitPos);
        const f3 d3 = mk3(lo.M[0].w, lo.M[1].w, lo.M[2].w) - yzw(P);
        const float len = length(d3);
        if (!(len > 0.0f) || !(len <= 3.402823466e38f)) continue;
        const f4 dLF = mk4(interval * len, d3.x, d3.y, d3.z);
        if (a.p.dobjs && !window_accepts(a.p.dobjs[i], P.x + dLF.x)) continue;                      // D3
        const f4 lightDir = transformPoint4D(lo.InvLorentz, dLF);                                   // D4
        const f4 dObj = transformPoint4D(L->Lorentz, lightDir);
        const f3 l3 = yzw(dObj);
        if constexpr (!__is_same(SHADOW, DustNoShadow)) {                                           // D5
            const f3 ld = normalize(yzw(lightDir));
            if (sample_light_occluded<SHADOW>(*k, hitPos, mk4(interval, ld.x, ld.y, ld.z), length(yzw(lightDir)), i)) {
                shadowed++;
                continue;
            }
        }
        const float kf = 1.0f / (1.0f + 0.1f * length(l3) + 0.01f * dot(l3, l3));                   // D6
        f3 col = ld3(lo.color);
        if (a.p.doppler != 0) col = doppler_colour(a.p.doppler, dObj.x / dLF.x, col);
        sum = sum + (rgb * kf) * col;
        lit++;
    }
    return sum;
}

// 1130's body with the colour decided late.  particle_place gives X, Y and dist (its colour, S_f of the albedo, is not used: the compiler
// drops it); the four taps are tested as 1130 tests them, inside the frame after the wrap and BEFORE a record is read; a particle with
// no tap to add to ends there, dark or not — the light loop runs for the seen ones only, which is what the two new counts are defined
// over.  Rule D7 is rule 3 on the scattered colour: r and D are formed again from the same floats by the same operations, so they are
// the floats particle_place held, and its tests on them have passed.  With interval 0 the host launches 1130 instead (rule D0).
template <class SHADOW>
RPT_DEV void dust_splat(const DustArgs &a, const KernelArgs *k) {
    __shared__ unsigned int block_counts[3];         // particles seen, pairs lit, pairs shadowed
    const int t = (int)threadIdx.x;
    if (t < 3) block_counts[t] = 0u;
    __syncthreads();
    const int i = (int)blockIdx.x * 256 + t;
    bool seen = false;
    unsigned int lit = 0u, shadowed = 0u;
    if (i < a.p.count) {
        const float4 *record = reinterpret_cast<const float4 *>(a.p.particles + i);
        const float4 lo = record[0], hi = record[1];     // pos.xyz, object | rgb.rgb, padding
        const int object = __float_as_int(lo.w);
        if (object >= 0 && object < a.p.object_count) {
            const rpt_object *L = a.p.objects + object;
            rpt_float4 inv[4];
            for (int j = 0; j < 4; j++) inv[j] = L->InvLorentz[j];
            const f4 cam = ld4(L->stationaryCam);
            const f3 pos = mk3(lo.x, lo.y, lo.z), rgb = mk3(hi.x, hi.y, hi.z);
            float X, Y, dist;
            f3 unused;
            if (particle_place<false>(a.p, inv, cam, a.p.dobjs ? a.p.dobjs + object : nullptr, pos, rgb, 0.0f, X, Y, dist, unused)) {
                const float xf = __builtin_floorf(X), yf = __builtin_floorf(Y);
                const int x0 = (int)xf, y0 = (int)yf;    // |X|, |Y| < 1e9: in range
                const float fx = X - xf, fy = Y - yf;
                const float depth = dist - a.p.depth_bias;
                unsigned int pass = 0u;                  // bit j: tap j is inside the frame and passes the depth test
                for (int j = 0; j < 4; j++) {
                    int x = x0 + (j & 1);
                    const int y = y0 + (j >> 1);
                    if (a.p.wrap) x = x < 0 ? x + a.p.width : (x >= a.p.width ? x - a.p.width : x);
                    if (x < 0 || x >= a.p.width || y < 0 || y >= a.p.height) continue;
                    const size_t p = (size_t)y * (size_t)a.p.width + (size_t)x;
                    const uint2 head = *reinterpret_cast<const uint2 *>(a.p.events + p);       // object, dist
                    if ((int)head.x < 0 || depth < __uint_as_float(head.y)) pass |= 1u << j;
                }
                seen = pass != 0u;
                if (seen) {
                    const f3 w = pos - yzw(cam);
                    const float r = __builtin_sqrtf(dot(w, w));
                    f3 c = dust_scattered<SHADOW>(a, k, L, inv, cam, -r, pos, rgb, lit, shadowed);
                    if (a.p.doppler != 0) {              // D7: rule 3 on the scattered colour
                        const float D = dist / r;
                        c = doppler_colour(a.p.doppler, D, c);
                        if (a.p.doppler & 2) c = c / (D * D);
                    }
                    if (a.p.inverse_square) c = c / (r * r);
                    for (int j = 0; j < 4; j++) {
                        if (!((pass >> j) & 1u)) continue;
                        int x = x0 + (j & 1);
                        const int y = y0 + (j >> 1);
                        if (a.p.wrap) x = x < 0 ? x + a.p.width : (x >= a.p.width ? x - a.p.width : x);
                        const size_t p = (size_t)y * (size_t)a.p.width + (size_t)x;       // (inside the frame: bit j says so)
                        const float wgt = ((j & 1) ? fx : 1.0f - fx) * ((j >> 1) ? fy : 1.0f - fy);
                        unsigned long long *word = a.p.acc + p * 3;
                        star_add(word + 0, c.x * wgt);
                        star_add(word + 1, c.y * wgt);
                        star_add(word + 2, c.z * wgt);
                    }
                }
            }
        }
    }
    // the three counts.  Particles seen as 1130 counts them: a ballot and a popcount per wave, one LDS add per wave that has any.  The
    // pairs are numbers per lane, not flags: an LDS add by every lane that has any.  Then one global atomic per workgroup and word that
    // has any.  (Every lane comes here, a particle that ended early included: the barrier is the workgroup's.)
    const unsigned long long set = __ballot(seen);
    if ((t & 63) == 0 && set) atomicAdd(&block_counts[0], (unsigned int)__popcll(set));
    if (lit) atomicAdd(&block_counts[1], lit);
    if (shadowed) atomicAdd(&block_counts[2], shadowed);
    __syncthreads();
    if (t < 3 && block_counts[t]) atomicAdd(a.p.counts + (t == 0 ? 0 : t + 1), (unsigned long long)block_counts[t]);
}

// 1134: lit.  Time windows through the dobjs pointer, as 1130 has them.
__global__ __launch_bounds__(256) void rpt_dust_splat_kernel(const DustArgs a) { dust_splat<DustNoShadow>(a, nullptr); }

// 1135: lit + shadowed.  The shadow ray is the un-culled one: the culled forms skip an occluder when a __ballot over the wave says no
// lane can meet it, which is right for any set of lanes but pays only where a wave's rays run alike — a wave of pixels, not of grains.
__global__ __launch_bounds__(256) void rpt_dust_shadowed_splat_kernel(const DustArgs a, const KernelArgs k) { dust_splat<Unculled>(a, &k); }

// 1136: 1135 for a context with time windows: occluders held against theirs (§17 rule 2), lights through a.p.dobjs (rule 3)
__global__ __launch_bounds__(256) void rpt_dust_shadowed_windowed_splat_kernel(const DustArgs a, const KernelArgs k) { dust_splat<Windowed<Unculled>>(a, &k); }

}  // namespace rptd
