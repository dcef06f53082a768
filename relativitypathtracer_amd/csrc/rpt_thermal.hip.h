// rpt_thermal.hip.h — thermal point sources (rpt_set_star_temperatures / rpt_set_particle_temperatures; not in the reference; DESIGN.md
// §21): a star or a particle with a temperature is a blackbody, and a blackbody shifted by D is a blackbody at D T, so its three samples
// follow Planck's law instead of S_f's piecewise-linear spectrum, which is zero beyond its outer knots.  The operator T_f, its exponential
// and its 1 - e^-z (only + - * /, compares and integer bit operations: no libm, no ocml, contraction off; tests/thermal_cases.py
// restates them in numpy float32 and rpt_probe which = 8 must match that restatement bit for bit), the probe's kernel, and kernels 1122
// and 1132: the lanes of 1120 and 1130 (star_splat, rpt_stars.hip.h; point_splat, rpt_particles.hip.h) around star_place<true> and
// particle_place<true>, the place functions' thermal instantiations, with one more kernel argument, x_G per source.
#pragma once

#include "rpt_particles.hip.h"

#pragma clang fp contract(off)

namespace rptd {

#define RPT_THERMAL_LOG2E ((float)1.4426950408889634)
#define RPT_THERMAL_LN2_HI ((float)0.693359375)             /* 355 / 512: k * LN2_HI is exact for |k| < 2^15 */
#define RPT_THERMAL_LN2_LO ((float)-2.12194440e-4)          /* ln 2 - LN2_HI */

// e^z.  0 for z <= -86 (and for a NaN): every result is a normal float.  z above 88 is taken as 88.  k = round(z log2 e), r = z - k ln 2
// in two steps (|r| <= 0.347 + a rounding), the Taylor polynomial of degree 7 in Horner's form, 2^k through the exponent field.
RPT_DEV float thermal_exp(float z) {
    if (!(z > -86.0f)) return 0.0f;
    if (z > 88.0f) z = 88.0f;
    const float t = z * RPT_THERMAL_LOG2E;
    const int k = (int)(t + (t < 0.0f ? -0.5f : 0.5f));
    const float kf = (float)k;
    const float r = (z - kf * RPT_THERMAL_LN2_HI) - kf * RPT_THERMAL_LN2_LO;
    float p = (float)(1.0 / 5040.0);
    p = p * r + (float)(1.0 / 720.0);
    p = p * r + (float)(1.0 / 120.0);
    p = p * r + (float)(1.0 / 24.0);
    p = p * r + (float)(1.0 / 6.0);
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    return p * __int_as_float((k + 127) << 23);
}

// 1 - e^-z for z >= 0.  Above 0.5 from thermal_exp (e^-z < 0.61: no cancellation); up to 0.5 the series z (1 - z/2 + z^2/6 - ... +
// z^8/9!), whose first omitted term is below 5.4e-10 of the sum.
RPT_DEV float thermal_one_minus_exp(float z) {
    if (z > 0.5f) return 1.0f - thermal_exp(-z);
    float p = (float)(1.0 / 362880.0);
    p = (float)(1.0 / 40320.0) - z * p;
    p = (float)(1.0 / 5040.0) - z * p;
    p = (float)(1.0 / 720.0) - z * p;
    p = (float)(1.0 / 120.0) - z * p;
    p = (float)(1.0 / 24.0) - z * p;
    p = (float)(1.0 / 6.0) - z * p;
    p = 0.5f - z * p;
    p = 1.0f - z * p;
    return z * p;
}

// expm1(x) / expm1(x / D) as e^(x - y) (1 - e^-x) / (1 - e^-y), y = x / D: no factor overflows for x <= 66.2 and D <= 1e8
RPT_DEV float thermal_ratio(float x, float D) {
    const float y = x / D;
    return (thermal_exp(x - y) * thermal_one_minus_exp(x)) / thermal_one_minus_exp(y);
}

// T_f(flags, D, c, x_G) — see rpt_stars.hip.h for its declaration.  x_G == 0 (not a thermal source) or no shift: S_f.  D == 1 returns c
// bit for bit.  With the shift, channel k is c_k times the ratio at x_k = x_G nu_k, over D^3 unless beaming is on.
RPT_DEV f3 thermal_colour(int flags, float D, f3 c, float xg) {
    if (xg == 0.0f || !(flags & 1)) return doppler_colour(flags, D, c);
    if (D == 1.0f) return c;
    f3 q = mk3(thermal_ratio(xg * RPT_NU_R, D), thermal_ratio(xg, D), thermal_ratio(xg * RPT_NU_B, D));
    if (!(flags & 2)) {
        const float d3 = (D * D) * D;
        q = q / d3;
    }
    return c * q;
}

// rpt_probe which = 8: T_f on n inputs {D, r, g, b, flags, x_G} -> 3 floats
__global__ __launch_bounds__(256) void rpt_probe_thermal_kernel(const float *in, float *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 6 * (size_t)i;
    const f3 o = thermal_colour((int)p[4], p[0], mk3(p[1], p[2], p[3]), p[5]);
    out[3 * (size_t)i + 0] = o.x;
    out[3 * (size_t)i + 1] = o.y;
    out[3 * (size_t)i + 2] = o.z;
}

// 1122: kernel 1120 with T_f for S_f and one more coalesced load, xg[i] (star_splat, rpt_stars.hip.h); kernel 1121 resolves
__global__ __launch_bounds__(256) void rpt_stars_thermal_splat_kernel(const StarArgs a, const float *xg) {
    splat_and_count(a.counts, [&](int i) { return star_splat<true>(a, xg, i); });
}

// 1132: kernel 1130 with T_f for S_f, xg[count] as 1122 reads it (point_splat, rpt_particles.hip.h); kernel 1131 resolves
__global__ __launch_bounds__(256) void rpt_particles_thermal_splat_kernel(const ParticleArgs a, const float *xg) {
    splat_and_count(a.counts, [&](int i) { return point_splat<ParticleSource, true>(a, xg, i); });
}

}  // namespace rptd
