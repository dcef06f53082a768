/*
 * doppler_colour.h — the colour operator S_f(D, c) of rpt_set_doppler restated in C from DESIGN.md "Doppler and beaming" (the arithmetic
 * order listed there), not from device code: float32, source order, no contraction.  TEST INFRASTRUCTURE ONLY.  The one C restatement:
 * doppler_oracle.c applies it to the lights and to the summed colour of a ray that hits, environment_oracle.c to the sky.
 * Included after oracle/rpt_oracle.c (f3, F3, muls3).
 */
#ifndef RPT_TESTS_DOPPLER_COLOUR_H
#define RPT_TESTS_DOPPLER_COLOUR_H

/* the emitted spectrum through (K0, 0), (nu_R, r), (1, g), (nu_B, b), (K4, 0) */
static float env_spectrum(float u, f3 c) {
    const float nu_r = (float)(546.1 / 700.0), nu_b = (float)(546.1 / 435.8);
    const float k0 = (float)(2.0 * (546.1 / 700.0) - 1.0), k4 = (float)(2.0 * (546.1 / 435.8) - 1.0);
    if (!(u > k0) || !(u < k4)) return 0.0f;
    float xa, xb, ya, yb;
    if (u < nu_r) { xa = k0; xb = nu_r; ya = 0.0f; yb = c.x; }
    else if (u < 1.0f) { xa = nu_r; xb = 1.0f; ya = c.x; yb = c.y; }
    else if (u < nu_b) { xa = 1.0f; xb = nu_b; ya = c.y; yb = c.z; }
    else { xa = nu_b; xb = k4; ya = c.z; yb = 0.0f; }
    const float t = (u - xa) / (xb - xa);
    return ya * (1.0f - t) + yb * t;
}

static f3 env_doppler(int flags, float D, f3 c) {
    const float nu_r = (float)(546.1 / 700.0), nu_b = (float)(546.1 / 435.8);
    if (D == 1.0f) return c;
    if (flags & 1) {
        f3 o = F3(env_spectrum(nu_r / D, c), env_spectrum(1.0f / D, c), env_spectrum(nu_b / D, c));
        if (flags & 2) o = muls3(o, (D * D) * D);
        return o;
    }
    if (flags & 2) return muls3(c, (D * D) * (D * D));
    return c;
}

#endif
