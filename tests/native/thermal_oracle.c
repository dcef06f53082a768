/*
 * thermal_oracle.c — the thermal point sources (rpt_set_star_temperatures / rpt_set_particle_temperatures) restated in C from DESIGN.md
 * §21: the operator T_f with its exponential and its 1 - e^-z, operation by operation as listed there (not from device code), and both
 * passes' rules with it.  TEST INFRASTRUCTURE ONLY; float32, source order, built with -ffp-contract=off.
 *
 * Built twice (tests/thermal_cases.py): with -DTHERMAL_STARS on top of stars_oracle.c and with -DTHERMAL_PARTICLES on top of
 * particles_oracle.c, both included unmodified.  A pass with temperatures is the plain pass of the same oracle, Doppler switched off,
 * over sources whose colours are already operated: rules 1-2 place each source (the plain oracle's own place function gives D), T_f
 * and the point-source division by D^2 give its colour, and rules 4-6 (and the particles' 1 / r^2) run unchanged.
 *
 * rpt_thermal_oracle_colour:          T_f on n inputs {D, r, g, b, flags as a float, x_G} -> 3 floats each (rpt_probe which = 8's contract).
 * rpt_thermal_oracle_x_green:         T in kelvin -> x_G as the host forms it (double, rounded to float once; 0 for 0).
 * rpt_thermal_oracle_stars_colours /
 * rpt_thermal_oracle_particles_colours: per source {visible by rules 1-3, r, g, b after rule 3, D}.
 * rpt_thermal_oracle_stars_pass /
 * rpt_thermal_oracle_particles_pass:  rules 1-6 with x_G per source (0: the source keeps S_f).
 */
#if defined(THERMAL_STARS)
#include "stars_oracle.c"
#elif defined(THERMAL_PARTICLES)
#include "particles_oracle.c"
#else
#error "build with -DTHERMAL_STARS or -DTHERMAL_PARTICLES"
#endif

static float thermal_exp(float z) {
    if (!(z > -86.0f)) return 0.0f;
    if (z > 88.0f) z = 88.0f;
    const float t = z * (float)1.4426950408889634;
    const int k = (int)(t + (t < 0.0f ? -0.5f : 0.5f));
    const float kf = (float)k;
    const float r = (z - kf * (float)0.693359375) - kf * (float)-2.12194440e-4;
    float p = (float)(1.0 / 5040.0);
    p = p * r + (float)(1.0 / 720.0);
    p = p * r + (float)(1.0 / 120.0);
    p = p * r + (float)(1.0 / 24.0);
    p = p * r + (float)(1.0 / 6.0);
    p = p * r + 0.5f;
    p = p * r + 1.0f;
    p = p * r + 1.0f;
    const int32_t bits = (int32_t)((uint32_t)(k + 127) << 23);
    float scale;
    memcpy(&scale, &bits, sizeof scale);
    return p * scale;
}

static float thermal_one_minus_exp(float z) {
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

static float thermal_ratio(float x, float D) {
    const float y = x / D;
    return (thermal_exp(x - y) * thermal_one_minus_exp(x)) / thermal_one_minus_exp(y);
}

static f3 thermal_colour(int flags, float D, f3 c, float xg) {
    const float nu_r = (float)(546.1 / 700.0), nu_b = (float)(546.1 / 435.8);
    if (xg == 0.0f || !(flags & 1)) return env_doppler(flags, D, c);
    if (D == 1.0f) return c;
    f3 q = F3(thermal_ratio(xg * nu_r, D), thermal_ratio(xg, D), thermal_ratio(xg * nu_b, D));
    if (!(flags & 2)) {
        const float d3 = (D * D) * D;
        q = F3(q.x / d3, q.y / d3, q.z / d3);
    }
    return F3(c.x * q.x, c.y * q.y, c.z * q.z);
}

int rpt_thermal_oracle_colour(const float *in6, int n, float *out3) {
    if (!in6 || !out3) return -1;
    for (int i = 0; i < n; i++) {
        const float *p = in6 + 6 * (size_t)i;
        const f3 o = thermal_colour((int)p[4], p[0], F3(p[1], p[2], p[3]), p[5]);
        out3[3 * (size_t)i + 0] = o.x;
        out3[3 * (size_t)i + 1] = o.y;
        out3[3 * (size_t)i + 2] = o.z;
    }
    return 0;
}

int rpt_thermal_oracle_x_green(const float *kelvin, int n, float *xg) {
    if (!kelvin || !xg) return -1;
    for (int i = 0; i < n; i++) xg[i] = kelvin[i] == 0.0f ? 0.0f : (float)(1.438776877e7 / (546.1 * (double)kelvin[i]));
    return 0;
}

/* rule 3 with T_f: the colour of a source seen at D (the caller has held D against 0 and infinity) */
static f3 thermal_rule3(int doppler, float D, f3 rgb, float xg) {
    f3 c = thermal_colour(doppler, D, rgb, xg);
    if (doppler & 2) {
        const float d2 = D * D;
        c = F3(c.x / d2, c.y / d2, c.z / d2);
    }
    return c;
}

#if defined(THERMAL_STARS)

/* rules 1-3 per star: operated[i] = the star with its colour after rule 3 (its direction untouched); seen[i] = 0 where rule 3 skips it */
static int thermal_stars_operate(const StarsView *v, const float *stars, const float *xg, int n, float *operated, int *seen) {
    rpt_float4 G[4];
    if (rpt_stars_oracle_matrix(v->E, v->interval, &G[0].x)) return -1;
    StarsView plain = *v;
    plain.doppler = 0;
    memcpy(operated, stars, sizeof(float) * 8 * (size_t)n);
    for (int i = 0; i < n; i++) {
        seen[i] = 1;
        if (v->interval == 0 || v->doppler == 0) continue;
        const Placed p = stars_place(&plain, G, stars + 8 * (size_t)i);
        if (!(p.D > 0.0f) || !(p.D <= 3.402823466e38f)) { seen[i] = 0; continue; }
        const f3 c = thermal_rule3(v->doppler, p.D, F3(stars[8 * (size_t)i + 3], stars[8 * (size_t)i + 4], stars[8 * (size_t)i + 5]), xg[i]);
        operated[8 * (size_t)i + 3] = c.x;
        operated[8 * (size_t)i + 4] = c.y;
        operated[8 * (size_t)i + 5] = c.z;
    }
    return 0;
}

int rpt_thermal_oracle_stars_colours(const StarsView *v, const float *stars, const float *xg, int n, float *out5) {
    if (!v || !stars || !xg || !out5) return -1;
    float *operated = (float *)malloc(sizeof(float) * 8 * (size_t)(n > 0 ? n : 1));
    int *seen = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
    float *placed = (float *)malloc(sizeof(float) * 10 * (size_t)(n > 0 ? n : 1));
    StarsView plain = *v;
    plain.doppler = 0;
    int rc = (operated && seen && placed) ? thermal_stars_operate(v, stars, xg, n, operated, seen) : -1;
    if (!rc) rc = rpt_stars_oracle_place(&plain, stars, n, placed);
    for (int i = 0; !rc && i < n; i++) {
        float *o = out5 + 5 * (size_t)i;
        o[0] = (float)(seen[i] && placed[10 * (size_t)i] != 0.0f);
        o[1] = operated[8 * (size_t)i + 3]; o[2] = operated[8 * (size_t)i + 4]; o[3] = operated[8 * (size_t)i + 5];
        o[4] = placed[10 * (size_t)i + 6];
    }
    free(operated); free(seen); free(placed);
    return rc;
}

int rpt_thermal_oracle_stars_pass(const StarsView *v, const float *stars, const float *xg, int n, uint8_t *pixels16, const uint8_t *events32, uint64_t *counts) {
    if (!v || !stars || !xg || n < 0) return -1;
    float *operated = (float *)malloc(sizeof(float) * 8 * (size_t)(n > 0 ? n : 1));
    int *seen = (int *)malloc(sizeof(int) * (size_t)(n > 0 ? n : 1));
    int rc = (operated && seen) ? thermal_stars_operate(v, stars, xg, n, operated, seen) : -1;
    if (!rc) {          /* (a star that rule 3 skips for its D is skipped by the plain pass as well: D does not depend on the flags) */
        StarsView plain = *v;
        plain.doppler = 0;
        rc = rpt_stars_oracle_pass(&plain, operated, n, pixels16, events32, counts);
    }
    free(operated); free(seen);
    return rc;
}

#else

/* rules 1-3 per particle: operated[i] = the particle with its colour after rule 3's Doppler part (1 / r^2 is left to the plain pass);
 * a particle that rule 3 skips for its D gets object -1, which every rule skips */
static void thermal_particles_operate(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows,
                                      const rpt_particle *particles, const float *xg, int n, rpt_particle *operated) {
    ParticlesView geometry = *v;
    geometry.doppler = 2;               /* (the plain place function forms D only under Doppler; its colour is not used) */
    geometry.inverse_square = 0;
    memcpy(operated, particles, sizeof(rpt_particle) * (size_t)n);
    for (int i = 0; i < n; i++) {
        if (v->interval == 0 || v->doppler == 0) continue;
        const PlacedParticle p = particles_place(&geometry, objects, object_count, windows, particles + i);
        if (!(p.r > 0.0f) || !(p.r <= 3.402823466e38f) || !(p.dist > 0.0f) || !(p.dist <= 3.402823466e38f)) continue;    /* skipped anyway */
        if (!(p.D > 0.0f) || !(p.D <= 3.402823466e38f)) { operated[i].object = -1; continue; }
        const f3 c = thermal_rule3(v->doppler, p.D, F3(particles[i].rgb[0], particles[i].rgb[1], particles[i].rgb[2]), xg[i]);
        operated[i].rgb[0] = c.x;
        operated[i].rgb[1] = c.y;
        operated[i].rgb[2] = c.z;
    }
}

int rpt_thermal_oracle_particles_colours(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                                         const rpt_particle *particles, const float *xg, int n, float *out5) {
    if (!v || !objects || !particles || !xg || !out5) return -1;
    rpt_particle *operated = (rpt_particle *)malloc(sizeof(rpt_particle) * (size_t)(n > 0 ? n : 1));
    float *placed = (float *)malloc(sizeof(float) * 10 * (size_t)(n > 0 ? n : 1));
    if (!operated || !placed) { free(operated); free(placed); return -1; }
    thermal_particles_operate(v, objects, object_count, windows_or_null, particles, xg, n, operated);
    ParticlesView plain = *v;
    plain.doppler = 0;
    ParticlesView geometry = *v;
    geometry.doppler = 2;
    int rc = rpt_particles_oracle_place(&plain, objects, object_count, windows_or_null, operated, n, placed);
    for (int i = 0; !rc && i < n; i++) {
        float *o = out5 + 5 * (size_t)i;
        o[0] = placed[10 * (size_t)i];
        o[1] = placed[10 * (size_t)i + 4]; o[2] = placed[10 * (size_t)i + 5]; o[3] = placed[10 * (size_t)i + 6];
        o[4] = particles_place(&geometry, objects, object_count, windows_or_null, particles + i).D;
    }
    free(operated); free(placed);
    return rc;
}

int rpt_thermal_oracle_particles_pass(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                                      const rpt_particle *particles, const float *xg, int n, uint8_t *pixels16, const uint8_t *events32, uint64_t *counts) {
    if (!v || !objects || !particles || !xg || n < 0) return -1;
    rpt_particle *operated = (rpt_particle *)malloc(sizeof(rpt_particle) * (size_t)(n > 0 ? n : 1));
    if (!operated) return -1;
    thermal_particles_operate(v, objects, object_count, windows_or_null, particles, xg, n, operated);
    ParticlesView plain = *v;
    plain.doppler = 0;
    const int rc = rpt_particles_oracle_pass(&plain, objects, object_count, windows_or_null, operated, n, pixels16, events32, counts);
    free(operated);
    return rc;
}

#endif
