/*
 * particles_oracle.c — the particle pass (rpt_set_particles / rpt_render_particles) restated in C from DESIGN.md §20, rules 1-6, on the
 * CPU oracle's own helpers (oracle/rpt_oracle.c, included unchanged: oracle_atan2f, oracle_asinf, transformPoint4D, hable, to_u8) and
 * doppler_colour.h's S_f.  TEST INFRASTRUCTURE ONLY; float32, source order, built with -ffp-contract=off.
 *
 * rpt_particles_oracle_place: rules 1-4 per particle -> {visible, X, Y, dist, r, g, b, D, te, rest-frame r}.
 * rpt_particles_oracle_pass:  rules 1-6 on a framebuffer (16 B per pixel, in place) and its event records (32 B per pixel, read only);
 *                             counts[0] = particles seen, counts[1] = pixels whose bytes changed.
 * The set is the 32-byte rpt_particle records; objects the 320-byte Object[] the frames were rendered with (re-based under an
 * orientation); windows {t0, t1} per object, or NULL.
 */
#include "../../oracle/rpt_oracle.c"
#include "doppler_colour.h"

#define PARTICLES_PI_D 3.14159265358979323846264338327950288

typedef struct {
    int width, height, interval;
    int doppler;                    /* RPT_DOPPLER_* as set on the context (the rules switch them off with interval 0) */
    int camera;                     /* 0: the pinhole (lens_scale 1.0f) or the lens; 1: equirect */
    int inverse_square;             /* RPT_PARTICLES_INVERSE_SQUARE */
    float depth_bias;
    float lens_scale;               /* s = (float)tan(v_fov / 2) */
    float h_fov, v_fov, yaw;        /* equirect */
    float white_point[3];
} ParticlesView;

typedef struct { int visible; float X, Y, dist, D, te, r; f3 c; } PlacedParticle;

/* in(W, t) of DESIGN.md "Time windows" */
static int particles_window_in(const float *windows, int i, float t) {
    return !(t < windows[2 * i]) && !(t >= windows[2 * i + 1]);
}

/* rules 1-4 */
static PlacedParticle particles_place(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows, const rpt_particle *p) {
    PlacedParticle o;
    memset(&o, 0, sizeof o);
    o.D = 1.0f;
    if (p->object < 0 || p->object >= object_count) return o;
    const rpt_object *L = objects + p->object;
    /* rule 1 */
    const f3 w = F3(p->pos[0] - L->stationaryCam.y, p->pos[1] - L->stationaryCam.z, p->pos[2] - L->stationaryCam.w);
    const float r = sqrtf(dot3(w, w));
    o.r = r;
    if (!(r > 0.0f) || !(r <= 3.402823466e38f)) return o;
    float tau = -r;
    if (v->interval == 0) {
        const rpt_float4 I0 = L->InvLorentz[0];
        tau = -(I0.y * w.x + I0.z * w.y + I0.w * w.z) / I0.x;
    }
    /* rule 2 */
    const f4 k = transformPoint4D(L->InvLorentz, F4(tau, w.x, w.y, w.z));
    const f3 s = yzw(k);
    const float dist = sqrtf(dot3(s, s));
    o.dist = dist;
    if (!(dist > 0.0f) || !(dist <= 3.402823466e38f)) return o;
    const f3 n = divs3(s, dist);
    o.te = L->stationaryCam.x + tau;
    if (windows && !particles_window_in(windows, p->object, o.te)) return o;
    /* rule 3 */
    const f3 rgb = F3(p->rgb[0], p->rgb[1], p->rgb[2]);
    o.c = rgb;
    if (v->doppler != 0 && v->interval != 0) {
        const float D = dist / r;
        o.D = D;
        if (!(D > 0.0f) || !(D <= 3.402823466e38f)) return o;
        o.c = env_doppler(v->doppler, D, rgb);
        if (v->doppler & 2) o.c = divs3(o.c, D * D);
    }
    if (v->inverse_square) o.c = divs3(o.c, r * r);
    /* rule 4: §19's */
    const float W = (float)v->width, H = (float)v->height;
    if (v->camera == 1) {
        const float pi = (float)PARTICLES_PI_D, two_pi = (float)(2.0 * PARTICLES_PI_D);
        float lambda = oracle_atan2f(n.x, n.z) - v->yaw;
        lambda = lambda - two_pi * floorf((lambda + pi) / two_pi);
        const float ny = n.y < -1.0f ? -1.0f : (n.y > 1.0f ? 1.0f : n.y);
        const float phi = oracle_asinf(ny);
        o.X = W * (lambda / v->h_fov + 0.5f) - 0.5f;
        o.Y = H * (phi / v->v_fov + 0.5f) - 0.5f;
    } else {
        if (!(n.z > 0.0f)) return o;
        const float plane_x = v->lens_scale * (W / H), plane_y = v->lens_scale;
        o.X = W * (0.5f + ((0.5f * n.x) / n.z) / plane_x);
        o.Y = H * (0.5f + ((0.5f * n.y) / n.z) / plane_y);
    }
    o.visible = fabsf(o.X) < 1e9f && fabsf(o.Y) < 1e9f;
    return o;
}

int rpt_particles_oracle_place(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                               const rpt_particle *particles, int n, float *out10) {
    if (!v || !objects || !particles || !out10) return -1;
    for (int i = 0; i < n; i++) {
        const PlacedParticle p = particles_place(v, objects, object_count, windows_or_null, particles + i);
        float *o = out10 + 10 * (size_t)i;
        o[0] = (float)p.visible; o[1] = p.X; o[2] = p.Y; o[3] = p.dist; o[4] = p.c.x; o[5] = p.c.y; o[6] = p.c.z; o[7] = p.D;
        o[8] = p.te; o[9] = p.r;
    }
    return 0;
}

/* rule 5, one channel of one tap */
static void particles_add(uint64_t *word, float p) {
    if (!(p > 0.0f)) return;
    if (p > 65536.0f) p = 65536.0f;
    *word += (uint64_t)(p * 16777216.0f);
}

int rpt_particles_oracle_pass(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                              const rpt_particle *particles, int n, uint8_t *pixels16, const uint8_t *events32, uint64_t *counts) {
    if (!v || !objects || !particles || !pixels16 || !events32 || !counts || v->width < 1 || v->height < 1) return -1;
    const int W = v->width, H = v->height;
    const int wrap = v->camera == 1 && v->h_fov == (float)(2.0 * PARTICLES_PI_D);
    uint64_t *acc = (uint64_t *)calloc((size_t)W * (size_t)H * 3, sizeof(uint64_t));
    if (!acc) return -1;
    counts[0] = counts[1] = 0;
    for (int i = 0; i < n; i++) {
        const PlacedParticle p = particles_place(v, objects, object_count, windows_or_null, particles + i);
        if (!p.visible) continue;
        const float xf = floorf(p.X), yf = floorf(p.Y);
        const int x0 = (int)xf, y0 = (int)yf;
        const float fx = p.X - xf, fy = p.Y - yf;
        const float depth = p.dist - v->depth_bias;
        int seen = 0;
        for (int k = 0; k < 4; k++) {
            int x = x0 + (k & 1);
            const int y = y0 + (k >> 1);
            if (wrap) x = x < 0 ? x + W : (x >= W ? x - W : x);
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            const size_t id = (size_t)y * (size_t)W + (size_t)x;
            int32_t object;
            float record_dist;
            memcpy(&object, events32 + 32 * id, sizeof object);
            memcpy(&record_dist, events32 + 32 * id + 4, sizeof record_dist);
            if (!(object < 0 || depth < record_dist)) continue;
            seen = 1;
            const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
            uint64_t *word = acc + id * 3;
            particles_add(word + 0, p.c.x * w);
            particles_add(word + 1, p.c.y * w);
            particles_add(word + 2, p.c.z * w);
        }
        counts[0] += (uint64_t)seen;
    }
    /* rule 6: every pixel with a non-zero sum, hit or miss */
    const f3 wp = hable(F3(v->white_point[0], v->white_point[1], v->white_point[2]));
    const float hwp[3] = {wp.x, wp.y, wp.z};
    for (size_t id = 0; id < (size_t)W * (size_t)H; id++) {
        const uint64_t *sum = acc + 3 * id;
        if ((sum[0] | sum[1] | sum[2]) == 0) continue;
        uint8_t *rgba = pixels16 + 16 * id + 8;
        int changed = 0;
        for (int k = 0; k < 3; k++) {
            const float S = (float)sum[k] * (1.0f / 16777216.0f);
            const f3 h = hable(F3(S, S, S));
            const unsigned add = to_u8(cl_min(h.x / hwp[k], 1.0f));
            const unsigned byte = (unsigned)rgba[k] + add;
            const uint8_t now = (uint8_t)(byte > 255u ? 255u : byte);
            changed |= now != rgba[k];
            rgba[k] = now;
        }
        counts[1] += (uint64_t)changed;
    }
    free(acc);
    return 0;
}
