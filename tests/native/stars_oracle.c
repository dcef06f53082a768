/*
 * stars_oracle.c — the star-field pass (rpt_set_stars / rpt_render_stars) restated in C from DESIGN.md §19, rules 1-6, on the CPU
 * oracle's own helpers (oracle/rpt_oracle.c, included unchanged: oracle_atan2f, oracle_asinf, transformPoint4D, normalize3, hable,
 * to_u8) and doppler_colour.h's S_f.  TEST INFRASTRUCTURE ONLY; float32, source order, built with -ffp-contract=off.
 *
 * rpt_stars_oracle_matrix: rule 1 — E' (the sky matrix as re-based for the orientation, float) -> G; 0, or -1 when E' cannot be inverted.
 * rpt_stars_oracle_place:  rules 1-4 per star -> {visible, X, Y, r, g, b, D, n.x, n.y, n.z}.
 * rpt_stars_oracle_pass:   rules 1-6 on a framebuffer (16 B per pixel, in place) and its event records (32 B per pixel, read only);
 *                          counts[0] = stars with a tap inside the frame, counts[1] = pixels whose bytes changed.
 * The catalogue is 8 floats per star as the caller gave it (dir of any non-zero length, rgb, two unused): normalised here, in double.
 */
#include "../../oracle/rpt_oracle.c"
#include "doppler_colour.h"

#define STARS_PI_D 3.14159265358979323846264338327950288

typedef struct {
    int width, height, interval;
    int doppler;                    /* RPT_DOPPLER_* as set on the context (the rules switch them off with interval 0) */
    int camera;                     /* 0: the pinhole (lens_scale 1.0f) or the lens; 1: equirect */
    float lens_scale;               /* s = (float)tan(v_fov / 2) */
    float h_fov, v_fov, yaw;        /* equirect */
    float white_point[3];
    float E[16];                    /* E', row-major, t first */
} StarsView;

/* Gauss-Jordan elimination with partial pivoting in double; singular: a pivot <= 1e-12 times the largest entry */
static int stars_invert(const double *a, int n, double *inv) {
    double m[4][8], scale = 0.0;
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) {
            if (!isfinite(a[r * n + c])) return 0;
            m[r][c] = a[r * n + c];
            m[r][n + c] = r == c ? 1.0 : 0.0;
            if (fabs(a[r * n + c]) > scale) scale = fabs(a[r * n + c]);
        }
    for (int col = 0; col < n; col++) {
        int p = col;
        for (int r = col + 1; r < n; r++)
            if (fabs(m[r][col]) > fabs(m[p][col])) p = r;
        if (!(fabs(m[p][col]) > 1e-12 * scale)) return 0;
        if (p != col)
            for (int c = 0; c < 2 * n; c++) { const double t = m[p][c]; m[p][c] = m[col][c]; m[col][c] = t; }
        const double d = m[col][col];
        for (int c = 0; c < 2 * n; c++) m[col][c] /= d;
        for (int r = 0; r < n; r++) {
            if (r == col) continue;
            const double f = m[r][col];
            if (f == 0.0) continue;
            for (int c = 0; c < 2 * n; c++) m[r][c] -= f * m[col][c];
        }
    }
    for (int r = 0; r < n; r++)
        for (int c = 0; c < n; c++) inv[r * n + c] = m[r][n + c];
    return 1;
}

/* rule 1 */
int rpt_stars_oracle_matrix(const float *E, int interval, float *G) {
    double a[16], inv[16];
    if (interval != 0) {
        for (int k = 0; k < 16; k++) a[k] = E[k];
        if (!stars_invert(a, 4, inv)) return -1;
        for (int k = 0; k < 16; k++) G[k] = (float)inv[k];
    } else {
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) a[r * 3 + c] = E[(r + 1) * 4 + (c + 1)];
        if (!stars_invert(a, 3, inv)) return -1;
        for (int k = 0; k < 16; k++) G[k] = (k % 5 == 0) ? 1.0f : 0.0f;
        for (int r = 0; r < 3; r++)
            for (int c = 0; c < 3; c++) G[(r + 1) * 4 + (c + 1)] = (float)inv[r * 3 + c];
    }
    for (int k = 0; k < 16; k++)
        if (!isfinite(G[k])) return -1;
    return 0;
}

typedef struct { int visible; float X, Y, D; f3 c, n; } Placed;

/* rules 2-4 */
static Placed stars_place(const StarsView *v, const rpt_float4 G[4], const float *star) {
    Placed o;
    memset(&o, 0, sizeof o);
    const double x = star[0], y = star[1], z = star[2];
    const double l = sqrt(x * x + y * y + z * z);
    const f3 s = F3((float)(x / l), (float)(y / l), (float)(z / l));
    const f3 rgb = F3(star[3], star[4], star[5]);
    const f4 q = transformPoint4D(G, F4((float)v->interval, s.x, s.y, s.z));
    o.c = rgb;
    o.D = 1.0f;
    if (v->interval != 0) {
        const float D = q.x / (float)v->interval;
        o.D = D;
        if (!(D > 0.0f) || !(D <= 3.402823466e38f)) return o;
        if (v->doppler != 0) o.c = env_doppler(v->doppler, D, rgb);
        if (v->doppler & 2) {
            const float d2 = D * D;
            o.c = F3(o.c.x / d2, o.c.y / d2, o.c.z / d2);
        }
    }
    const f3 n = normalize3(yzw(q));
    o.n = n;
    const float W = (float)v->width, H = (float)v->height;
    if (v->camera == 1) {
        const float pi = (float)STARS_PI_D, two_pi = (float)(2.0 * STARS_PI_D);
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

int rpt_stars_oracle_place(const StarsView *v, const float *stars, int n, float *out10) {
    rpt_float4 G[4];
    if (!v || !stars || !out10 || rpt_stars_oracle_matrix(v->E, v->interval, &G[0].x)) return -1;
    for (int i = 0; i < n; i++) {
        const Placed p = stars_place(v, G, stars + 8 * (size_t)i);
        float *o = out10 + 10 * (size_t)i;
        o[0] = (float)p.visible; o[1] = p.X; o[2] = p.Y; o[3] = p.c.x; o[4] = p.c.y; o[5] = p.c.z; o[6] = p.D;
        o[7] = p.n.x; o[8] = p.n.y; o[9] = p.n.z;
    }
    return 0;
}

/* Where the sky lookup looks for camera direction n: the first three lines of environment_oracle.c's env_sky (DESIGN.md "Environment
 * map"), for the registration test — a star's n must come back as the star's own dir. */
int rpt_stars_oracle_sky_direction(const float *E, int interval, const float *dirs, int n, float *out3) {
    if (!E || !dirs || !out3) return -1;
    rpt_float4 M[4];
    memcpy(M, E, sizeof M);
    for (int i = 0; i < n; i++) {
        const f3 nd = normalize3(F3(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2]));
        const f4 k = transformPoint4D(M, F4((float)interval, nd.x, nd.y, nd.z));
        const f3 d = normalize3(yzw(k));
        out3[3 * (size_t)i] = d.x; out3[3 * (size_t)i + 1] = d.y; out3[3 * (size_t)i + 2] = d.z;
    }
    return 0;
}

/* rule 5, one channel of one tap */
static void stars_add(uint64_t *word, float p) {
    if (!(p > 0.0f)) return;
    if (p > 65536.0f) p = 65536.0f;
    *word += (uint64_t)(p * 16777216.0f);
}

int rpt_stars_oracle_pass(const StarsView *v, const float *stars, int n, uint8_t *pixels16, const uint8_t *events32, uint64_t *counts) {
    rpt_float4 G[4];
    if (!v || !stars || !pixels16 || !events32 || !counts || v->width < 1 || v->height < 1) return -1;
    if (rpt_stars_oracle_matrix(v->E, v->interval, &G[0].x)) return -1;
    const int W = v->width, H = v->height;
    const int wrap = v->camera == 1 && v->h_fov == (float)(2.0 * STARS_PI_D);
    uint64_t *acc = (uint64_t *)calloc((size_t)W * (size_t)H * 3, sizeof(uint64_t));
    if (!acc) return -1;
    counts[0] = counts[1] = 0;
    for (int i = 0; i < n; i++) {
        const Placed p = stars_place(v, G, stars + 8 * (size_t)i);
        if (!p.visible) continue;
        const float xf = floorf(p.X), yf = floorf(p.Y);
        const int x0 = (int)xf, y0 = (int)yf;
        const float fx = p.X - xf, fy = p.Y - yf;
        int inside = 0;
        for (int k = 0; k < 4; k++) {
            int x = x0 + (k & 1);
            const int y = y0 + (k >> 1);
            if (wrap) x = x < 0 ? x + W : (x >= W ? x - W : x);
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            inside = 1;
            const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
            uint64_t *word = acc + ((size_t)y * (size_t)W + (size_t)x) * 3;
            stars_add(word + 0, p.c.x * w);
            stars_add(word + 1, p.c.y * w);
            stars_add(word + 2, p.c.z * w);
        }
        counts[0] += (uint64_t)inside;
    }
    /* rule 6 */
    const f3 wp = hable(F3(v->white_point[0], v->white_point[1], v->white_point[2]));
    const float hwp[3] = {wp.x, wp.y, wp.z};
    for (size_t id = 0; id < (size_t)W * (size_t)H; id++) {
        const uint64_t *sum = acc + 3 * id;
        if ((sum[0] | sum[1] | sum[2]) == 0) continue;
        int32_t object;
        memcpy(&object, events32 + 32 * id, sizeof object);
        if (object >= 0) continue;
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
