/*
 * rockets_oracle.c — the rocket pass (rpt_set_rockets / rpt_render_rockets) restated in C from DESIGN.md §25, rules 1-7, on the particle
 * oracle's own helpers (particles_oracle.c: ParticlesView, particles_add, and through it oracle/rpt_oracle.c and doppler_colour.h's S_f)
 * and thermal_oracle.c's T_f, both included unmodified.  TEST INFRASTRUCTURE ONLY; float32, source order, built with -ffp-contract=off.
 *
 * rpt_rockets_oracle_place: rules 1-6 per record -> {visible, X, Y, dist, r, g, b, D, te, r', n, tau, Aq, z, d, branch}; branch: 0 the
 *                           root where n > 0, 1 the root where n <= 0 and Aq < 0, 2 no root (Aq >= 0), 3 a root with d <= 0, -1 skipped
 *                           before rule 5 (or the slice).
 * rpt_rockets_oracle_pass:  rules 1-7 on a framebuffer (16 B per pixel, in place) and its event records (32 B per pixel, read only);
 *                           counts[0] = records seen, counts[1] = pixels whose bytes changed.
 * The set is the 64-byte rpt_rocket records; objects the 320-byte Object[] the frames were rendered with (re-based under an
 * orientation); xg one float per record (x_G, 0: the record keeps S_f), or NULL: no temperatures.
 */
#define THERMAL_PARTICLES
#include "thermal_oracle.c"

typedef struct { int visible, branch; float X, Y, dist, D, te, r, n, tau, Aq, z, d; f3 c; } PlacedRocket;

/* rules 1-6 */
static PlacedRocket rockets_place(const ParticlesView *v, const rpt_object *objects, int object_count, const rpt_rocket *p, const float *xg_or_null) {
    PlacedRocket o;
    memset(&o, 0, sizeof o);
    o.D = 1.0f;
    o.branch = -1;
    if (p->object < 0 || p->object >= object_count) return o;
    const rpt_object *L = objects + p->object;
    const rpt_float4 cam = L->stationaryCam;
    const f3 pos = F3(p->pos[0], p->pos[1], p->pos[2]), u = F3(p->u[0], p->u[1], p->u[2]), acc = F3(p->acc[0], p->acc[1], p->acc[2]);
    /* rule 1 */
    const float al2 = dot3(acc, acc);
    const float g = sqrtf(1.0f + dot3(u, u));
    const float a0 = dot3(u, acc);
    const f3 av = add3(acc, muls3(u, a0 / (g + 1.0f)));
    /* rule 3 */
    const float T = cam.x;
    const float G = sqrtf((g * g + (2.0f * a0) * T) + (al2 * T) * T);
    const float gG = g + G;
    const float D0 = g * gG + a0 * T;
    if (!(D0 > 0.0f)) return o;
    const float S0 = (T * gG) / D0;
    const float C0 = (T * T) / D0;
    const float ch0 = 1.0f + al2 * C0;
    const float sh0 = al2 * S0;
    const f3 q = add3(add3(pos, muls3(u, S0)), muls3(av, C0));
    const f3 u1 = add3(muls3(u, ch0), muls3(av, S0));
    const float a01 = g * sh0 + a0 * ch0;
    const f3 a1 = add3(muls3(u, sh0), muls3(av, ch0));
    /* rule 4 */
    const f3 w0 = sub3(q, F3(cam.y, cam.z, cam.w));
    const float ww = dot3(w0, w0);
    const float n1 = dot3(u1, w0);
    const float m = dot3(a1, w0);
    const float Aq = (m - 1.0f) - (ww * al2) * 0.25f;
    const float rp = sqrtf(n1 * n1 - Aq * ww);
    o.r = rp;
    o.n = n1;
    o.Aq = Aq;
    if (!(rp > 0.0f) || !(rp <= 3.402823466e38f)) return o;
    /* rule 5 */
    float z;
    if (v->interval == 0) {
        const rpt_float4 I0 = L->InvLorentz[0];
        const float P = I0.y * w0.x + I0.z * w0.y + I0.w * w0.z;
        const float Q = I0.x * G + (I0.y * u1.x + I0.z * u1.y + I0.w * u1.z);
        const float R = I0.x * a01 + (I0.y * a1.x + I0.z * a1.y + I0.w * a1.z);
        const float As = 0.5f * R - (P * al2) * 0.25f;
        z = -((2.0f * P) / (Q + sqrtf(Q * Q - (4.0f * As) * P)));
    } else if (n1 > 0.0f) {
        o.branch = 0;
        z = -(ww / (n1 + rp));
    } else if (Aq < 0.0f) {
        o.branch = 1;
        z = (rp - n1) / Aq;
    } else {
        o.branch = 2;
        return o;
    }
    const float d = 1.0f - ((al2 * z) * z) * 0.25f;
    o.z = z;
    o.d = d;
    if (!(d > 0.0f)) {
        if (v->interval != 0) o.branch = 3;
        return o;
    }
    /* rule 6 */
    const float S = z / d;
    const float C = (z * S) * 0.5f;
    const float tau = G * S + a01 * C;
    o.tau = tau;
    const f3 w = add3(add3(w0, muls3(u1, S)), muls3(a1, C));
    o.te = cam.x + tau;
    if (o.te < p->t0 || o.te >= p->t1) return o;
    const f4 k = transformPoint4D(L->InvLorentz, F4(tau, w.x, w.y, w.z));
    const f3 s = yzw(k);
    const float dist = sqrtf(dot3(s, s));
    o.dist = dist;
    if (!(dist > 0.0f) || !(dist <= 3.402823466e38f)) return o;
    const f3 n = divs3(s, dist);
    const f3 rgb = F3(p->rgb[0], p->rgb[1], p->rgb[2]);
    o.c = rgb;
    if (v->doppler != 0 && v->interval != 0) {
        const float D = dist / rp;
        o.D = D;
        if (!(D > 0.0f) || !(D <= 3.402823466e38f)) return o;
        o.c = xg_or_null ? thermal_colour(v->doppler, D, rgb, *xg_or_null) : env_doppler(v->doppler, D, rgb);
        if (v->doppler & 2) o.c = divs3(o.c, D * D);
    }
    if (v->inverse_square) o.c = divs3(o.c, rp * rp);
    /* rule 7's projection: §19 rule 4 */
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

int rpt_rockets_oracle_place(const ParticlesView *v, const rpt_object *objects, int object_count, const rpt_rocket *records, const float *xg_or_null, int n,
                             float *out16) {
    if (!v || !objects || !records || !out16) return -1;
    for (int i = 0; i < n; i++) {
        const PlacedRocket p = rockets_place(v, objects, object_count, records + i, xg_or_null ? xg_or_null + i : NULL);
        float *o = out16 + 16 * (size_t)i;
        o[0] = (float)p.visible; o[1] = p.X; o[2] = p.Y; o[3] = p.dist; o[4] = p.c.x; o[5] = p.c.y; o[6] = p.c.z; o[7] = p.D;
        o[8] = p.te; o[9] = p.r; o[10] = p.n; o[11] = p.tau; o[12] = p.Aq; o[13] = p.z; o[14] = p.d; o[15] = (float)p.branch;
    }
    return 0;
}

int rpt_rockets_oracle_pass(const ParticlesView *v, const rpt_object *objects, int object_count, const rpt_rocket *records, const float *xg_or_null, int n,
                            uint8_t *pixels16, const uint8_t *events32, uint64_t *counts) {
    if (!v || !objects || !records || !pixels16 || !events32 || !counts || v->width < 1 || v->height < 1) return -1;
    const int W = v->width, H = v->height;
    const int wrap = v->camera == 1 && v->h_fov == (float)(2.0 * PARTICLES_PI_D);
    uint64_t *acc = (uint64_t *)calloc((size_t)W * (size_t)H * 3, sizeof(uint64_t));
    if (!acc) return -1;
    counts[0] = counts[1] = 0;
    for (int i = 0; i < n; i++) {
        const PlacedRocket p = rockets_place(v, objects, object_count, records + i, xg_or_null ? xg_or_null + i : NULL);
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
    /* the resolve: §20 rule 6, every pixel with a non-zero sum, hit or miss */
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
