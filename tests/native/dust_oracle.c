/*
 * dust_oracle.c — the lit particles (rpt_set_particle_lighting) restated in C from DESIGN.md §23, rules D0-D7, on the particle oracle
 * (tests/native/particles_oracle.c, included unchanged: rules 1-6 of §20, and through it oracle/rpt_oracle.c with its sample_light, its
 * intersectors and transformPoint4D, and doppler_colour.h's S_f).  TEST INFRASTRUCTURE ONLY; float32, source order, built with
 * -ffp-contract=off.
 *
 * window_oracle.c cannot be included next to particles_oracle.c (both include oracle/rpt_oracle.c, which has no guard), so its
 * sample_light_w — the oracle's sample_light with §17 rule 2 — is restated here from that section: dust_sample_light_w.  Without windows
 * the shadow ray is the oracle's own sample_light.
 *
 * rpt_dust_oracle_pass:  rules D0-D7 and §20's rules 5-6 on a framebuffer (16 B per pixel, in place) and its event records (32 B per pixel,
 *                        read only); counts[0] = particles seen, [1] = pixels changed, [2] = (particle, light) pairs lit, [3] = pairs shadowed.
 * rpt_dust_oracle_pairs: D1-D6 for EVERY grain whose r is valid, seen or not, and every object i: per pair 8 floats {state, te, len, k,
 *                        di, contribution r, g, b} with state 0 = no light, 1 = lit, 2 = skipped for len, 3 = outside the light's window,
 *                        4 = shadowed, -1 = the grain has no event; per pair a 64-bit mask of ALL occluders below lightDist (objects 0 .. 63;
 *                        SHADOWED only); per grain c_rest (3 floats).
 */
#include "particles_oracle.c"

#define DUST_LIT 1
#define DUST_SHADOWED 2
#define DUST_AMBIENT 4

static int dust_window_in(const float *windows, int i, float t) {
    if (!windows) return 1;
    return !(t < windows[2 * i]) && !(t >= windows[2 * i + 1]);
}

/* opencl_kernel.cl:488-545 + §17 rule 2: the first occluder's index or -1.  mask != NULL: no early return, every occluder is collected */
static int dust_sample_light_w(const Scene *s, const float *windows, const Ray4D *ray, float lightDist, const int lightIndex, uint64_t *mask) {
    float inf = 1e20f;
    const int interval = s->interval;
    int first = -1;
    for (int i = 0; i < s->object_count; i++) {
        if (i != lightIndex) {
            Hit newHit;
            newHit.dist = inf;
            Ray4D newRay;
            f4 newEvent0 = transformPoint4D(s->objects[i].Lorentz, ray->origin);
            f3 nd = normalize3(yzw(ray->dir));
            f4 lightDir = F4((float)interval, nd.x, nd.y, nd.z);
            lightDir = transformPoint4D(s->objects[i].Lorentz, lightDir);
            newRay.origin = newEvent0;
            newRay.dir = lightDir;

            int got = 0;
            switch (s->objects[i].type) {
            case RPT_SPHERE: got = intersect_sphere(s, i, &newRay, &newHit); break;
            case RPT_CUBE:   got = intersect_cube(s, i, &newRay, &newHit); break;
            case RPT_MESH:   got = intersect_octree(s, i, &newRay, &newHit); break;
            }
            if (got) {
                if (newHit.dist < lightDist) {
                    const float ts = newEvent0.x + lightDir.x * newHit.dist;
                    if (dust_window_in(windows, i, ts)) {
                        if (!mask) return i;
                        if (first < 0) first = i;
                        if (i < 64) *mask |= 1ull << i;
                    }
                }
            }
        }
    }
    return first;
}

/* D1-D6 for one grain of object L whose event is at the rest-frame time te: the colour at rest it scatters.  counts: [0] += pairs lit,
 * [1] += pairs shadowed.  pairs (8 floats per object), masks (one per object): optional detail */
static f3 dust_scattered(const Scene *s, int doppler, int lighting, float ambient, const float *windows, const rpt_particle *p, float te,
                         uint64_t *counts, float *pairs, uint64_t *masks) {
    const rpt_object *L = s->objects + p->object;
    const int interval = s->interval;
    const f3 rgb = F3(p->rgb[0], p->rgb[1], p->rgb[2]);
    /* D1 */
    const f4 hitPos = transformPoint4D(L->InvLorentz, F4(te, p->pos[0], p->pos[1], p->pos[2]));
    /* D2 */
    f3 sum = (lighting & DUST_AMBIENT) ? muls3(rgb, ambient) : F3(0.0f, 0.0f, 0.0f);
    for (int i = 0; i < s->object_count; i++) {
        float *o = pairs ? pairs + 8 * (size_t)i : NULL;
        if (o) memset(o, 0, 8 * sizeof(float));
        if (masks) masks[i] = 0;
        if (!s->objects[i].light) continue;
        const rpt_object *lo = s->objects + i;
        const f4 P = transformPoint4D(lo->Lorentz, hitPos);
        const f3 d3 = sub3(F3(lo->M[0].w, lo->M[1].w, lo->M[2].w), yzw(P));
        const float len = length3(d3);
        if (o) { o[0] = 2.0f; o[2] = len; }
        if (!(len > 0.0f) || !(len <= 3.402823466e38f)) continue;
        const f4 dLF = F4(interval * len, d3.x, d3.y, d3.z);
        /* D3 */
        if (o) { o[0] = 3.0f; o[1] = P.x + dLF.x; }
        if (windows && !dust_window_in(windows, i, P.x + dLF.x)) continue;
        /* D4 */
        const f4 lightDir = transformPoint4D(lo->InvLorentz, dLF);
        const f4 dObj = transformPoint4D(L->Lorentz, lightDir);
        const f3 l3 = yzw(dObj);
        /* D6's numbers (before D5, for the detail: a shadowed pair reports them too) */
        const float k = 1.0f / (1.0f + 0.1f * length3(l3) + 0.01f * dot3(l3, l3));
        const float di = dObj.x / dLF.x;
        if (o) { o[3] = k; o[4] = di; }
        /* D5 */
        if (lighting & DUST_SHADOWED) {
            Ray4D ray;
            const f3 ld = normalize3(yzw(lightDir));
            ray.dir = F4((float)interval, ld.x, ld.y, ld.z);
            ray.origin = hitPos;
            const float lightDist = length3(yzw(lightDir));
            int occluder;
            if (masks) occluder = dust_sample_light_w(s, windows, &ray, lightDist, i, masks + i);
            else occluder = windows ? dust_sample_light_w(s, windows, &ray, lightDist, i, NULL) : sample_light(s, &ray, lightDist, i);
            if (occluder != -1) {
                if (o) o[0] = 4.0f;
                counts[1]++;
                continue;
            }
        }
        /* D6 */
        f3 col = xyz(lo->color);
        if (doppler != 0) col = env_doppler(doppler, di, col);
        const f3 contribution = mul3(muls3(rgb, k), col);
        sum = add3(sum, contribution);
        counts[0]++;
        if (o) { o[0] = 1.0f; o[5] = contribution.x; o[6] = contribution.y; o[7] = contribution.z; }
    }
    return sum;
}

/* D7: §20 rule 3 on the colour at rest */
static f3 dust_rule3(const ParticlesView *v, const PlacedParticle *p, f3 c) {
    if (v->doppler != 0 && v->interval != 0) {
        c = env_doppler(v->doppler, p->D, c);
        if (v->doppler & 2) c = divs3(c, p->D * p->D);
    }
    if (v->inverse_square) c = divs3(c, p->r * p->r);
    return c;
}

int rpt_dust_oracle_pass(const rpt_oracle_args *a, const ParticlesView *v, int lighting, const float *windows_or_null,
                         const rpt_particle *particles, int n, uint8_t *pixels16, const uint8_t *events32, uint64_t *counts) {
    if (!a || !v || !particles || !pixels16 || !events32 || !counts || v->width < 1 || v->height < 1 || a->interval != v->interval) return -1;
    counts[2] = counts[3] = 0;
    /* D0: flags 0 and light propagation off are the plain pass */
    if (!(lighting & DUST_LIT) || v->interval == 0)
        return rpt_particles_oracle_pass(v, (const rpt_object *)a->objects, a->object_count, windows_or_null, particles, n, pixels16, events32, counts);
    Scene sc;
    scene_from_args(a, &sc);
    const int W = v->width, H = v->height;
    const int wrap = v->camera == 1 && v->h_fov == (float)(2.0 * PARTICLES_PI_D);
    uint64_t *acc = (uint64_t *)calloc((size_t)W * (size_t)H * 3, sizeof(uint64_t));
    if (!acc) return -1;
    counts[0] = counts[1] = 0;
    for (int i = 0; i < n; i++) {
        const PlacedParticle p = particles_place(v, sc.objects, sc.object_count, windows_or_null, particles + i);
        if (!p.visible) continue;
        const float xf = floorf(p.X), yf = floorf(p.Y);
        const int x0 = (int)xf, y0 = (int)yf;
        const float fx = p.X - xf, fy = p.Y - yf;
        const float depth = p.dist - v->depth_bias;
        size_t ids[4];
        int pass[4], seen = 0;
        for (int k = 0; k < 4; k++) {
            pass[k] = 0;
            int x = x0 + (k & 1);
            const int y = y0 + (k >> 1);
            if (wrap) x = x < 0 ? x + W : (x >= W ? x - W : x);
            if (x < 0 || x >= W || y < 0 || y >= H) continue;
            ids[k] = (size_t)y * (size_t)W + (size_t)x;
            int32_t object;
            float record_dist;
            memcpy(&object, events32 + 32 * ids[k], sizeof object);
            memcpy(&record_dist, events32 + 32 * ids[k] + 4, sizeof record_dist);
            if (!(object < 0 || depth < record_dist)) continue;
            pass[k] = seen = 1;
        }
        if (!seen) continue;        /* the light loop runs for the seen particles only: the two new counts are defined over them */
        counts[0]++;
        const f3 c_rest = dust_scattered(&sc, v->doppler, lighting, a->ambient, windows_or_null, particles + i, p.te, counts + 2, NULL, NULL);
        const f3 c = dust_rule3(v, &p, c_rest);
        for (int k = 0; k < 4; k++) {
            if (!pass[k]) continue;
            const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
            uint64_t *word = acc + ids[k] * 3;
            particles_add(word + 0, c.x * w);
            particles_add(word + 1, c.y * w);
            particles_add(word + 2, c.z * w);
        }
    }
    /* §20 rule 6, unchanged */
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

int rpt_dust_oracle_pairs(const rpt_oracle_args *a, int doppler, int lighting, const float *windows_or_null, const rpt_particle *particles,
                          int n, float *pairs8, uint64_t *masks, float *c_rest3) {
    if (!a || !particles || !pairs8 || !masks || !c_rest3 || a->interval == 0) return -1;
    Scene sc;
    scene_from_args(a, &sc);
    const size_t no = (size_t)sc.object_count;
    for (int i = 0; i < n; i++) {
        const rpt_particle *p = particles + i;
        float *o = pairs8 + 8 * no * (size_t)i;
        for (size_t j = 0; j < 8 * no; j++) o[j] = j % 8 == 0 ? -1.0f : 0.0f;
        memset(masks + no * (size_t)i, 0, no * sizeof(uint64_t));
        c_rest3[3 * i] = c_rest3[3 * i + 1] = c_rest3[3 * i + 2] = 0.0f;
        if (p->object < 0 || (size_t)p->object >= no) continue;
        const rpt_object *L = sc.objects + p->object;
        /* §20 rule 1 */
        const f3 w = F3(p->pos[0] - L->stationaryCam.y, p->pos[1] - L->stationaryCam.z, p->pos[2] - L->stationaryCam.w);
        const float r = sqrtf(dot3(w, w));
        if (!(r > 0.0f) || !(r <= 3.402823466e38f)) continue;
        const float tau = -r;
        uint64_t counts[2] = {0, 0};
        const f3 c = dust_scattered(&sc, doppler, lighting, a->ambient, windows_or_null, p, L->stationaryCam.x + tau, counts, o, masks + no * (size_t)i);
        c_rest3[3 * i] = c.x; c_rest3[3 * i + 1] = c.y; c_rest3[3 * i + 2] = c.z;
    }
    return 0;
}
