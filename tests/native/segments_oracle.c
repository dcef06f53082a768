/*
 * segments_oracle.c — the segment pass (rpt_set_segments / rpt_render_segments) restated in C from DESIGN.md §22, rules S0-S5, on
 * particles_oracle.c (included unchanged: rule S1 IS its particles_place, rule S5 its resolve) and, through it, on the CPU oracle's own
 * helpers.  TEST INFRASTRUCTURE ONLY; float32, source order, built with -ffp-contract=off.
 *
 * rpt_segments_oracle_nodes:  rules S0-S1 per node  -> {visible, X, Y, dist, r, g, b, D, te, rest-frame r, pos.x, pos.y, pos.z}
 * rpt_segments_oracle_pieces: rule S2 per piece     -> {placed, shift of X1, L, m, q}
 * rpt_segments_oracle_pass:   rules S0-S5 on a framebuffer (16 B per pixel, in place) and its event records (32 B per pixel, read only);
 *                             counts[0] = pieces drawn, counts[1] = pixels whose bytes changed; optionally the accumulator as it
 *                             stood before the resolve (3 x uint64 per pixel) and extra[0] = the most adds any one piece made to
 *                             any one word (zero adds, which rule 5 skips, not counted), extra[1] = samples taken; and per piece
 *                             {samples, taps inside the frame, taps that pass the depth test, passing taps over a hit pixel}.
 * The set is the 48-byte rpt_segment records; the view is particles_oracle.c's, its inverse_square and depth_bias the segment options'.
 */
#include "particles_oracle.c"

#define SEGMENT_MAX_STEPS 1024

typedef struct { int placed; float X0, dX, Y0, dY, dist0, ddist, shift, L, q; f3 c0, dc; int m; } SegmentPiece;

/* rule S0: the length of one piece, or a value that fails the test */
static float segments_len(const rpt_segment *s, int P) {
    const f3 d = F3(s->b[0] - s->a[0], s->b[1] - s->a[1], s->b[2] - s->a[2]);
    return sqrtf(dot3(d, d)) / (float)P;
}

static int segments_live(float len) { return len > 0.0f && len <= 3.402823466e38f; }

/* rules S0-S1: node j of a segment as a particle, and its placement */
static PlacedParticle segments_node(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows, const rpt_segment *s,
                                    int P, int j, rpt_particle *as_particle) {
    rpt_particle p;
    memset(&p, 0, sizeof p);
    const float f = (float)j / (float)P;
    for (int k = 0; k < 3; k++) {
        const float d = s->b[k] - s->a[k];
        p.pos[k] = j == P ? s->b[k] : s->a[k] + d * f;
        p.rgb[k] = s->rgb[k];
    }
    p.object = s->object;
    if (as_particle) *as_particle = p;
    return particles_place(v, objects, object_count, windows, &p);
}

/* rule S2 */
static SegmentPiece segments_piece(const ParticlesView *v, float len, const PlacedParticle *n0, const PlacedParticle *n1) {
    SegmentPiece o;
    memset(&o, 0, sizeof o);
    if (!segments_live(len) || !n0->visible || !n1->visible) return o;
    o.placed = 1;
    float X1 = n1->X;
    if (v->camera == 1) {
        const float two_pi = (float)(2.0 * PARTICLES_PI_D);
        const float Px = (float)v->width * (two_pi / v->h_fov);
        if (X1 - n0->X > 0.5f * Px) X1 -= Px;
        if (X1 - n0->X < -0.5f * Px) X1 += Px;
    }
    o.shift = X1 - n1->X;
    o.X0 = n0->X;
    o.dX = X1 - n0->X;
    o.Y0 = n0->Y;
    o.dY = n1->Y - n0->Y;
    o.dist0 = n0->dist;
    o.ddist = n1->dist - n0->dist;
    o.c0 = n0->c;
    o.dc = F3(n1->c.x - n0->c.x, n1->c.y - n0->c.y, n1->c.z - n0->c.z);
    o.L = fmaxf(fabsf(o.dX), fabsf(o.dY));
    if (!(o.L <= (float)SEGMENT_MAX_STEPS)) return o;
    const int m = (int)ceilf(o.L);
    o.m = m < 1 ? 1 : m;
    o.q = len / (float)o.m;
    return o;
}

int rpt_segments_oracle_nodes(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                              const rpt_segment *segments, int n, int pieces, float *out13) {
    if (!v || !objects || !segments || !out13 || pieces < 1) return -1;
    for (int i = 0; i < n; i++)
        for (int j = 0; j <= pieces; j++) {
            rpt_particle q;
            const PlacedParticle p = segments_node(v, objects, object_count, windows_or_null, segments + i, pieces, j, &q);
            float *o = out13 + 13 * ((size_t)i * (size_t)(pieces + 1) + (size_t)j);
            o[0] = (float)p.visible; o[1] = p.X; o[2] = p.Y; o[3] = p.dist; o[4] = p.c.x; o[5] = p.c.y; o[6] = p.c.z; o[7] = p.D;
            o[8] = p.te; o[9] = p.r; o[10] = q.pos[0]; o[11] = q.pos[1]; o[12] = q.pos[2];
        }
    return 0;
}

int rpt_segments_oracle_pieces(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                               const rpt_segment *segments, int n, int pieces, float *out5) {
    if (!v || !objects || !segments || !out5 || pieces < 1) return -1;
    for (int i = 0; i < n; i++) {
        const float len = segments_len(segments + i, pieces);
        PlacedParticle n0 = segments_node(v, objects, object_count, windows_or_null, segments + i, pieces, 0, NULL);
        for (int j = 0; j < pieces; j++) {
            const PlacedParticle n1 = segments_node(v, objects, object_count, windows_or_null, segments + i, pieces, j + 1, NULL);
            const SegmentPiece e = segments_piece(v, len, &n0, &n1);
            float *o = out5 + 5 * ((size_t)i * (size_t)pieces + (size_t)j);
            o[0] = (float)e.placed; o[1] = e.shift; o[2] = e.L; o[3] = (float)e.m; o[4] = e.q;
            n0 = n1;
        }
    }
    return 0;
}

int rpt_segments_oracle_pass(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                             const rpt_segment *segments, int n, int pieces, uint8_t *pixels16, const uint8_t *events32, uint64_t *counts,
                             uint64_t *acc_out_or_null, uint64_t *extra_or_null, uint32_t *piece_taps_or_null) {
    if (!v || !objects || !segments || !pixels16 || !events32 || !counts || v->width < 1 || v->height < 1 || pieces < 1) return -1;
    const int W = v->width, H = v->height;
    const int wrap = v->camera == 1 && v->h_fov == (float)(2.0 * PARTICLES_PI_D);
    const size_t words = (size_t)W * (size_t)H * 3;
    uint64_t *acc = (uint64_t *)calloc(words, sizeof(uint64_t));
    uint32_t *adder = (uint32_t *)calloc(words, sizeof(uint32_t));       /* the piece (1-based) that last added to a word ... */
    uint32_t *adds = (uint32_t *)calloc(words, sizeof(uint32_t));        /* ... and how often it has */
    if (!acc || !adder || !adds) { free(acc); free(adder); free(adds); return -1; }
    counts[0] = counts[1] = 0;
    uint64_t most_adds = 0, samples = 0;
    uint32_t piece_id = 0;
    for (int i = 0; i < n; i++) {
        const float len = segments_len(segments + i, pieces);
        PlacedParticle n0 = segments_node(v, objects, object_count, windows_or_null, segments + i, pieces, 0, NULL);
        for (int j = 0; j < pieces; j++) {
            const PlacedParticle n1 = segments_node(v, objects, object_count, windows_or_null, segments + i, pieces, j + 1, NULL);
            const SegmentPiece e = segments_piece(v, len, &n0, &n1);
            piece_id++;
            int seen = 0;
            uint32_t taps[4] = {(uint32_t)e.m, 0, 0, 0};
            for (int s = 0; s < e.m; s++) {
                /* rule S3 */
                const float u = ((float)s + 0.5f) / (float)e.m;
                const float X = e.X0 + e.dX * u;
                const float Y = e.Y0 + e.dY * u;
                const float dist = e.dist0 + e.ddist * u;
                const float c[3] = {(e.c0.x + e.dc.x * u) * e.q, (e.c0.y + e.dc.y * u) * e.q, (e.c0.z + e.dc.z * u) * e.q};
                samples++;
                /* rule S4 */
                const float xf = floorf(X), yf = floorf(Y);
                const int x0 = (int)xf, y0 = (int)yf;
                const float fx = X - xf, fy = Y - yf;
                const float depth = dist - v->depth_bias;
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
                    taps[1]++;
                    if (!(object < 0 || depth < record_dist)) continue;
                    seen = 1;
                    taps[2]++;
                    taps[3] += object >= 0;
                    const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
                    for (int ch = 0; ch < 3; ch++) {
                        const size_t word = id * 3 + (size_t)ch;
                        const uint64_t before = acc[word];
                        particles_add(acc + word, c[ch] * w);
                        if (acc[word] == before) continue;
                        adds[word] = adder[word] == piece_id ? adds[word] + 1 : 1;
                        adder[word] = piece_id;
                        if (adds[word] > most_adds) most_adds = adds[word];
                    }
                }
            }
            counts[0] += (uint64_t)seen;
            if (piece_taps_or_null) memcpy(piece_taps_or_null + 4 * (size_t)(piece_id - 1), taps, sizeof taps);
            n0 = n1;
        }
    }
    if (acc_out_or_null) memcpy(acc_out_or_null, acc, words * sizeof(uint64_t));
    if (extra_or_null) { extra_or_null[0] = most_adds; extra_or_null[1] = samples; }
    /* rule S5: §20 rule 6 — every pixel with a non-zero sum, hit or miss */
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
    free(adder);
    free(adds);
    return 0;
}

/* §20 rules 1-5 for a particle set, up to the accumulator (3 x uint64 per pixel, overwritten): what the continuum test compares a rod's
 * sums with.  particles_place and particles_add are particles_oracle.c's; the loop is its pass's. */
int rpt_segments_oracle_lamps(const ParticlesView *v, const rpt_object *objects, int object_count, const float *windows_or_null,
                              const rpt_particle *particles, int n, const uint8_t *events32, uint64_t *acc) {
    if (!v || !objects || !particles || !events32 || !acc || v->width < 1 || v->height < 1) return -1;
    const int W = v->width, H = v->height;
    const int wrap = v->camera == 1 && v->h_fov == (float)(2.0 * PARTICLES_PI_D);
    memset(acc, 0, (size_t)W * (size_t)H * 3 * sizeof(uint64_t));
    for (int i = 0; i < n; i++) {
        const PlacedParticle p = particles_place(v, objects, object_count, windows_or_null, particles + i);
        if (!p.visible) continue;
        const float xf = floorf(p.X), yf = floorf(p.Y);
        const int x0 = (int)xf, y0 = (int)yf;
        const float fx = p.X - xf, fy = p.Y - yf;
        const float depth = p.dist - v->depth_bias;
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
            const float w = ((k & 1) ? fx : 1.0f - fx) * ((k >> 1) ? fy : 1.0f - fy);
            particles_add(acc + id * 3 + 0, p.c.x * w);
            particles_add(acc + id * 3 + 1, p.c.y * w);
            particles_add(acc + id * 3 + 2, p.c.z * w);
        }
    }
    return 0;
}
