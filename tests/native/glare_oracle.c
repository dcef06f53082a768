/*
 * glare_oracle.c — the glare stage of the splat passes (rpt_set_glare) restated in C from DESIGN.md §26, rules G2-G6, on top of one of
 * the passes' own restatements, included unchanged.  TEST INFRASTRUCTURE ONLY; built by tests/glare_cases.py, once per pass:
 *   -DGLARE_STARS       thermal_oracle.c over stars_oracle.c            (rpt_stars_oracle_pass, rpt_thermal_oracle_stars_pass)
 *   -DGLARE_SEGMENTS    segments_oracle.c over particles_oracle.c       (rpt_particles_oracle_pass, rpt_segments_oracle_pass)
 *   -DGLARE_DUST        dust_oracle.c over particles_oracle.c           (rpt_dust_oracle_pass)
 *   -DGLARE_BALLISTICS  ballistics_oracle.c over thermal_oracle.c       (rpt_ballistics_oracle_pass, rpt_thermal_oracle_particles_pass)
 *   -DGLARE_ROCKETS     rockets_oracle.c over thermal_oracle.c          (rpt_rockets_oracle_pass)
 *
 * A glared pass is the plain pass up to its accumulator, then the stage.  Those restatements keep the accumulator to themselves: each
 * pass function callocs it first, sums into it, resolves from it without changing it, and frees it.  So the two calls are routed
 * through this file while the restatement is included: after rpt_glare_oracle_arm(words) the first calloc of exactly `words` 64-bit
 * words is remembered, and its free copies the words out first.  The plain pass runs on a scratch copy of the frame (its bytes are
 * thrown away, its first count kept), and rules G2-G6 run here on what was captured.  Nothing of the restatements is changed.
 *
 * The taps and the weights are arguments: the tests take them from rpt_glare_taps through ctypes, and hold that function to float64
 * on its own (tests/test_glare_model.py).
 *
 * rpt_glare_oracle_arm / _captured: see above.
 * rpt_glare_oracle_stage:   rules G2-G5 -> S, 3 words per pixel.
 * rpt_glare_oracle_resolve: rule G6 on a framebuffer (16 B per pixel, in place); *changed = pixels whose bytes changed.
 */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <stdio.h>
#include <pthread.h>

static size_t glare_armed_words;        /* > 0: waiting for the accumulator's calloc */
static void *glare_watched;             /* the accumulator, until it is freed */
static uint64_t *glare_kept;            /* its words as they were when it was freed */
static size_t glare_kept_words;

static void *glare_calloc(size_t n, size_t size) {
    void *p = calloc(n, size);
    if (p && glare_armed_words != 0 && !glare_watched && size == sizeof(uint64_t) && n == glare_armed_words) {
        glare_watched = p;
        glare_armed_words = 0;
    }
    return p;
}

static void glare_free(void *p) {
    if (p && p == glare_watched) {
        memcpy(glare_kept, p, glare_kept_words * sizeof(uint64_t));
        glare_watched = NULL;
    }
    free(p);
}

#define calloc(n, size) glare_calloc(n, size)
#define free(p) glare_free(p)
#if defined(GLARE_STARS)
#define THERMAL_STARS
#include "thermal_oracle.c"
#elif defined(GLARE_SEGMENTS)
#include "segments_oracle.c"
#elif defined(GLARE_DUST)
#include "dust_oracle.c"
#elif defined(GLARE_BALLISTICS)
#include "ballistics_oracle.c"
#elif defined(GLARE_ROCKETS)
#include "rockets_oracle.c"
#else
#error "build with -DGLARE_STARS, -DGLARE_SEGMENTS, -DGLARE_DUST, -DGLARE_BALLISTICS or -DGLARE_ROCKETS"
#endif
#undef calloc
#undef free

#define GLARE_RADIUS_MAX 32
#define GLARE_SOURCE_MAX (1ull << 44)

/* the next pass function's accumulator, `words` = width * height * 3, is kept when the function lets go of it */
int rpt_glare_oracle_arm(size_t words) {
    if (words == 0) return -1;
    free(glare_kept);
    glare_kept = (uint64_t *)malloc(words * sizeof(uint64_t));
    if (!glare_kept) return -1;
    glare_kept_words = words;
    glare_armed_words = words;
    glare_watched = NULL;
    return 0;
}

/* 0 and the words, or -1 when no accumulator of that size was allocated and freed since rpt_glare_oracle_arm */
int rpt_glare_oracle_captured(uint64_t *out, size_t words) {
    if (!out || !glare_kept || words != glare_kept_words || glare_armed_words != 0 || glare_watched) return -1;
    memcpy(out, glare_kept, words * sizeof(uint64_t));
    return 0;
}

/* rules G2-G5.  taps: [layers][65], taps[k][32 + j] = t_k[j]; weights: w_0, w_1 .. w_layers.  events32_or_null: the star pass's mask */
int rpt_glare_oracle_stage(const uint64_t *acc, int W, int H, int wrap, const uint8_t *events32_or_null, int layers, const uint32_t *weights,
                           const uint32_t *taps, const int *radius, uint64_t *S) {
    if (!acc || !S || W < 1 || H < 1 || layers < 1 || layers > 3 || !weights || !taps || !radius) return -1;
    const size_t words = (size_t)W * (size_t)H * 3;
    uint64_t *a = (uint64_t *)malloc(words * sizeof(uint64_t)), *h = (uint64_t *)malloc(words * sizeof(uint64_t));
    if (!a || !h) { free(a); free(h); return -1; }
    /* G2 */
    for (size_t id = 0; id < (size_t)W * (size_t)H; id++) {
        int32_t object = -1;
        if (events32_or_null) memcpy(&object, events32_or_null + 32 * id, sizeof object);
        for (int c = 0; c < 3; c++) {
            const uint64_t word = acc[3 * id + c];
            a[3 * id + c] = object >= 0 ? 0 : (word < GLARE_SOURCE_MAX ? word : GLARE_SOURCE_MAX);
        }
    }
    for (size_t i = 0; i < words; i++) S[i] = (uint64_t)weights[0] * a[i];
    for (int k = 0; k < layers; k++) {
        const int R = radius[k];
        if (R < 0 || R > GLARE_RADIUS_MAX) { free(a); free(h); return -1; }
        const uint32_t *t = taps + 65 * (size_t)k + GLARE_RADIUS_MAX;
        /* G3 */
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                for (int c = 0; c < 3; c++) {
                    uint64_t sum = 0;
                    for (int j = -R; j <= R; j++) {
                        int xx = x + j;
                        if (wrap) xx = ((xx % W) + W) % W;
                        if (xx < 0 || xx >= W) continue;
                        sum += (uint64_t)t[j] * a[((size_t)y * (size_t)W + (size_t)xx) * 3 + (size_t)c];
                    }
                    h[((size_t)y * (size_t)W + (size_t)x) * 3 + (size_t)c] = sum >> 16;
                }
        /* G4, and this layer's term of G5 */
        for (int y = 0; y < H; y++)
            for (int x = 0; x < W; x++)
                for (int c = 0; c < 3; c++) {
                    uint64_t sum = 0;
                    for (int j = -R; j <= R; j++) {
                        const int yy = y + j;
                        if (yy < 0 || yy >= H) continue;
                        sum += (uint64_t)t[j] * h[((size_t)yy * (size_t)W + (size_t)x) * 3 + (size_t)c];
                    }
                    S[((size_t)y * (size_t)W + (size_t)x) * 3 + (size_t)c] += (uint64_t)weights[1 + k] * (sum >> 16);
                }
    }
    for (size_t i = 0; i < words; i++) S[i] >>= 16;
    free(a);
    free(h);
    return 0;
}

/* rule G6 */
int rpt_glare_oracle_resolve(const uint64_t *S, int W, int H, const float *white_point, uint8_t *pixels16, uint64_t *changed_out) {
    if (!S || !white_point || !pixels16 || !changed_out || W < 1 || H < 1) return -1;
    const f3 wp = hable(F3(white_point[0], white_point[1], white_point[2]));
    const float hwp[3] = {wp.x, wp.y, wp.z};
    *changed_out = 0;
    for (size_t id = 0; id < (size_t)W * (size_t)H; id++) {
        const uint64_t *sum = S + 3 * id;
        if ((sum[0] | sum[1] | sum[2]) == 0) continue;
        uint8_t *rgba = pixels16 + 16 * id + 8;
        int changed = 0;
        for (int k = 0; k < 3; k++) {
            const float s = (float)sum[k] * (1.0f / 16777216.0f);
            const f3 hb = hable(F3(s, s, s));
            const unsigned add = to_u8(cl_min(hb.x / hwp[k], 1.0f));
            const unsigned byte = (unsigned)rgba[k] + add;
            const uint8_t now = (uint8_t)(byte > 255u ? 255u : byte);
            changed |= now != rgba[k];
            rgba[k] = now;
        }
        *changed_out += (uint64_t)changed;
    }
    return 0;
}
