/*
 * environment_oracle.c — the CPU oracle (oracle/rpt_oracle.c, included unchanged) with the camera ray given per pixel and the sky
 * path of rpt_set_environment restated in C (DESIGN.md "Environment map"), for tests/test_gpu_environment.py.  TEST INFRASTRUCTURE ONLY.
 *
 * rpt_environment_oracle_lookup: n directions {d.x, d.y, d.z} (normalised here) -> {u, v, r, g, b}: what rpt_probe which = 7 returns.
 * rpt_environment_oracle_render: pixel id = y * width + x looks along dirs[3 id .. 3 id + 2] (unnormalised: the pinhole's plane point or
 * the panorama's p); a ray that hits something is the oracle's trace, or with doppler != 0 doppler_oracle.c's trace_doppler (the trace
 * with the light and camera factors); one that hits nothing takes the sky path with Doppler flags `doppler`; then the tonemap, the clamp
 * and the pack of render_pixel.  hit_out[id] = 1 where the ray hit.
 * S_f (doppler_colour.h) is restated from DESIGN.md "Doppler and beaming" (the arithmetic order listed there), not from device code.
 */
#include "doppler_oracle.c"

#define ENV_PI_D 3.14159265358979323846264338327950288

typedef struct { const uint8_t *rgb8; int width, height; } EnvImage;

static f3 env_texel(const EnvImage *e, int x, int y) {
    const uint8_t *t = e->rgb8 + 3 * ((size_t)y * (size_t)e->width + (size_t)x);
    return F3(t[0] / 255.0f, t[1] / 255.0f, t[2] / 255.0f);
}

static f2 env_uv(f3 d) {
    const float dy = d.y < -1.0f ? -1.0f : (d.y > 1.0f ? 1.0f : d.y);
    f2 uv;
    uv.x = (float)(0.5f + oracle_atan2f(d.z, d.x) / (2 * ENV_PI_D));
    uv.y = (float)(oracle_asinf(dy) / ENV_PI_D + 0.5f);
    return uv;
}

/* the four taps of opencl_kernel.cl:427-471 in their order; columns wrap, rows clamp; indices clamped on both sides first */
static f3 env_bilinear(const EnvImage *e, f2 uv) {
    const int width = e->width, height = e->height;
    float u = width * uv.x;
    float v = height * (1.0f - uv.y);
    int x = iclamp(f2i_sat(floorf(u)), 0, width - 1);
    int y = iclamp(f2i_sat(floorf(v)), 0, height - 1);
    float u_ratio = u - x;
    float v_ratio = v - y;
    float u_opp = 1 - u_ratio;
    float v_opp = 1 - v_ratio;
    f3 result = muls3(env_texel(e, x, y), u_opp);
    x = x + 1 >= width ? 0 : x + 1;
    result = add3(result, muls3(env_texel(e, x, y), u_ratio));
    result = muls3(result, v_opp);
    y = iclamp(y + 1, 0, height - 1);
    f3 result2 = muls3(env_texel(e, x, y), u_ratio);
    x = x - 1 < 0 ? width - 1 : x - 1;
    result2 = add3(result2, muls3(env_texel(e, x, y), u_opp));
    result2 = muls3(result2, v_ratio);
    return add3(result, result2);
}

static f3 env_sky(const EnvImage *e, const rpt_float4 E[4], int interval, int doppler, f3 dir) {
    const f3 nd = normalize3(dir);
    const f4 rayDir = F4((float)interval, nd.x, nd.y, nd.z);
    const f4 k = transformPoint4D(E, rayDir);
    const f3 d = normalize3(yzw(k));
    f3 c = env_bilinear(e, env_uv(d));
    if (doppler != 0 && interval != 0) c = env_doppler(doppler, (float)interval / k.x, c);
    return c;
}

int rpt_environment_oracle_lookup(const float *dirs, int n, const uint8_t *rgb8, int width, int height, float *out5) {
    if (!dirs || !rgb8 || !out5 || width < 1 || height < 1) return -1;
    const EnvImage e = {rgb8, width, height};
    for (int i = 0; i < n; i++) {
        const f2 uv = env_uv(normalize3(F3(dirs[3 * (size_t)i], dirs[3 * (size_t)i + 1], dirs[3 * (size_t)i + 2])));
        const f3 c = env_bilinear(&e, uv);
        float *o = out5 + 5 * (size_t)i;
        o[0] = uv.x; o[1] = uv.y; o[2] = c.x; o[3] = c.y; o[4] = c.z;
    }
    return 0;
}

typedef struct {
    const rpt_oracle_args *a;
    const Scene *scene;
    const float *dirs;
    EnvImage env;
    rpt_float4 E[4];
    int doppler;
    uint8_t *hit_out;
    volatile int next_row;
} EnvJob;

static void env_pixel(const EnvJob *job, unsigned int id) {
    const rpt_oracle_args *a = job->a;
    const f3 wp = F3(a->white_point[0], a->white_point[1], a->white_point[2]);
    Ray camray;
    camray.origin = F3(0, 0, 0);
    camray.dir = normalize3(F3(job->dirs[3 * (size_t)id], job->dirs[3 * (size_t)id + 1], job->dirs[3 * (size_t)id + 2]));
    Hit probe;
    const int hit = intersect_scene(job->scene, &camray, &probe);
    f3 finalcolor;
    if (!hit) finalcolor = env_sky(&job->env, job->E, a->interval, job->doppler, camray.dir);
    else if (job->doppler != 0) trace_doppler(job->scene, a->ambient, &camray, job->doppler, NULL, &finalcolor);
    else finalcolor = trace(job->scene, a->ambient, &camray);
    if (job->hit_out) job->hit_out[id] = (uint8_t)hit;
    finalcolor = div3(hable(finalcolor), hable(wp));
    finalcolor = F3(cl_min(finalcolor.x, 1.0f), cl_min(finalcolor.y, 1.0f), cl_min(finalcolor.z, 1.0f));
    if (a->out_rgb) {
        a->out_rgb[3 * (size_t)id + 0] = finalcolor.x;
        a->out_rgb[3 * (size_t)id + 1] = finalcolor.y;
        a->out_rgb[3 * (size_t)id + 2] = finalcolor.z;
    }
    if (a->out_pixels) {
        rpt_pixel *p = &((rpt_pixel *)a->out_pixels)[id];
        p->x = (float)(id % (unsigned int)a->width);
        p->y = (float)(id / (unsigned int)a->width);
        p->rgba[0] = to_u8(finalcolor.x);
        p->rgba[1] = to_u8(finalcolor.y);
        p->rgba[2] = to_u8(finalcolor.z);
        p->rgba[3] = 1;
        p->unspecified = 0;
    }
}

static void *env_worker(void *p) {
    EnvJob *job = (EnvJob *)p;
    for (;;) {
        const int y = __sync_fetch_and_add(&job->next_row, 1);
        if (y >= job->a->height) break;
        for (int x = 0; x < job->a->width; x++) env_pixel(job, (unsigned int)y * (unsigned int)job->a->width + (unsigned int)x);
    }
    return NULL;
}

int rpt_environment_oracle_render(const rpt_oracle_args *a, const float *dirs, const float *E16, const uint8_t *rgb8, int env_width,
                                  int env_height, int doppler, uint8_t *hit_out, int threads) {
    if (!a || !dirs || !E16 || !rgb8 || a->width <= 0 || a->height <= 0 || env_width < 1 || env_height < 1) return -1;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    Scene sc;
    scene_from_args(a, &sc);
    EnvJob job;
    memset(&job, 0, sizeof job);
    job.a = a;
    job.scene = &sc;
    job.dirs = dirs;
    job.env.rgb8 = rgb8; job.env.width = env_width; job.env.height = env_height;
    memcpy(job.E, E16, sizeof job.E);
    job.doppler = doppler;
    job.hit_out = hit_out;
    pthread_t th[64];
    int started = 1;
    while (started < threads && pthread_create(&th[started], NULL, env_worker, &job) == 0) started++;
    env_worker(&job);
    for (int i = 1; i < started; i++) pthread_join(th[i], NULL);
    return 0;
}
