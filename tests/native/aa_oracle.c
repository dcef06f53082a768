/*
 * aa_oracle.c — the CPU references of the camera and colour families (the oracle with the camera ray given per pixel, and the sky
 * path of environment_oracle.c, both included unchanged) extended by the sample loop of opencl_kernel.cl:641-648, for
 * tests/test_gpu_adaptive_aa.py.  TEST INFRASTRUCTURE ONLY.
 *
 * rpt_aa_oracle_render: pixel id = y * width + x has n * n samples; sample s = sy * n + sx looks along
 * dirs[3 (id n n + s) .. + 2] (unnormalised: the pinhole's or the lens's plane point at (x + sx / n, y + sy / n), or the panorama's p
 * of pixel (n x + sx, n y + sy) at n times the size — built by the test from the library's own tables).  Each sample's colour is the
 * oracle's trace (a miss is its background; with doppler != 0 doppler_oracle.c's trace_doppler, sky image or none) or, with a sky image
 * (rgb8 != NULL), the sky of the sample's own direction where the ray hits nothing; the colours are summed in sample order, one float addition after another, divided by n * n, then tonemapped,
 * clamped and packed exactly as render_pixel does.  hits_out[id] (if not NULL) = how many of the pixel's samples hit an object.
 */
#include "environment_oracle.c"

typedef struct {
    const rpt_oracle_args *a;
    const Scene *scene;
    const float *dirs;
    int n;
    int use_env;
    EnvImage env;
    rpt_float4 E[4];
    int doppler;
    uint8_t *hits_out;
    volatile int next_row;
} AaJob;

static void aa_pixel(const AaJob *job, unsigned int id) {
    const rpt_oracle_args *a = job->a;
    const f3 wp = F3(a->white_point[0], a->white_point[1], a->white_point[2]);
    const int n2 = job->n * job->n;
    f3 finalcolor = F3(0.0f, 0.0f, 0.0f);
    int hits = 0;
    for (int s = 0; s < n2; s++) {
        const float *d = job->dirs + 3 * ((size_t)id * (size_t)n2 + (size_t)s);
        Ray camray;
        camray.origin = F3(0, 0, 0);
        camray.dir = normalize3(F3(d[0], d[1], d[2]));
        Hit probe;
        const int hit = intersect_scene(job->scene, &camray, &probe);
        hits += hit ? 1 : 0;
        f3 c;
        if (!hit && job->use_env) c = env_sky(&job->env, job->E, a->interval, job->doppler, camray.dir);
        else if (job->doppler != 0) trace_doppler(job->scene, a->ambient, &camray, job->doppler, NULL, &c);
        else c = trace(job->scene, a->ambient, &camray);
        finalcolor = add3(finalcolor, c);
    }
    if (job->hits_out) job->hits_out[id] = (uint8_t)hits;
    const float fn2 = (float)n2;
    finalcolor = F3(finalcolor.x / fn2, finalcolor.y / fn2, finalcolor.z / fn2);
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

static void *aa_worker(void *p) {
    AaJob *job = (AaJob *)p;
    for (;;) {
        const int y = __sync_fetch_and_add(&job->next_row, 1);
        if (y >= job->a->height) break;
        for (int x = 0; x < job->a->width; x++) aa_pixel(job, (unsigned int)y * (unsigned int)job->a->width + (unsigned int)x);
    }
    return NULL;
}

int rpt_aa_oracle_render(const rpt_oracle_args *a, const float *dirs, int n, const float *E16, const uint8_t *rgb8, int env_width,
                         int env_height, int doppler, uint8_t *hits_out, int threads) {
    if (!a || !dirs || n < 1 || n > 8 || a->width <= 0 || a->height <= 0) return -1;
    if (rgb8 && (!E16 || env_width < 1 || env_height < 1)) return -1;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    Scene sc;
    scene_from_args(a, &sc);
    AaJob job;
    memset(&job, 0, sizeof job);
    job.a = a;
    job.scene = &sc;
    job.dirs = dirs;
    job.n = n;
    job.use_env = rgb8 != NULL;
    if (rgb8) {
        job.env.rgb8 = rgb8; job.env.width = env_width; job.env.height = env_height;
        memcpy(job.E, E16, sizeof job.E);
    }
    job.doppler = doppler;
    job.hits_out = hits_out;
    pthread_t th[64];
    int started = 1;
    while (started < threads && pthread_create(&th[started], NULL, aa_worker, &job) == 0) started++;
    aa_worker(&job);
    for (int i = 1; i < started; i++) pthread_join(th[i], NULL);
    return 0;
}
