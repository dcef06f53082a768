/*
 * panorama_oracle.c — the CPU oracle (oracle/rpt_oracle.c, included unchanged) with the camera ray given per pixel: what the
 * panorama kernels compute (rpt_set_projection), for tests/test_gpu_panorama.py.  TEST INFRASTRUCTURE ONLY.
 *
 * rpt_panorama_oracle_render: pixel id = y * width + x of rows [row_begin, row_end) looks along dirs[3 id .. 3 id + 2] (the
 * unnormalised p of include/rpt.h, built by the test from the library's own tables); the ray is Ray{0, normalize3(p)} as createCamRay
 * builds it, then trace, the tonemap, the clamp and the pack exactly as render_pixel does for msaa <= 1.
 */
#include "../../oracle/rpt_oracle.c"

typedef struct {
    const rpt_oracle_args *a;
    const Scene *scene;
    const float *dirs;
    int row_begin, row_end;
    volatile int next_row;
} PanoJob;

static void pano_pixel(const PanoJob *job, unsigned int id) {
    const rpt_oracle_args *a = job->a;
    const f3 wp = F3(a->white_point[0], a->white_point[1], a->white_point[2]);
    Ray camray;
    camray.origin = F3(0, 0, 0);
    camray.dir = normalize3(F3(job->dirs[3 * (size_t)id], job->dirs[3 * (size_t)id + 1], job->dirs[3 * (size_t)id + 2]));
    f3 finalcolor = trace(job->scene, a->ambient, &camray);
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

static void *pano_worker(void *p) {
    PanoJob *job = (PanoJob *)p;
    for (;;) {
        const int y = job->row_begin + __sync_fetch_and_add(&job->next_row, 1);
        if (y >= job->row_end) break;
        for (int x = 0; x < job->a->width; x++) pano_pixel(job, (unsigned int)y * (unsigned int)job->a->width + (unsigned int)x);
    }
    return NULL;
}

int rpt_panorama_oracle_render(const rpt_oracle_args *a, const float *dirs, int row_begin, int row_end, int threads) {
    if (!a || !dirs || a->width <= 0 || a->height <= 0) return -1;
    if (row_begin < 0) row_begin = 0;
    if (row_end > a->height) row_end = a->height;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    Scene sc;
    scene_from_args(a, &sc);
    PanoJob job = {a, &sc, dirs, row_begin, row_end, 0};
    pthread_t th[64];
    int started = 1;
    while (started < threads && pthread_create(&th[started], NULL, pano_worker, &job) == 0) started++;
    pano_worker(&job);          /* (fewer threads than asked for: the rows are still all rendered) */
    for (int i = 1; i < started; i++) pthread_join(th[i], NULL);
    return 0;
}
