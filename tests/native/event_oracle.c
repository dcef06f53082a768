/*
 * event_oracle.c — the CPU oracle (oracle/rpt_oracle.c, included unchanged) with the camera ray given per pixel, reporting the
 * per-pixel event record of rpt_render_events (include/rpt_layout.h: rpt_event; DESIGN.md "Event pass") instead of a colour, for
 * tests/test_events_model.py and tests/test_gpu_events.py.  TEST INFRASTRUCTURE ONLY.
 *
 * rpt_event_oracle_render: pixel id = y * width + x looks along dirs[3 id .. 3 id + 2] (unnormalised: the pinhole's plane point, the
 * lens' scaled one or the panorama's p).  intersect_scene finds the winner; the record is formed from its Hit and the hit object:
 *   object = Hit.object, dist = Hit.dist, uv = Hit.uv,
 *   event  = stationaryCam + (Lorentz (interval, normalize(dir))) * dist      (opencl_kernel.cl:386-388, :396; intersect_scene's own
 *            `event`, which it keeps to itself, recomputed here with the same float operations in the same order)
 * A miss is {-1, 0, 0, 0, 0, 0, 0, 0}.
 */
#include "../../oracle/rpt_oracle.c"

typedef struct {
    int32_t object;
    float dist;
    float event[4];
    float uv[2];
} EventRecord;
_Static_assert(sizeof(EventRecord) == 32, "the record is 32 B");

typedef struct {
    const rpt_oracle_args *a;
    const Scene *scene;
    const float *dirs;
    EventRecord *out;
    volatile int next_row;
} EventJob;

static void event_pixel(const EventJob *job, size_t id) {
    const Scene *s = job->scene;
    Ray camray;
    camray.origin = F3(0, 0, 0);
    camray.dir = normalize3(F3(job->dirs[3 * id], job->dirs[3 * id + 1], job->dirs[3 * id + 2]));
    EventRecord *r = &job->out[id];
    Hit hit;
    if (!intersect_scene(s, &camray, &hit)) {
        r->object = -1;
        r->dist = 0.0f;
        r->event[0] = r->event[1] = r->event[2] = r->event[3] = 0.0f;
        r->uv[0] = r->uv[1] = 0.0f;
        return;
    }
    const rpt_object *ho = &s->objects[hit.object];
    const f3 nd = normalize3(camray.dir);                      /* intersect_scene's own line (:386) */
    f4 lightDir = F4((float)s->interval, nd.x, nd.y, nd.z);
    lightDir = transformPoint4D(ho->Lorentz, lightDir);
    const f4 event = add4(ld4(ho->stationaryCam), muls4(lightDir, hit.dist));
    r->object = hit.object;
    r->dist = hit.dist;
    r->event[0] = event.x; r->event[1] = event.y; r->event[2] = event.z; r->event[3] = event.w;
    r->uv[0] = hit.uv.x; r->uv[1] = hit.uv.y;
}

static void *event_worker(void *p) {
    EventJob *job = (EventJob *)p;
    for (;;) {
        const int y = __sync_fetch_and_add(&job->next_row, 1);
        if (y >= job->a->height) break;
        for (int x = 0; x < job->a->width; x++) event_pixel(job, (size_t)y * (size_t)job->a->width + (size_t)x);
    }
    return NULL;
}

int rpt_event_oracle_render(const rpt_oracle_args *a, const float *dirs, void *records_out, int threads) {
    if (!a || !dirs || !records_out || a->width <= 0 || a->height <= 0) return -1;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    Scene sc;
    scene_from_args(a, &sc);
    EventJob job;
    memset(&job, 0, sizeof job);
    job.a = a;
    job.scene = &sc;
    job.dirs = dirs;
    job.out = (EventRecord *)records_out;
    pthread_t th[64];
    int started = 1;
    while (started < threads && pthread_create(&th[started], NULL, event_worker, &job) == 0) started++;
    event_worker(&job);
    for (int i = 1; i < started; i++) pthread_join(th[i], NULL);
    return 0;
}

/* intersect_sphere alone on one rest-frame ray {origin4, dir4} of object `object_index`: the float the analytic anchor compares with */
int rpt_event_oracle_sphere_dist(const rpt_oracle_args *a, int object_index, const float *origin4, const float *dir4, float *dist_out) {
    if (!a || !origin4 || !dir4 || !dist_out || object_index < 0 || object_index >= a->object_count) return -1;
    Scene sc;
    scene_from_args(a, &sc);
    Ray4D ray;
    ray.origin = F4(origin4[0], origin4[1], origin4[2], origin4[3]);
    ray.dir = F4(dir4[0], dir4[1], dir4[2], dir4[3]);
    Hit hit;
    hit.dist = 1e20f;
    if (!intersect_sphere(&sc, object_index, &ray, &hit)) return 1;
    *dist_out = hit.dist;
    return 0;
}
