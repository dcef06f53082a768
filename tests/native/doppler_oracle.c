/*
 * doppler_oracle.c — the CPU oracle (oracle/rpt_oracle.c, included unchanged) with the camera ray given per pixel and the Doppler and
 * beaming of rpt_set_doppler restated in C for rays that HIT an object, for tests/test_doppler_oracle.py (no GPU) and
 * tests/test_gpu_doppler_parity.py.  TEST INFRASTRUCTURE ONLY.
 *
 * trace_doppler is the oracle's trace() (opencl_kernel.cl:548-604) with the three changes of DESIGN.md "Doppler and beaming", written
 * from that section and from trace(), not from device code; float32, source order, built with -ffp-contract=off:
 *   1. each lit light's colour becomes S_f(D_i, lo.color), D_i = lightDir_ObjFrame.x / lightDir_LightFrame.x;
 *   2. the summed colour (ambient, emission, flash, lights) goes through S_f(D_cam, .), D_cam = (float)interval / dot4(ho.Lorentz[0], rayDir);
 *   3. with interval == 0 both factors are skipped.
 * With flags == 0 S_f is the identity and the colour is trace()'s, bit for bit.
 *
 * The record per pixel (rpt_doppler_oracle_record, 17 words) starts with the 11 floats of rpt_set_debug_doppler — D_cam, the first
 * contributing light's D (1 if none), the reference's colour, the colour after the light factors, the final colour — and adds what the
 * float64 checks need: that light's index (-1 if none), its lightDir_LightFrame, and the hit object's index.  A miss: 11 zeros, -1, 0s, -1.
 *
 * rpt_doppler_oracle_render: pixel id = y * width + x looks along dirs[3 id .. 3 id + 2] (unnormalised: the pinhole's or the lens's plane
 * point, the panorama's p, against re-based objects a turned camera), traced with Doppler flags `flags`, then the tonemap, the clamp and
 * the pack of render_pixel.  rpt_doppler_oracle_render_pinhole: the same with createCamRay's ray of a width x height frame.
 * rpt_doppler_oracle_colour: S_f on n inputs {D, r, g, b, flags} -> {r, g, b}.
 */
#include "../../oracle/rpt_oracle.c"
#include "doppler_colour.h"

typedef struct {
    float dcam, dlight;
    float ref[3], lit[3], final[3];
    int32_t light;
    float lightDir_LightFrame[4];
    int32_t object;
} rpt_doppler_oracle_record;

static void record_miss(rpt_doppler_oracle_record *rec) {
    memset(rec, 0, sizeof *rec);
    rec->light = -1;
    rec->object = -1;
}

/* opencl_kernel.cl:548-604 + DESIGN.md "Doppler and beaming"; returns 1 where the ray hit (the colour is the background otherwise) */
static int trace_doppler(const Scene *s, const float ambient, const Ray *camray, const int flags, rpt_doppler_oracle_record *rec, f3 *out) {
    Hit hit;
    const int interval = s->interval;
    if (!intersect_scene(s, camray, &hit)) {
        if (rec) record_miss(rec);
        *out = F3(0.15f, 0.15f, 0.25f);
        return 0;
    }

    const rpt_object *ho = &s->objects[hit.object];
    f3 color = muls3(hit.color, (interval != 0 ? ambient : 1.0f));

    if (ho->light) {
        color = add3(color, hit.color);
    }
    f3 color_ref = color;               /* the same sum with the reference's light colours (the record only) */
    float dlight = 1.0f;
    int first_light = -1;
    f4 first_dir = F4(0, 0, 0, 0);
    const f3 nd0 = normalize3(camray->dir);
    const f4 rayDir0 = F4((float)interval, nd0.x, nd0.y, nd0.z);
    if (interval != 0) {
        for (int i = 0; i < s->object_count; i++) {
            if (i != hit.object && s->objects[i].light) {
                const rpt_object *lo = &s->objects[i];
                f4 cameraPos_ObjFrame = ld4(ho->stationaryCam);
                f3 nd = normalize3(camray->dir);
                f4 rayDir = F4((float)interval, nd.x, nd.y, nd.z);
                f4 rayDir_ObjFrame = transformPoint4D(ho->Lorentz, rayDir);
                f4 hitPos_ObjFrame = add4(cameraPos_ObjFrame, muls4(rayDir_ObjFrame, hit.dist));
                hitPos_ObjFrame = add4(hitPos_ObjFrame,
                                       F4(0, hit.normal.x * 0.001f, hit.normal.y * 0.001f, hit.normal.z * 0.001f));
                f4 hitPos = transformPoint4D(ho->InvLorentz, hitPos_ObjFrame);
                f4 hitPos_LightFrame = transformPoint4D(lo->Lorentz, hitPos);
                f3 hitPos3_LightFrame = yzw(hitPos_LightFrame);
                f3 lightPos3_LightFrame = F3(lo->M[0].w, lo->M[1].w, lo->M[2].w);
                f3 lightDir3_LightFrame = sub3(lightPos3_LightFrame, hitPos3_LightFrame);
                f4 lightDir_LightFrame = F4(interval * length3(lightDir3_LightFrame),
                                            lightDir3_LightFrame.x, lightDir3_LightFrame.y, lightDir3_LightFrame.z);
                f4 lightDir = transformPoint4D(lo->InvLorentz, lightDir_LightFrame);
                f4 lightDir_ObjFrame = transformPoint4D(ho->Lorentz, lightDir);
                f3 lightDir3_ObjFrame = yzw(lightDir_ObjFrame);
                f3 unitLightDir3 = normalize3(lightDir3_ObjFrame);

                if (dot3(hit.normal, unitLightDir3) > 0) {
                    Ray4D newRay;
                    f3 ld = normalize3(yzw(lightDir));
                    newRay.dir = F4((float)interval, ld.x, ld.y, ld.z);
                    newRay.origin = hitPos;
                    int shadowIndex = sample_light(s, &newRay, length3(yzw(lightDir)), i);
                    if (shadowIndex == -1) {
                        float k = dot3(hit.normal, unitLightDir3) /
                                  (1.0f + 0.1f * length3(lightDir3_ObjFrame) +
                                   0.01f * dot3(lightDir3_ObjFrame, lightDir3_ObjFrame));
                        /* the light factor: received / emitted frequency, the time components of the same path in the two frames */
                        const float di = lightDir_ObjFrame.x / lightDir_LightFrame.x;
                        if (first_light < 0) {
                            first_light = i;
                            dlight = di;
                            first_dir = lightDir_LightFrame;
                        }
                        color_ref = add3(color_ref, mul3(muls3(hit.color, k), xyz(lo->color)));
                        color = add3(color, mul3(muls3(hit.color, k), env_doppler(flags, di, xyz(lo->color))));
                    }
                }
            }
        }
    }
    float dcam = 1.0f;
    const f3 lit = color;
    if (interval != 0) {
        /* the camera factor: camera / emitted frequency, interval over the ray's time component in the hit object's frame */
        dcam = (float)interval / dot4(ld4(ho->Lorentz[0]), rayDir0);
        color = env_doppler(flags, dcam, color);
    }
    if (rec) {
        rec->dcam = dcam;
        rec->dlight = dlight;
        rec->ref[0] = color_ref.x; rec->ref[1] = color_ref.y; rec->ref[2] = color_ref.z;
        rec->lit[0] = lit.x; rec->lit[1] = lit.y; rec->lit[2] = lit.z;
        rec->final[0] = color.x; rec->final[1] = color.y; rec->final[2] = color.z;
        rec->light = first_light;
        rec->lightDir_LightFrame[0] = first_dir.x; rec->lightDir_LightFrame[1] = first_dir.y;
        rec->lightDir_LightFrame[2] = first_dir.z; rec->lightDir_LightFrame[3] = first_dir.w;
        rec->object = hit.object;
    }
    *out = color;
    return 1;
}

typedef struct {
    const rpt_oracle_args *a;
    const Scene *scene;
    const float *dirs;          /* NULL: createCamRay */
    int flags;
    rpt_doppler_oracle_record *records;
    volatile int next_row;
} DopplerJob;

static void doppler_pixel(const DopplerJob *job, unsigned int id) {
    const rpt_oracle_args *a = job->a;
    const f3 wp = F3(a->white_point[0], a->white_point[1], a->white_point[2]);
    Ray camray;
    if (job->dirs) {
        camray.origin = F3(0, 0, 0);
        camray.dir = normalize3(F3(job->dirs[3 * (size_t)id], job->dirs[3 * (size_t)id + 1], job->dirs[3 * (size_t)id + 2]));
    } else {
        camray = createCamRay((float)(id % (unsigned int)a->width), (float)(id / (unsigned int)a->width), a->width, a->height);
    }
    f3 finalcolor;
    trace_doppler(job->scene, a->ambient, &camray, job->flags, job->records ? &job->records[id] : NULL, &finalcolor);
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

static void *doppler_worker(void *p) {
    DopplerJob *job = (DopplerJob *)p;
    for (;;) {
        const int y = __sync_fetch_and_add(&job->next_row, 1);
        if (y >= job->a->height) break;
        for (int x = 0; x < job->a->width; x++) doppler_pixel(job, (unsigned int)y * (unsigned int)job->a->width + (unsigned int)x);
    }
    return NULL;
}

static int doppler_run(const rpt_oracle_args *a, const float *dirs, int flags, void *records, int threads) {
    if (!a || a->width <= 0 || a->height <= 0 || flags < 0 || flags > 3) return -1;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    Scene sc;
    scene_from_args(a, &sc);
    DopplerJob job;
    memset(&job, 0, sizeof job);
    job.a = a;
    job.scene = &sc;
    job.dirs = dirs;
    job.flags = flags;
    job.records = (rpt_doppler_oracle_record *)records;
    pthread_t th[64];
    int started = 1;
    while (started < threads && pthread_create(&th[started], NULL, doppler_worker, &job) == 0) started++;
    doppler_worker(&job);
    for (int i = 1; i < started; i++) pthread_join(th[i], NULL);
    return 0;
}

int rpt_doppler_oracle_render(const rpt_oracle_args *a, const float *dirs, int flags, void *records, int threads) {
    if (!dirs) return -1;
    return doppler_run(a, dirs, flags, records, threads);
}

int rpt_doppler_oracle_render_pinhole(const rpt_oracle_args *a, int flags, void *records, int threads) {
    return doppler_run(a, NULL, flags, records, threads);
}

int rpt_doppler_oracle_record_bytes(void) { return (int)sizeof(rpt_doppler_oracle_record); }

int rpt_doppler_oracle_colour(const float *in5, float *out3, int n) {
    if (!in5 || !out3) return -1;
    for (int i = 0; i < n; i++) {
        const float *p = in5 + 5 * (size_t)i;
        const f3 o = env_doppler((int)p[4], p[0], F3(p[1], p[2], p[3]));
        out3[3 * (size_t)i + 0] = o.x; out3[3 * (size_t)i + 1] = o.y; out3[3 * (size_t)i + 2] = o.z;
    }
    return 0;
}
