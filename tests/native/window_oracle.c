/*
 * window_oracle.c — the CPU oracle (oracle/rpt_oracle.c through tests/native/environment_oracle.c and doppler_oracle.c, all included
 * unchanged) with the per-object time windows of rpt_set_object_windows restated in C (DESIGN.md "Time windows"), for
 * tests/test_window_oracle.py (no GPU) and tests/test_gpu_windows.py.  TEST INFRASTRUCTURE ONLY.
 *
 * intersect_scene_w / sample_light_w / trace_w are the oracle's intersect_scene / sample_light / trace (with trace_doppler's colour
 * operator, whose flags 0 is the identity) and these changes, written from the section's four rules, float32, source order, built with
 * -ffp-contract=off; in(W, t) := !(t < t0) && !(t >= t1):
 *   1. a primary candidate of object i replaces the winner iff newHit.dist < hit.dist && in(W_i, stationaryCam_i.t + dot4(Lorentz_i[0],
 *      rayDir) * newHit.dist);
 *   2. an occluder i != light occludes iff newHit.dist < lightDist && in(W_i, (Lorentz_i origin4).t + (Lorentz_i shadowDir).t * newHit.dist);
 *   3. a light i contributes, and shoots its shadow ray, only if in(W_i, hitPos_LightFrame.t + lightDir_LightFrame.t);
 *   4. interval == 0: the same formulas (the directions' time components are 0).
 * With windows == NULL every test accepts, and the frame is the un-windowed oracle's.
 *
 * rpt_window_oracle_render: pixel id = y * width + x looks along dirs[3 id .. 3 id + 2] (unnormalised).  Outputs, each optional: the
 * frame (a->out_pixels, a->out_rgb; with a sky image a miss looks it up as environment_oracle.c does), the event records
 * (event_oracle.c's layout: the winner of rule 1), and one byte of bookkeeping per pixel for the tests' non-vacuity conditions:
 *   bit 0  the ray hit an object
 *   bit 1  the winner lies BEHIND a candidate that its window rejected (a farther object seen through a rejected nearer one)
 *   bit 2  some light reached the pixel only because every occluder below lightDist was outside its window (a shadow removed)
 *   bit 3  some light other than the hit object was outside its window at this pixel
 */
#include "environment_oracle.c"

typedef struct {
    int32_t object;
    float dist;
    float event[4];
    float uv[2];
} WindowEventRecord;
_Static_assert(sizeof(WindowEventRecord) == 32, "the record is 32 B");

static int window_in(const float *windows, int i, float t) {
    if (!windows) return 1;
    return !(t < windows[2 * i]) && !(t >= windows[2 * i + 1]);
}

/* opencl_kernel.cl:361-486 + rule 1; *behind_rejected: the winner is farther than a rejected candidate */
static int intersect_scene_w(const Scene *s, const float *windows, const Ray *ray, Hit *hit, f4 *event_out, int *behind_rejected) {
    float inf = 1e20f;
    hit->dist = inf;
    int didHit = 0;
    f4 event = F4(0, 0, 0, 0);
    const int interval = s->interval;
    float nearest_rejected = inf;

    for (int i = 0; i < s->object_count; i++) {
        Hit newHit;
        newHit.dist = inf;
        Ray4D newRay;
        f4 newEvent0 = ld4(s->objects[i].stationaryCam);
        f3 nd = normalize3(ray->dir);
        f4 rayDir = F4((float)interval, nd.x, nd.y, nd.z);
        f4 lightDir = transformPoint4D(s->objects[i].Lorentz, rayDir);
        newRay.origin = newEvent0;
        newRay.dir = lightDir;

        int got = 0;
        switch (s->objects[i].type) {
        case RPT_SPHERE: got = intersect_sphere(s, i, &newRay, &newHit); break;
        case RPT_CUBE:   got = intersect_cube(s, i, &newRay, &newHit); break;
        case RPT_MESH:   got = intersect_octree(s, i, &newRay, &newHit); break;
        }
        if (got) {
            const float te = s->objects[i].stationaryCam.x + dot4(ld4(s->objects[i].Lorentz[0]), rayDir) * newHit.dist;
            if (newHit.dist < hit->dist) {
                if (window_in(windows, i, te)) {
                    event = add4(newEvent0, muls4(lightDir, newHit.dist));
                    *hit = newHit;
                    hit->object = i;
                    didHit = 1;
                } else if (newHit.dist < nearest_rejected) {
                    nearest_rejected = newHit.dist;
                }
            }
        }
    }
    if (event_out) *event_out = event;
    if (behind_rejected) *behind_rejected = didHit && nearest_rejected < hit->dist;
    if (didHit) {
        const rpt_object *ho = &s->objects[hit->object];
        if (ho->textureIndex != -1) {
            int width = ho->textureWidth;
            int height = ho->textureHeight;
            float u = width * hit->uv.x;
            float v = height * (1.0f - hit->uv.y);
            int x = imin(f2i_sat(floorf(u)), width - 1);
            int y = imin(f2i_sat(floorf(v)), height - 1);
            float u_ratio = u - x;
            float v_ratio = v - y;
            float u_opp = 1 - u_ratio;
            float v_opp = 1 - v_ratio;

            int offset = ho->textureIndex;
            f3 result = muls3(texel3(s, offset, width, x, y), u_opp);
            x = iclamp(x + 1, 0, width - 1);
            result = add3(result, muls3(texel3(s, offset, width, x, y), u_ratio));
            result = muls3(result, v_opp);
            y = iclamp(y + 1, 0, height - 1);
            f3 result2 = muls3(texel3(s, offset, width, x, y), u_ratio);
            x = iclamp(x - 1, 0, width - 1);
            result2 = add3(result2, muls3(texel3(s, offset, width, x, y), u_opp));
            result2 = muls3(result2, v_ratio);

            hit->color = add3(result, result2);
        } else {
            hit->color = xyz(ho->color);
        }
        if (ho->flashPeriod > 0) {
            float period = ho->flashPeriod;
            float duration = ho->flashDuration;
            if (event.x - period * floorf(event.x / period) < duration) {
                hit->color = muls3(hit->color, 2);
            }
        }
        return 1;
    }
    return 0;
}

/* opencl_kernel.cl:488-545 + rule 2; *rejected: an occluder below lightDist was outside its window */
static int sample_light_w(const Scene *s, const float *windows, const Ray4D *ray, float lightDist, const int lightIndex, int *rejected) {
    float inf = 1e20f;
    const int interval = s->interval;
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
                    if (window_in(windows, i, ts)) return i;
                    *rejected = 1;
                }
            }
        }
    }
    return -1;
}

/* opencl_kernel.cl:548-604 + trace_doppler's colour operator + rule 3; returns 1 where the ray hit */
static int trace_w(const Scene *s, const float *windows, const float ambient, const Ray *camray, const int flags, f3 *out,
                   WindowEventRecord *rec, uint8_t *book) {
    Hit hit;
    const int interval = s->interval;
    f4 event;
    int behind = 0;
    uint8_t bits = 0;
    if (!intersect_scene_w(s, windows, camray, &hit, &event, &behind)) {
        if (rec) {
            memset(rec, 0, sizeof *rec);
            rec->object = -1;
        }
        if (book) *book = 0;
        *out = F3(0.15f, 0.15f, 0.25f);
        return 0;
    }
    bits |= 1;
    if (behind) bits |= 2;
    if (rec) {
        rec->object = hit.object;
        rec->dist = hit.dist;
        rec->event[0] = event.x; rec->event[1] = event.y; rec->event[2] = event.z; rec->event[3] = event.w;
        rec->uv[0] = hit.uv.x; rec->uv[1] = hit.uv.y;
    }

    const rpt_object *ho = &s->objects[hit.object];
    f3 color = muls3(hit.color, (interval != 0 ? ambient : 1.0f));

    if (ho->light) {
        color = add3(color, hit.color);
    }
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
                const float tl = hitPos_LightFrame.x + lightDir_LightFrame.x;
                if (!window_in(windows, i, tl)) {
                    bits |= 8;
                    continue;
                }
                f4 lightDir = transformPoint4D(lo->InvLorentz, lightDir_LightFrame);
                f4 lightDir_ObjFrame = transformPoint4D(ho->Lorentz, lightDir);
                f3 lightDir3_ObjFrame = yzw(lightDir_ObjFrame);
                f3 unitLightDir3 = normalize3(lightDir3_ObjFrame);

                if (dot3(hit.normal, unitLightDir3) > 0) {
                    Ray4D newRay;
                    f3 ld = normalize3(yzw(lightDir));
                    newRay.dir = F4((float)interval, ld.x, ld.y, ld.z);
                    newRay.origin = hitPos;
                    int rejected = 0;
                    int shadowIndex = sample_light_w(s, windows, &newRay, length3(yzw(lightDir)), i, &rejected);
                    if (shadowIndex == -1) {
                        if (rejected) bits |= 4;
                        float k = dot3(hit.normal, unitLightDir3) /
                                  (1.0f + 0.1f * length3(lightDir3_ObjFrame) +
                                   0.01f * dot3(lightDir3_ObjFrame, lightDir3_ObjFrame));
                        const float di = lightDir_ObjFrame.x / lightDir_LightFrame.x;
                        color = add3(color, mul3(muls3(hit.color, k), env_doppler(flags, di, xyz(lo->color))));
                    }
                }
            }
        }
    }
    if (interval != 0) {
        const float dcam = (float)interval / dot4(ld4(ho->Lorentz[0]), rayDir0);
        color = env_doppler(flags, dcam, color);
    }
    if (book) *book = bits;
    *out = color;
    return 1;
}

typedef struct {
    const rpt_oracle_args *a;
    const Scene *scene;
    const float *dirs;
    const float *windows;
    int flags;
    int sky;
    EnvImage env;
    rpt_float4 E[4];
    WindowEventRecord *events;
    uint8_t *book;
    volatile int next_row;
} WindowJob;

static void window_pixel(const WindowJob *job, unsigned int id) {
    const rpt_oracle_args *a = job->a;
    const f3 wp = F3(a->white_point[0], a->white_point[1], a->white_point[2]);
    Ray camray;
    camray.origin = F3(0, 0, 0);
    camray.dir = normalize3(F3(job->dirs[3 * (size_t)id], job->dirs[3 * (size_t)id + 1], job->dirs[3 * (size_t)id + 2]));
    f3 finalcolor;
    const int hit = trace_w(job->scene, job->windows, a->ambient, &camray, job->flags, &finalcolor, job->events ? &job->events[id] : NULL,
                            job->book ? &job->book[id] : NULL);
    if (!hit && job->sky) finalcolor = env_sky(&job->env, job->E, a->interval, job->flags, camray.dir);
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

static void *window_worker(void *p) {
    WindowJob *job = (WindowJob *)p;
    for (;;) {
        const int y = __sync_fetch_and_add(&job->next_row, 1);
        if (y >= job->a->height) break;
        for (int x = 0; x < job->a->width; x++) window_pixel(job, (unsigned int)y * (unsigned int)job->a->width + (unsigned int)x);
    }
    return NULL;
}

/* windows: 2 * object_count floats or NULL; flags: the Doppler flags (0 = plain); E16 / rgb8 / env_width / env_height: the sky, or NULL
 * / 0; events_out: width * height records or NULL; book_out: width * height bytes or NULL */
int rpt_window_oracle_render(const rpt_oracle_args *a, const float *dirs, const float *windows, int flags, const float *E16,
                             const uint8_t *rgb8, int env_width, int env_height, void *events_out, uint8_t *book_out, int threads) {
    if (!a || !dirs || a->width <= 0 || a->height <= 0 || flags < 0 || flags > 3) return -1;
    if (rgb8 && (!E16 || env_width < 1 || env_height < 1)) return -1;
    if (threads < 1) threads = 1;
    if (threads > 64) threads = 64;
    Scene sc;
    scene_from_args(a, &sc);
    WindowJob job;
    memset(&job, 0, sizeof job);
    job.a = a;
    job.scene = &sc;
    job.dirs = dirs;
    job.windows = windows;
    job.flags = flags;
    job.sky = rgb8 != NULL;
    if (rgb8) {
        job.env.rgb8 = rgb8; job.env.width = env_width; job.env.height = env_height;
        memcpy(job.E, E16, sizeof job.E);
    }
    job.events = (WindowEventRecord *)events_out;
    job.book = book_out;
    pthread_t th[64];
    int started = 1;
    while (started < threads && pthread_create(&th[started], NULL, window_worker, &job) == 0) started++;
    window_worker(&job);
    for (int i = 1; i < started; i++) pthread_join(th[i], NULL);
    return 0;
}
