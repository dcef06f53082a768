/*
 * rpt_layout.h — byte-level buffer layouts of the render path.
 *
 * These are the exact layouts the reference host writes and its kernel reads:
 *   Object   reference Object.h:6-22   == opencl_kernel.cl:21-36   (320 B)
 *   Octree   reference Octree.h:4-12   == opencl_kernel.cl:46-53   ( 96 B)
 *   Mesh SoA reference Mesh.h:7-13     (vertices/normals 16 B stride, uvs 8 B,
 *            triangles 9 x u32 per triangle [v,uv,n]x3, octreeTris i32,
 *            textures interleaved RGB8 rows, top row first)
 *   pixel    reference opencl_kernel.cl:652-659, gl_interop.cpp:56-57 (16 B)
 *
 * cl_float3 is cl_float4 (16 B, align 16) on the host side (CL/cl_platform.h),
 * so every float3 slot is 16 bytes with an unused 4th lane.
 *
 * Shared by plain C (oracle), C++ (host library) and HIP device code.
 */
#ifndef RPT_LAYOUT_H
#define RPT_LAYOUT_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rpt_float2 { float x, y; } rpt_float2;                 /* cl_float2 */
typedef struct rpt_float4 { float x, y, z, w; } rpt_float4;           /* cl_float4 == cl_float3 */
typedef rpt_float4 rpt_float3;                                        /* 16 B slot, .w unused */

enum rpt_object_type { RPT_SPHERE = 0, RPT_CUBE = 1, RPT_MESH = 2 }; /* Object.h:4 */

typedef struct rpt_object {
    rpt_float4 M[4];          /*   0  object -> world, row-major rows          */
    rpt_float4 InvM[4];       /*  64  world -> object                          */
    rpt_float4 Lorentz[4];    /* 128  camera frame -> object rest frame (t,x,y,z) */
    rpt_float4 InvLorentz[4]; /* 192  object rest frame -> camera frame        */
    rpt_float4 stationaryCam; /* 256  camera event in the object's rest frame  */
    rpt_float3 color;         /* 272                                           */
    int32_t    type;          /* 288  rpt_object_type                          */
    int32_t    meshIndex;     /* 292  index of the mesh's octree root          */
    int32_t    textureIndex;  /* 296  BYTE offset into the texture pool, -1 = none */
    int32_t    textureWidth;  /* 300                                           */
    int32_t    textureHeight; /* 304                                           */
    uint8_t    light;         /* 308  bool                                     */
    uint8_t    _pad[3];       /* 309                                           */
    float      flashPeriod;   /* 312                                           */
    float      flashDuration; /* 316                                           */
} rpt_object;

typedef struct rpt_octree {
    rpt_float3 min;           /*  0 */
    rpt_float3 max;           /* 16 */
    int32_t    trisIndex;     /* 32  first entry in octreeTris */
    int32_t    trisCount;     /* 36 */
    int32_t    children[8];   /* 40  index z + 2y + 4x, -1 = leaf */
    int32_t    neighbors[6];  /* 72  -z,+z,-x,+x,-y,+y ; -1 = outside */
} rpt_octree;

typedef struct rpt_pixel {
    float   x, y;             /* 0,4  pixel coordinates as floats (GL vertex)  */
    uint8_t rgba[4];          /* 8    R,G,B,1 (GL colour, reinterpreted float) */
    uint32_t unspecified;     /* 12   never read by the consumer               */
} rpt_pixel;

/*
 * One record of the event pass (rpt_render_events; not in the reference): what a pixel's primary ray sees, where and when.
 * A miss is {-1, 0, 0, 0, 0, 0, 0, 0}, stored exactly so.
 */
typedef struct rpt_event {
    int32_t object;           /*  0  index into the context's Object[] of the closest hit; -1 = the ray hits nothing */
    float   dist;             /*  4  Hit.dist of the winner (opencl_kernel.cl:395-397): the camera-frame distance    */
    float   event[4];         /*  8  stationaryCam + (Lorentz (interval, normalize(dir))) * dist of the hit object:
                                     t, x, y, z in ITS rest frame, the float operations of :386-388 and :396 in that order */
    float   uv[2];            /* 24  Hit.uv of the winner, as the texture lookup of :430-431 receives it */
} rpt_event;

/* One object's display in the readout pass (not in the reference; include/rpt.h, rpt_set_readouts, states the rules) */
typedef struct rpt_readout {      /* 36 B, one per entry of Object[] */
    float   rate, offset;         /* value shown: offset + rate * event[0] */
    float   u0, v0, u1, v1;       /* the display's rectangle in the hit's (u, v); u0 > u1 or v0 > v1 mirrors it */
    uint8_t digits;               /* 0 = this object has no display; else 1..9 character cells */
    uint8_t decimals;             /* 0..6 and < digits */
    uint8_t _pad[2];
    uint8_t on_rgba[4], off_rgba[4];   /* lit segments / the rest of the rectangle; alpha 0 leaves the picture */
} rpt_readout;

/* One point source of the particle pass (not in the reference; include/rpt.h, rpt_set_particles, states the rules) */
typedef struct rpt_particle {     /* 32 B: two aligned 16-byte loads */
    float   pos[3];               /* position in the REST FRAME of Object[object]: the coordinates of rpt_event.event[1..3] */
    int32_t object;               /* index into the context's Object[]: the frame the particle is at rest in */
    float   rgb[3];               /* linear colour at rest, on the scale of object colours (as rpt_star.rgb) */
    float   _pad;
} rpt_particle;

/* One rod of the segment pass (not in the reference; include/rpt.h, rpt_set_segments, states the rules) */
typedef struct rpt_segment {      /* 48 B: three aligned 16-byte loads */
    float   a[3];                 /* one end, in the REST FRAME of Object[object]: the coordinates of rpt_event.event[1..3] */
    int32_t object;               /* index into the context's Object[]: the frame the rod is at rest in */
    float   b[3];                 /* the other end, same frame */
    float   _pad0;
    float   rgb[3];               /* linear colour at rest PER UNIT REST-FRAME LENGTH, on the scale of object colours */
    float   _pad1;
} rpt_segment;

/* One point source of the ballistic pass (not in the reference; include/rpt.h, rpt_set_ballistics, states the rules) */
typedef struct rpt_ballistic {    /* 48 B: three aligned 16-byte loads */
    float   pos[3];               /* position at time 0 of Object[object]'s rest-frame clock (the clock of rpt_event.event[0]) */
    int32_t object;               /* index into the context's Object[]: the frame the worldline is WRITTEN in; the particle does not ride it */
    float   rgb[3];               /* linear colour at rest in the PARTICLE's own frame, on the scale of object colours */
    float   t0;                   /* the emission window [t0, t1) on that object's clock; -inf / +inf = always */
    float   u[3];                 /* proper velocity gamma * beta in that object's rest frame: every finite u is subluminal */
    float   t1;
} rpt_ballistic;

/* One accelerated point source of the rocket pass (not in the reference; include/rpt.h, rpt_set_rockets, states the rules) */
typedef struct rpt_rocket {       /* 64 B: four aligned 16-byte loads */
    float   pos[3];               /* position at time 0 of Object[object]'s rest-frame clock (the clock of rpt_event.event[0]) */
    int32_t object;               /* index into the context's Object[]: the frame the worldline is WRITTEN in; the rocket does not ride it */
    float   rgb[3];               /* linear colour at rest in the ROCKET's own frame, on the scale of object colours */
    float   t0;                   /* the emission window [t0, t1) on that object's clock; -inf / +inf = always */
    float   u[3];                 /* proper velocity gamma * beta in that object's rest frame at that frame's time 0 */
    float   t1;
    float   acc[3];               /* proper acceleration in the rocket's own instantaneous rest frame at that moment (what the crew feels), c = 1 */
    float   reserved;             /* must be 0 */
} rpt_rocket;

/*
 * The eight read-only scene arrays the reference uploads once (main.cpp:33-55), in the
 * reference's layouts, as {pointer, element count} pairs.  Zero-length arrays are legal and
 * their pointer may be NULL (main.cpp:34 passes NULL for empty vectors).
 */
typedef struct rpt_scene_desc {
    const rpt_object *objects;    size_t object_count;     /* Object[]            arg 0,1 */
    const rpt_float3 *vertices;   size_t vertex_count;     /* cl_float3[]         arg 2   */
    const rpt_float3 *normals;    size_t normal_count;     /* cl_float3[]         arg 3   */
    const rpt_float2 *uvs;        size_t uv_count;         /* cl_float2[]         arg 4   */
    const uint32_t   *triangles;  size_t triangle_words;   /* u32[9*T] (words)    arg 5   */
    const rpt_octree *octrees;    size_t octree_count;     /* Octree[]            arg 6   */
    const int32_t    *octreeTris; size_t octree_tri_count; /* i32[]               arg 7   */
    const uint8_t    *textures;   size_t texture_bytes;    /* u8[] RGB8 pool      arg 8   */
} rpt_scene_desc;

#define RPT_TRI_STRIDE 9      /* u32 per triangle: v0,uv0,n0, v1,uv1,n1, v2,uv2,n2 */

#ifdef __cplusplus
}
#define RPT_SA(c, m) static_assert(c, m)
#else
#define RPT_SA(c, m) _Static_assert(c, m)
#endif

RPT_SA(sizeof(rpt_float2) == 8, "cl_float2");
RPT_SA(sizeof(rpt_float4) == 16, "cl_float4");
RPT_SA(sizeof(rpt_object) == 320, "Object is 320 B");
RPT_SA(offsetof(rpt_object, InvM) == 64, "InvM");
RPT_SA(offsetof(rpt_object, Lorentz) == 128, "Lorentz");
RPT_SA(offsetof(rpt_object, InvLorentz) == 192, "InvLorentz");
RPT_SA(offsetof(rpt_object, stationaryCam) == 256, "stationaryCam");
RPT_SA(offsetof(rpt_object, color) == 272, "color");
RPT_SA(offsetof(rpt_object, type) == 288, "type");
RPT_SA(offsetof(rpt_object, meshIndex) == 292, "meshIndex");
RPT_SA(offsetof(rpt_object, textureIndex) == 296, "textureIndex");
RPT_SA(offsetof(rpt_object, textureWidth) == 300, "textureWidth");
RPT_SA(offsetof(rpt_object, textureHeight) == 304, "textureHeight");
RPT_SA(offsetof(rpt_object, light) == 308, "light");
RPT_SA(offsetof(rpt_object, flashPeriod) == 312, "flashPeriod");
RPT_SA(offsetof(rpt_object, flashDuration) == 316, "flashDuration");
RPT_SA(sizeof(rpt_octree) == 96, "Octree is 96 B");
RPT_SA(offsetof(rpt_octree, max) == 16, "max");
RPT_SA(offsetof(rpt_octree, trisIndex) == 32, "trisIndex");
RPT_SA(offsetof(rpt_octree, trisCount) == 36, "trisCount");
RPT_SA(offsetof(rpt_octree, children) == 40, "children");
RPT_SA(offsetof(rpt_octree, neighbors) == 72, "neighbors");
RPT_SA(sizeof(rpt_pixel) == 16, "pixel is 16 B");
RPT_SA(sizeof(rpt_event) == 32, "event record is 32 B");
RPT_SA(offsetof(rpt_event, event) == 8, "event");
RPT_SA(offsetof(rpt_event, uv) == 24, "uv");
RPT_SA(sizeof(rpt_readout) == 36, "readout is 36 B");
RPT_SA(offsetof(rpt_readout, digits) == 24, "digits");
RPT_SA(offsetof(rpt_readout, on_rgba) == 28, "on_rgba");
RPT_SA(sizeof(rpt_particle) == 32, "particle is 32 B");
RPT_SA(offsetof(rpt_particle, object) == 12, "object");
RPT_SA(offsetof(rpt_particle, rgb) == 16, "rgb");
RPT_SA(sizeof(rpt_segment) == 48, "segment is 48 B");
RPT_SA(offsetof(rpt_segment, object) == 12, "object");
RPT_SA(offsetof(rpt_segment, b) == 16, "b");
RPT_SA(offsetof(rpt_segment, _pad0) == 28, "_pad0");
RPT_SA(offsetof(rpt_segment, rgb) == 32, "rgb");
RPT_SA(offsetof(rpt_segment, _pad1) == 44, "_pad1");
RPT_SA(sizeof(rpt_ballistic) == 48, "ballistic is 48 B");
RPT_SA(offsetof(rpt_ballistic, object) == 12, "object");
RPT_SA(offsetof(rpt_ballistic, rgb) == 16, "rgb");
RPT_SA(offsetof(rpt_ballistic, t0) == 28, "t0");
RPT_SA(offsetof(rpt_ballistic, u) == 32, "u");
RPT_SA(offsetof(rpt_ballistic, t1) == 44, "t1");
RPT_SA(sizeof(rpt_rocket) == 64, "rocket is 64 B");
RPT_SA(offsetof(rpt_rocket, pos) == 0, "pos");
RPT_SA(offsetof(rpt_rocket, object) == 12, "object");
RPT_SA(offsetof(rpt_rocket, rgb) == 16, "rgb");
RPT_SA(offsetof(rpt_rocket, t0) == 28, "t0");
RPT_SA(offsetof(rpt_rocket, u) == 32, "u");
RPT_SA(offsetof(rpt_rocket, t1) == 44, "t1");
RPT_SA(offsetof(rpt_rocket, acc) == 48, "acc");
RPT_SA(offsetof(rpt_rocket, reserved) == 60, "reserved");

#endif /* RPT_LAYOUT_H */
