// rpt_kernels.hip.h — the per-pixel render path for gfx950 (CDNA4, wave64).
//
// What is computed is the reference's render_kernel (opencl_kernel.cl:620-660) and everything it
// calls; how it is computed is organised for MI355X:
//   * one wavefront owns an 8x8 pixel tile (coherent rays, 8 full 128-B lines per store wave) and is a workgroup
//     of its own (its slot is free again when IT ends, not when the longest of four neighbours does); the grid is
//     (4 ceil(W/32), row tiles): 129 600 workgroups at 4K.  The measurement arms keep four waves per workgroup;
//   * Object[] is indexed with a wave-uniform loop counter, so the matrices arrive through the
//     scalar cache into SGPRs (s_load) and are broadcast for free; per-frame constants that do
//     not depend on the pixel (aspect ratio, hable(white_point)) are computed once on the host
//     with the same IEEE operations;
//   * 16 B/pixel framebuffer stores are one global_store_dwordx4 per lane; the multi-GPU variant
//     writes only the 4-B packed colour into a compact plane;
//   * what a wavefront can skip as a whole it skips with a __ballot: its object mask for the primary rays comes from
//     per-object screen bounds (host, rpt_screen_bounds.hpp) tested lane-parallel (wave_object_mask), and a shadow ray's
//     sphere and cube tests are dropped when no lane's segment to the light can reach the object's box (intersect_object).
// fp32 arithmetic order is that of the reference expression by expression (see the oracle for the
// built-in semantics); UB of the reference is neutralised exactly as in oracle/rpt_oracle.c.
#pragma once
#include "../../include/rpt_layout.h"
#include "rpt_device_math.hip.h"

#ifdef RPT_RELAXED_FP
#pragma clang fp contract(fast)      /* rpt_relaxed.hip only: the opt-in "OpenCL-conformant arithmetic" build of the same source */
#else
#pragma clang fp contract(off)
#endif

namespace rptd {

#define RPT_EPSILON 0.0000001f       /* opencl_kernel.cl:6 */
#define RPT_MAX_LEAF_STEPS 4096
#define RPT_LINK_CHILD_MASK 0x00ffffff   /* DNode::link: low 24 bits = first child, high 8 = which children are leaves */
#define RPT_TOP_MAX 3072                 /* node links of the octrees' top levels kept in LDS by the persistent kernels (12 KB) */
#define RPT_PI_D 3.14159265358979323846264338327950288   /* OpenCL C M_PI (double) */

// ---- derived, device-only layouts (built by the library at upload / per frame; values are the
// reference's own numbers or IEEE results of the reference's own operations, so nothing rounds
// differently) ----------------------------------------------------------------------------------
// One octree node in one 64-B line.  Children of a node are consecutive in the reference's builder
// (Octree.cpp:191-269 pushes the eight children back to back), so children[k] = firstChild + k.
// The derived array is numbered breadth first over the whole forest (all roots, then all nodes of level 1, ...): the top levels
// of every octree are the first KernelArgs::top_count records, which is what the persistent kernels keep in LDS.
struct alignas(64) DNode {
    float minx, miny, minz; int link;            // -1 = leaf; else firstChild | (leaf mask of the eight children) << 24
    float maxx, maxy, maxz; int leafBegin;       // first DTri of a leaf
    int leafCount; int nb[6]; int pad;           // neighbours -z,+z,-x,+x,-y,+y
};
static_assert(sizeof(DNode) == 64, "DNode is one 64-B line");
// One leaf triangle reference, gathered: A, B-A, C-A (the ray-independent part of
// intersect_triangle, opencl_kernel.cl:108-109) and the triangle id, instead of the
// octreeTris -> triangles -> vertices chain of three dependent loads.
struct alignas(16) DTri { float ax, ay, az, e1x; float e1y, e1z, e2x, e2y; float e2z; int tri; int pad0, pad1; };
static_assert(sizeof(DTri) == 48, "DTri is three 16-B loads");
// What a walk that leaves node n through side s stands on next, by (n, s): record 6 n + s, two 16-B loads from ONE address instead of
// nb[s] and then the neighbour's node record from the address it returned.  The box is the very floats of the neighbour's DNode;
//   the neighbour is a leaf:  a = its index (24 bits),          b = its leafBegin word (leafBegin | min(leafCount, 255) << 24);
//   the neighbour is inner:   a = its link (any 32 bits but -1), b = RPT_EXIT_INNER;
//   there is no neighbour:    a = -1,                            b = RPT_EXIT_INNER, the box zeros.
// RPT_EXIT_INNER is no leaf's word: a top byte of 1 says the list has exactly one record, which would end at 0x1000000, and the derived
// layout holds at most 0xffffff records (rpt_api.hip: derive_layouts checks both).  So no bit that a link or a begin word can set is taken.
#ifndef RPT_EXIT_RECORDS
#define RPT_EXIT_RECORDS 1      /* 0: the throughput walk reads nb[] and the node record, as before (tools/exit_hit_ab.py builds that arm) */
#endif
#ifndef RPT_HIT_RECORDS
#define RPT_HIT_RECORDS 1       /* 0: a hit's normals and uvs through triangles[] -> normals[] / uvs[], as before (likewise) */
#endif
#define RPT_EXIT_INNER 0x01ffffff
struct alignas(32) DExit { float minx, miny, minz; int a; float maxx, maxy, maxz; int b; };
static_assert(sizeof(DExit) == 32, "DExit is two 16-B loads");
// What mesh_hit_finish needs of triangle id t, record t: the three normals and the three uvs that triangles[9 t ...] names, the floats
// of normals[] / uvs[] themselves — one hop and four 16-B loads behind the id instead of two hops and twelve loads.
struct alignas(64) DHit { float nA[3], nB[3], nC[3]; float uvA[2], uvB[2], uvC[2]; int spare; };
static_assert(sizeof(DHit) == 64, "DHit is one 64-B line");
// Per object, per frame: the primary-ray origin in object space (every primary ray of a frame
// starts at the camera event, opencl_kernel.cl:386-389) and what follows from it alone.
struct alignas(16) DObj {
    float ox, oy, oz; float sphere_c;        // exact (kernel operation order): used by the intersectors
    float winding;
    // conservative culling data (approximate arithmetic is fine here, see rpt_tile_bin_kernel):
    float cbx, cby, cbz;                     // bounding-sphere centre in object space
    float rb;                                // bounding-sphere radius, inflated; < 0 = never cull this object
    float B[9];                              // object-space direction = B * nd + b for a camera direction nd
    float b[3];
    float mesh_in_box;                       // mesh objects: 1 = every triangle the octree can report lies inside the root's box
    int root;                                // mesh objects: the root's index in the derived (breadth-first) node numbering
    float win_t0;                            // the object's time window (rpt_set_object_windows; the Windowed kernels only): a hit whose emission time t in
                                             // the object's rest frame has t < win_t0 or t >= win_t1 (below) does not exist.  0, 0 while the context has none
    // the shadow-ray culls of a mesh object (mesh_ray_misses_root, mesh_segment_apart below; build_dobjs derives them per frame):
    // half extents of the root box about (cbx, cby, cbz) grown by 8u max(|lo|, |hi|) (mh[0] < 0: no cull of this object at all);
    // the segment cull's margin = mconst + mslope * (L1 distance of the ray origin from the centre) (mslope < 0: no segment cull);
    // the allowance of the segment's end per unit of the rest-frame origin's L1 norm.
    float mh[3];
    float mconst, mslope, mcw;
    float ms0;                               // the constant part of that allowance (1e-4 + what the object's own translation costs)
    float win_t1;
};
static_assert(sizeof(DObj) == 128, "DObj");

struct KernelArgs {
    // ---- the first 64 bytes are everything a wave that hits nothing needs (its cull and its store): one scalar load at the top
    // of the kernel instead of one per place of first use (each is a dependent round trip in a wave that lives a microsecond)
    // per-object image-plane rectangles (rpt_screen_bounds.hpp), tested lane-parallel by each wavefront (culled kernels)
    const float4 *rects;                     // [2 * object_count] per object: u0, v0, u1, v1 on the plane z = 0.5, then the
                                             // diagonal slabs p_lo, p_hi (u + v) and m_lo, m_hi (u - v)
    rpt_pixel *out16;        // 16 B/pixel framebuffer (full frame addressing) or null
    uint32_t *plane;         // compact 4 B/pixel colour plane (local tile addressing) or null
    float *debug_rgb;        // 3 floats/pixel, full frame addressing, or null
    int object_count;
    int width, height;
    int diagonals;                           // some object has diagonal slabs and the frame lies inside their window
    float inv_width, inv_height;             // 1/width, 1/height (for the cull only: approximate is fine there)
    float aspect;            // (float)width / (float)height
    uint32_t bg_packed;      // the packed R,G,B,1 word of a miss pixel
    // ---- second line: tile addressing, dispatch order, the rest of the scalars
    int first_tile, tile_step;      // local tile t holds global tile (t >> run_log2) * tile_step + first_tile + (t & (run - 1))
    int run_log2;                   // run = 1 << run_log2 consecutive tiles per period of tile_step tiles (rpt_set_tile_pattern)
    int interval;
    // tile_x0 (in the place of first_sx, which no kernel ever read): the column of 8x8 tiles that workgroup 0 of a row renders, for the
    // kernels a sky split launches over the object box alone (tile_origin_policy below; launch() leaves it 0 everywhere else).  The
    // box's first tile row goes through first_tile, as a rank's share of the rows does.
    // dispatch order (band_first kernels, never split): the tile rows [first_ty, first_ty + first_h) — where the meshes are, i.e. where
    // the frame's longest waves live — are handed out FIRST, the rest in natural order; first_h = 0: off (first_w: never read)
    int tile_x0, first_ty, first_w, first_h;
    int msaa;                       // MSAASAMPLES of opencl_kernel.cl:7 when it is not 1 (rpt_set_msaa; the kernels of render_pixel_body_msaa only)
    float bg_mapped[3];      // min(hable(background)/hable(white_point), 1): what every miss pixel maps to
    float ambient;
    float hable_wp[3];       // hable(white_point), host-computed
    // per-tile object masks: 8x8-pixel tiles of this context's rows, classified once per frame by rpt_tile_bin_kernel
    int mask_tiles_x, n_tiles;               // tiles per row, tiles in this context's rows
    unsigned long long *tile_masks;          // [n_tiles] bit i = primary rays of the tile may hit object i (i < 64)
    // ---- the scene
    const DNode *dnodes;
    const DTri *dtris;
    const DObj *dobjs;
    const int *links;               // DNode::link of every node again, 4 B apart: what a descent reads per level
    const DTri *first_tris;         // per node: the first triangle record of its leaf list again, addressable by the NODE's index
    // the tile bitmaps of the still meshes (rpt_tile_bitmap.hpp; in the place of two tables of removed measurement arms, so that the
    // fields below keep their offsets): bit i of tile_bits_objects = object i has one, at tile_bits + i * ceil(tiles / 32) dwords,
    // bit ty * ceil(width / 8) + tx of it = 0: no primary ray of that 8x8 tile can report a hit of object i.  Null / 0: none.
    const uint32_t *tile_bits;
    unsigned long long tile_bits_objects;
    int reserved;                   // unused
    int top_count;                  // nodes [0, top_count) are the forest's top levels (whole levels, <= RPT_TOP_MAX)
    // persistent kernels (rpt_persistent.hip.h): the band of tile rows that holds the meshes (first_ty, first_h above) is
    // claimed tile by tile from per-queue counters, the other rows are dealt statically in runs of RPT_SKY_RUN tiles
    int tiles_x;                    // 8x8 tiles per row of tiles
    unsigned int tiles_x_magic;     // ceil(2^32 / tiles_x): t / tiles_x = mulhi(t, magic) for every t the host allows
    int runs_x;                     // runs per row of tiles outside the band
    unsigned int runs_x_magic;
    int band_tiles, sky_runs;
    int claim_set;                  // which of the two counter sets this launch counts in
    const rpt_object *objects;
    const rpt_float3 *vertices;
    const rpt_float3 *normals;
    const rpt_float2 *uvs;
    const uint32_t *triangles;
    const rpt_octree *octrees;
    const int32_t *octreeTris;
    const uint8_t *textures;
    long long texture_bytes;
    unsigned long long *wave_times; // diagnostic build only (variant 11): ten words per wave, {start, end} of s_memrealtime (100 MHz) + loop accounting
    unsigned long long *counters;   // diagnostic builds only (variant 7): [0..2] lane-level leaf/tri/descent
                                    // iterations, [3..5] the same counted once per executing wave
    const DExit *exits;             // [6 * nodes] where a walk stands after leaving node n through side s (DExit above)
    const DHit *hits;               // [triangles] the normals and uvs of a triangle id, gathered (DHit above)
};

// The Doppler kernels' arguments (rpt_set_doppler; not in the reference): KernelArgs with two fields appended at the end.  A struct
// of its own rather than more KernelArgs fields, so that every other kernel keeps its argument block — and with it its code, the
// probe kernels' trailing arguments included — byte for byte.  The Doppler bodies reach the fields through a static_cast of the
// KernelArgs they are handed (it is always a DopplerArgs there).
struct DopplerArgs : KernelArgs {
    int doppler;                    // RPT_DOPPLER_SHIFT (1) | RPT_DOPPLER_BEAMING (2); the twins are launched only when != 0
    float *debug_doppler;           // the Doppler debug kernel only: RPT_DOPPLER_RECORD floats per pixel (rpt_set_debug_doppler)
};

// The panorama kernels' arguments (rpt_set_projection; not in the reference): DopplerArgs with the two tables of the equirectangular
// camera appended, for the same reason — no other kernel's argument block changes.  Every panorama kernel takes them, its Doppler
// twins and the others alike (doppler = 0 there).
struct PanoramaArgs : DopplerArgs {
    const float2 *pano_cols;        // [width]  {sin, cos} of the longitude of column x (global x)
    const float2 *pano_rows;        // [height] {sin, cos} of the latitude of row y (global y: row tiles and tile patterns need nothing else)
};

// The environment kernels' arguments (rpt_set_environment; not in the reference): PanoramaArgs with the sky image and its frame appended,
// for the same reason again.  Every environment kernel takes them, pinhole and panorama, with Doppler on or off (they carry
// `doppler` as a run-time flag: 0 there means no Doppler).
struct EnvironmentArgs : PanoramaArgs {
    const uint32_t *env_texels;     // [env_width * env_height] one dword per texel, R | G << 8 | B << 16, row 0 the top (+y)
    int env_width, env_height;
    rpt_float4 env_frame[4];        // E: camera frame -> the sky's rest frame, rows t, x, y, z (rpt_set_environment_frame)
};

// The lens kernels' arguments (rpt_set_field_of_view; not in the reference): EnvironmentArgs with the scale of the image plane appended, for
// the same reason once more.  Every lens kernel takes them: the plain ones (doppler = 0 and env_texels unused there), their Doppler
// twins and the environment forms.
struct LensArgs : EnvironmentArgs {
    float lens_scale;               // s = (float)tan(v_fov / 2): pixel (x, y) looks through (s fx2, s fy2, 0.5); 1.0f is the reference's lens
};

// One LensArgs on the host serves every render kernel (rpt_api.hip: launch): each block is a PREFIX of the next — single inheritance,
// the base at offset 0, the new fields behind it — and a kernel's launch copies its own kernarg size from the block's address.
// (RefineArgs and EventArgs below extend LensArgs in the same way.)
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(__builtin_offsetof(LensArgs, rects) == 0 && __builtin_offsetof(LensArgs, hits) + sizeof(void *) == sizeof(KernelArgs), "KernelArgs first");
static_assert(__builtin_offsetof(LensArgs, doppler) >= sizeof(KernelArgs) && __builtin_offsetof(LensArgs, debug_doppler) + sizeof(void *) == sizeof(DopplerArgs), "then DopplerArgs' fields");
static_assert(__builtin_offsetof(LensArgs, pano_cols) >= sizeof(DopplerArgs) && __builtin_offsetof(LensArgs, pano_rows) + sizeof(void *) == sizeof(PanoramaArgs), "then PanoramaArgs' fields");
static_assert(__builtin_offsetof(LensArgs, env_texels) >= sizeof(PanoramaArgs) && __builtin_offsetof(LensArgs, env_frame) + sizeof(rpt_float4[4]) == sizeof(EnvironmentArgs), "then EnvironmentArgs' fields");
static_assert(__builtin_offsetof(LensArgs, lens_scale) >= sizeof(EnvironmentArgs), "then LensArgs' own");
#pragma clang diagnostic pop

// The ray-map kernels' arguments (rpt_set_raymap; not in the reference): LensArgs with the map appended, for the same reason once more.
// Every ray-map render kernel takes them (doppler = 0 in the plain ones, lens_scale unused); the event form has a block of its own
// behind EventArgs (RaymapEventArgs below).  The map holds one float4 {p.x, p.y, p.z, 0} per pixel, row-major, row 0 the bottom, rows
// raymap_pitch pixels apart (the width rounded up to a multiple of 8): the 8 pixels a wave's tile has in one row are one aligned
// 128-byte line, read by one 16-byte-aligned vector load a lane.  p == (0, 0, 0): the pixel has no ray.  DESIGN.md "Ray-map camera".
struct RaymapArgs : LensArgs {
    const float4 *raymap;           // [raymap_pitch * height]; addressed by GLOBAL pixel (row tiles and tile patterns need nothing else)
    int raymap_pitch;
};
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winvalid-offsetof"
static_assert(__builtin_offsetof(RaymapArgs, raymap) >= sizeof(LensArgs), "RaymapArgs' own fields lie behind LensArgs");
#pragma clang diagnostic pop

struct Hit {                 // opencl_kernel.cl:38-44
    float dist;
    f3 normal;
    f2 uv;
    int object;
};

struct Ray { f3 origin, dir; };

// ---------------------------------------------------------------------------------------------
// opencl_kernel.cl:55-73
RPT_DEV f3 createCamRayDir(float x_coord, float y_coord, int width, int height, float aspect_ratio) {
    const float fx = x_coord / (float)width;
    const float fy = y_coord / (float)height;
    const float fx2 = (fx - 0.5f) * aspect_ratio;
    const float fy2 = fy - 0.5f;
    return normalize(mk3(fx2, fy2, 0.5f));
}

// The pinhole with a lens (rpt_set_field_of_view; not in the reference): createCamRayDir's fx2, fy2 as it forms them, each times s =
// (float)tan(v_fov / 2) — two more float products, nothing reassociated.  s = 1.0f makes both products exact: the reference's ray.
RPT_DEV f3 lensCamRayDir(float x_coord, float y_coord, int width, int height, float aspect_ratio, float s) {
    const float fx = x_coord / (float)width;
    const float fy = y_coord / (float)height;
    const float fx2 = (fx - 0.5f) * aspect_ratio;
    const float fy2 = fy - 0.5f;
    return normalize(mk3(s * fx2, s * fy2, 0.5f));
}

// The equirectangular camera (rpt_set_projection; not in the reference): p = (cos phi sin lambda, sin phi, cos phi cos lambda) from the
// host's tables (rpt_projection_tables: (float) sin / cos of angles evaluated in double), three float products, then the pinhole's
// normalize.  Yaw 0 looks down +z at the centre column; x grows towards +x, row 0 is the bottom.
RPT_DEV f3 equirectCamDir(const PanoramaArgs &a, int x, int y) {
    const float2 c = a.pano_cols[x];
    const float2 r = a.pano_rows[y];
    return normalize(mk3(r.y * c.x, r.x, r.y * c.y));
}

// The ray-map camera (rpt_set_raymap; not in the reference): the map's entry of pixel (x, y), then the pinhole's normalize.  The load is
// one 16-byte read per lane; a wave's 8 x 8 tile reads eight whole 128-byte lines.  (0, 0, 0) = no ray: the caller must not normalise it.
RPT_DEV float4 raymapLoad(const float4 *map, int pitch, int x, int y) { return map[(size_t)y * (size_t)pitch + (size_t)x]; }
RPT_DEV bool raymapHasRay(float4 p) { return !(p.x == 0.0f && p.y == 0.0f && p.z == 0.0f); }

// opencl_kernel.cl:106-126
RPT_DEV bool intersect_triangle(f3 A, f3 B, f3 C, const Ray &ray, float &dist, f2 &uv) {
    const f3 v0v1 = B - A;
    const f3 v0v2 = C - A;
    const f3 pvec = cross(ray.dir, v0v2);
    const float det = dot(v0v1, pvec);
    if (det < RPT_EPSILON && -RPT_EPSILON < det) return false;
    const float invDet = 1 / det;
    const f3 tvec = ray.origin - A;
    uv.x = dot(tvec, pvec) * invDet;
    if (uv.x < 0 || uv.x > 1) return false;
    const f3 qvec = cross(tvec, v0v1);
    uv.y = dot(ray.dir, qvec) * invDet;
    if (uv.y < 0 || uv.x + uv.y > 1) return false;
    dist = dot(v0v2, qvec) * invDet;
    return true;
}

// opencl_kernel.cl:128-170.  bounds[sign] is written as a select so nothing is indexed dynamically.
RPT_DEV bool intersect_AABB(f3 bmin, f3 bmax, const Ray &ray, f2 &d, int &closeSide, int &farSide) {
    const f3 origin = ray.origin;
    const f3 inv_dir = mk3(1.0f / ray.dir.x, 1.0f / ray.dir.y, 1.0f / ray.dir.z);
    const int sx = inv_dir.x < 0 ? 1 : 0, sy = inv_dir.y < 0 ? 1 : 0, sz = inv_dir.z < 0 ? 1 : 0;
    d.x = ((sx ? bmax.x : bmin.x) - origin.x) * inv_dir.x;
    d.y = ((sx ? bmin.x : bmax.x) - origin.x) * inv_dir.x;
    closeSide = 2 + sx;
    farSide = 3 - sx;
    const float tymin = ((sy ? bmax.y : bmin.y) - origin.y) * inv_dir.y;
    const float tymax = ((sy ? bmin.y : bmax.y) - origin.y) * inv_dir.y;
    if ((d.x > tymax) || (tymin > d.y)) return false;
    if (tymin > d.x) { d.x = tymin; closeSide = 4 + sy; }
    if (tymax < d.y) { d.y = tymax; farSide = 5 - sy; }
    const float tzmin = ((sz ? bmax.z : bmin.z) - origin.z) * inv_dir.z;
    const float tzmax = ((sz ? bmin.z : bmax.z) - origin.z) * inv_dir.z;
    if ((d.x > tzmax) || (tzmin > d.y)) return false;
    if (tzmin > d.x) { d.x = tzmin; closeSide = sz; }
    if (tzmax < d.y) { d.y = tzmax; farSide = 1 - sz; }
    return d.y > 0;
}

// opencl_kernel.cl:172-198 with the direction reciprocals and signs hoisted out of the leaf walk
// (scaledDir is constant along one traversal, so 1/scaledDir is computed once: same values).
struct ExitPlan { f3 scaledDir, inv_dir; int sx, sy, sz; };

RPT_DEV ExitPlan makeExitPlan(f3 scaledDir) {
    ExitPlan p;
    p.scaledDir = scaledDir;
    p.inv_dir = mk3(1.0f / scaledDir.x, 1.0f / scaledDir.y, 1.0f / scaledDir.z);
    p.sx = p.inv_dir.x < 0;
    p.sy = p.inv_dir.y < 0;
    p.sz = p.inv_dir.z < 0;
    return p;
}

// The same step for a walk that cannot afford the plan's hoisted face ids (KernelPolicy::park_bystanders: 3 - sx, 5 - sy and 1 - sz are
// loop invariants, and what a compiler keeps of them across the leaf loop at 80 registers it keeps in scratch).  The three far-plane
// bits 1 - s travel in ONE register, and the id is formed in the branch that picks it: 2 + bit, 4 + bit, bit — the integers above.
struct ExitPlanBits { f3 scaledDir, inv_dir; int far_bits; };      // far_bits = (1 - sx) | (1 - sy) << 1 | (1 - sz) << 2

RPT_DEV ExitPlanBits makeExitPlanBits(f3 scaledDir) {
    const ExitPlan q = makeExitPlan(scaledDir);
    ExitPlanBits p;
    p.scaledDir = q.scaledDir;
    p.inv_dir = q.inv_dir;
    p.far_bits = (1 - q.sx) | ((1 - q.sy) << 1) | ((1 - q.sz) << 2);
    return p;
}

RPT_DEV int getOppositeBoxSide(const ExitPlanBits &p, f3 &uv) {
    const int bx = p.far_bits & 1, by = (p.far_bits >> 1) & 1, bz = p.far_bits >> 2;
    const float dx = ((float)bx - uv.x) * p.inv_dir.x;
    const float dy = ((float)by - uv.y) * p.inv_dir.y;
    const float dz = ((float)bz - uv.z) * p.inv_dir.z;
    // (the branches pick two immediates, the axis' first id and its bit's place; 2 + bx written in the branch would be a loop invariant
    // again and be hoisted like the ids of the form below)
    float t;
    int first, place;
    if (dx < dy) {
        if (dx < dz) { t = dx; first = 2; place = 0; } else { t = dz; first = 0; place = 2; }
    } else {
        if (dy < dz) { t = dy; first = 4; place = 1; } else { t = dz; first = 0; place = 2; }
    }
    uv = uv + p.scaledDir * t;
    return first + ((p.far_bits >> place) & 1);
}

RPT_DEV int getOppositeBoxSide(const ExitPlan &p, f3 &uv) {
    const float dx = ((float)(1 - p.sx) - uv.x) * p.inv_dir.x;
    const float dy = ((float)(1 - p.sy) - uv.y) * p.inv_dir.y;
    const float dz = ((float)(1 - p.sz) - uv.z) * p.inv_dir.z;
    float t;
    int side;
    if (dx < dy) {
        if (dx < dz) { t = dx; side = 3 - p.sx; } else { t = dz; side = 1 - p.sz; }
    } else {
        if (dy < dz) { t = dy; side = 5 - p.sy; } else { t = dz; side = 1 - p.sz; }
    }
    uv = uv + p.scaledDir * t;
    return side;
}

// The same step for the common case 0 <= uv < 1.5 on every axis (+0 included, -0/NaN/negative excluded by
// the unsigned compare on the bit patterns): there round(c) is (c >= 0.5), min(c, 1-eps) keeps that bit, and
// 2*fmod(m, 0.5) is 2*(m - 0.5*bit) — every operation exact, so the results are those of the general form.
RPT_DEV int octree_child_step(f3 &uv);
RPT_DEV int octree_child_step_fast(f3 &uv) {
    const unsigned int lim = 0x3FC00000u;   // 1.5f
    const bool in_range = (__float_as_uint(uv.x) < lim) && (__float_as_uint(uv.y) < lim) && (__float_as_uint(uv.z) < lim);
    if (!in_range) return octree_child_step(uv);
    const float top = 1.0f - RPT_EPSILON;
    const bool bx = uv.x >= 0.5f, by = uv.y >= 0.5f, bz = uv.z >= 0.5f;
    const float mx = top < uv.x ? top : uv.x, my = top < uv.y ? top : uv.y, mz = top < uv.z ? top : uv.z;
    uv.x = 2.0f * (mx - (bx ? 0.5f : 0.0f));
    uv.y = 2.0f * (my - (by ? 0.5f : 0.0f));
    uv.z = 2.0f * (mz - (bz ? 0.5f : 0.0f));
    return (bz ? 1 : 0) + (by ? 2 : 0) + (bx ? 4 : 0);
}

// child selection and re-normalisation of opencl_kernel.cl:237-238 / 257-258
RPT_DEV int octree_child_step(f3 &uv) {
    const float fidx = __builtin_roundf(uv.z) + 2 * __builtin_roundf(uv.y) + 4 * __builtin_roundf(uv.x);
    const int childIndex = !(fidx >= 0.0f) ? 0 : (fidx > 7.0f ? 7 : (int)fidx);
    uv.x = 2.0f * fmod_half(cl_min(uv.x, 1.0f - RPT_EPSILON));
    uv.y = 2.0f * fmod_half(cl_min(uv.y, 1.0f - RPT_EPSILON));
    uv.z = 2.0f * fmod_half(cl_min(uv.z, 1.0f - RPT_EPSILON));
    return childIndex;
}

// ---- octree storage policies -------------------------------------------------------------------
// Node<0>: the reference's 96-B nodes read field by field (a traversal step needs min/max,
//          (trisIndex,trisCount), children[0], one children[k] and one neighbors[k], not the whole
//          struct the reference copies).  Works for any valid octree.
// (The derived 64-B DNode + gathered DTri records are read by octree_walk below, record by record.)
typedef float v4f __attribute__((ext_vector_type(4)));   // native vectors: one 16-B load, SROA-friendly
typedef int v4i __attribute__((ext_vector_type(4)));
template <int V> struct NodeRef;

template <> struct NodeRef<0> {
    int idx;
    RPT_DEV void load(const KernelArgs &a, int i) { idx = i; }
    RPT_DEV f3 bmin(const KernelArgs &a) const { return ld3(a.octrees[idx].min); }
    RPT_DEV f3 bmax(const KernelArgs &a) const { return ld3(a.octrees[idx].max); }
    RPT_DEV bool is_leaf(const KernelArgs &a) const { return a.octrees[idx].children[0] == -1; }
    RPT_DEV int child(const KernelArgs &a, int k) const { return a.octrees[idx].children[k]; }
    RPT_DEV int neighbor(const KernelArgs &a, int side) const { return a.octrees[idx].neighbors[side]; }
    RPT_DEV int tri_begin(const KernelArgs &a) const { return a.octrees[idx].trisIndex; }
    RPT_DEV int tri_count(const KernelArgs &a) const { return a.octrees[idx].trisCount; }
    // triangle k of the leaf: A, B-A, C-A and its id
    RPT_DEV void tri(const KernelArgs &a, int k, f3 &A, f3 &v0v1, f3 &v0v2, int &id) const {
        id = a.octreeTris[k];
        A = ld3(a.vertices[a.triangles[9 * id + 3 * 0]]);
        const f3 B = ld3(a.vertices[a.triangles[9 * id + 3 * 1]]);
        const f3 C = ld3(a.vertices[a.triangles[9 * id + 3 * 2]]);
        v0v1 = B - A;
        v0v2 = C - A;
    }
};
// opencl_kernel.cl:106-126 with the two edge vectors supplied.  EXACT_RCP: 1 / det through rcp_exact (rpt_device_math.hip.h), the
// same float on the domain 2^-125 <= |det| <= 2^125.  The line above it leaves |det| >= 1e-7 > 2^-24; the ray's direction is
// normalised (intersect_object / intersect_object_primary), so |det| <= |e1| |e2| (1 + 2^-20) with e1, e2 the record's edges, and
// the host instantiates this form only for scenes whose triangles all have |e1| |e2| <= 2^60 (rpt_upload_scene: exact_rcp_ok).
// A NaN det (a NaN vertex or direction) passes the line above as before; both forms then give a NaN invDet, a NaN dist, and
// test_tri_rec's 0 <= dist rejects the triangle either way (uv's NaN never leaves this function).  So on every mesh that selects
// it the observable result is the IEEE form's.
template <bool EXACT_RCP = false>
RPT_DEV bool intersect_triangle_edges(f3 A, f3 v0v1, f3 v0v2, const Ray &ray, float &dist, f2 &uv) {
    const f3 pvec = cross(ray.dir, v0v2);
    const float det = dot(v0v1, pvec);
    if (det < RPT_EPSILON && -RPT_EPSILON < det) return false;
    const float invDet = EXACT_RCP ? rcp_exact(det) : 1 / det;
    const f3 tvec = ray.origin - A;
    uv.x = dot(tvec, pvec) * invDet;
    if (uv.x < 0 || uv.x > 1) return false;
    const f3 qvec = cross(tvec, v0v1);
    uv.y = dot(ray.dir, qvec) * invDet;
    if (uv.y < 0 || uv.x + uv.y > 1) return false;
    dist = dot(v0v2, qvec) * invDet;
    return true;
}
// The walk's stop test (opencl_kernel.cl:283): length(exit point - origin) > hit.dist.  Until a triangle has been hit,
// hit.dist is the caller's 1e20f, and sqrt(s) > 1e20f holds for no finite float s (sqrt(FLT_MAX) < 1.9e19), for s = +inf
// only, and not for NaN: so while no lane of the wave has a hit the square root is not needed to decide it — same answer.
RPT_DEV bool exit_is_past_hit(f3 v, float hit_dist, bool didHit) {
    const float s = dot(v, v);
    if (__ballot(didHit) == 0ull && hit_dist == 1e20f) return s == __builtin_inff();
    return __builtin_sqrtf(s) > hit_dist;
}
// opencl_kernel.cl:287-306: normal, texture coordinates and the distance re-measured in the caller's frame, from the walk's
// closest triangle (hit.dist parametric, hit.uv barycentric on entry).  HIT_RECORD: the fifteen floats from the triangle's DHit (the
// derived layouts' walk); otherwise through triangles[] into normals[] / uvs[] (the reference's layouts, the persistent kernels) — the
// same floats either way, and the same arithmetic on them.
template <bool HIT_RECORD = false>
RPT_DEV void mesh_hit_finish(const KernelArgs &a, const rpt_object &obj, f3 origin, f3 dir, int hitTri, f3 world_origin,
                             float world_dirlen, Hit &hit) {
    const float u = hit.uv.x, v = hit.uv.y;
    const float w = 1.0f - u - v;
    f3 normA, normB, normC;
    rpt_float2 uvA, uvB, uvC;
    if (HIT_RECORD) {
        const v4f *p = reinterpret_cast<const v4f *>(a.hits + hitTri);
        const v4f h0 = p[0], h1 = p[1], h2 = p[2], h3 = p[3];
        normA = mk3(h0.x, h0.y, h0.z);
        normB = mk3(h0.w, h1.x, h1.y);
        normC = mk3(h1.z, h1.w, h2.x);
        uvA.x = h2.y; uvA.y = h2.z;
        uvB.x = h2.w; uvB.y = h3.x;
        uvC.x = h3.y; uvC.y = h3.z;
    } else {
        normA = ld3(a.normals[a.triangles[2 + 9 * hitTri + 3 * 0]]);
        normB = ld3(a.normals[a.triangles[2 + 9 * hitTri + 3 * 1]]);
        normC = ld3(a.normals[a.triangles[2 + 9 * hitTri + 3 * 2]]);
        uvA = a.uvs[a.triangles[1 + 9 * hitTri + 3 * 0]];
        uvB = a.uvs[a.triangles[1 + 9 * hitTri + 3 * 1]];
        uvC = a.uvs[a.triangles[1 + 9 * hitTri + 3 * 2]];
    }
    hit.normal = normalize(applyTranspose(obj.InvM, normA * w + normB * u + normC * v));
    hit.uv.x = w * uvA.x + u * uvB.x + v * uvC.x;
    hit.uv.y = w * uvA.y + u * uvB.y + v * uvC.y;
    const f3 objPoint = origin + dir * hit.dist;
    const f3 worldPoint = transformPoint(obj.M, objPoint);
    hit.dist = length(worldPoint - world_origin) / world_dirlen;
}

// opencl_kernel.cl:200-308 on the reference's own layouts (any valid octree; the fallback kernel, variant 1): from the point
// where the ray is in object space.  newRay = object-space ray (direction normalised); world_origin/world_dirlen are
// ray->origin.yzw and |ray->dir.yzw|.
RPT_DEV bool octree_core_ref(const KernelArgs &a, const rpt_object &obj, const Ray &newRay, f3 world_origin, float world_dirlen, Hit &hit) {
    NodeRef<0> node;
    int currOctreeIndex = obj.meshIndex;
    node.load(a, currOctreeIndex);
    f2 d;
    int closeSide, farSide;
    f3 nmin = node.bmin(a), nmax = node.bmax(a);
    if (!intersect_AABB(nmin, nmax, newRay, d, closeSide, farSide)) return false;
    f3 uv = newRay.origin + newRay.dir * d.x;
    if (d.x < 0) {   // ray starts inside the root: descend to the leaf holding the origin
        uv = (newRay.origin - nmin) / (nmax - nmin);
        while (!node.is_leaf(a)) {
            currOctreeIndex = node.child(a, octree_child_step(uv));
            node.load(a, currOctreeIndex);
        }
        nmin = node.bmin(a);
        nmax = node.bmax(a);
        if (!intersect_AABB(nmin, nmax, newRay, d, closeSide, farSide)) return false;
        uv = newRay.origin + newRay.dir * d.x;
    }
    const ExitPlan plan = makeExitPlan(normalize(newRay.dir / (nmax - nmin)));
    bool didHit = false;
    int hitTri = 0;
    int steps = 0;
    while (currOctreeIndex != -1) {
        if (++steps > RPT_MAX_LEAF_STEPS) break;
        node.load(a, currOctreeIndex);
        nmin = node.bmin(a);
        nmax = node.bmax(a);
        uv = (uv - nmin) / (nmax - nmin);
        while (!node.is_leaf(a)) {
            currOctreeIndex = node.child(a, octree_child_step(uv));
            node.load(a, currOctreeIndex);
            nmin = node.bmin(a);
            nmax = node.bmax(a);
        }
        const int trisIndex = node.tri_begin(a);
        const int trisEnd = trisIndex + node.tri_count(a);
        for (int i = trisIndex; i < trisEnd; i++) {
            f3 A, v0v1, v0v2;
            int tri;
            node.tri(a, i, A, v0v1, v0v2, tri);
            float dist;
            f2 triUV;
            if (intersect_triangle_edges(A, v0v1, v0v2, newRay, dist, triUV)) {
                if (0 <= dist && dist < hit.dist) {
                    hitTri = tri;
                    hit.dist = dist;
                    hit.uv = triUV;
                    didHit = true;
                }
            }
        }
        const f3 extents = nmax - nmin;
        farSide = getOppositeBoxSide(plan, uv);
        uv = nmin + uv * extents;
        currOctreeIndex = node.neighbor(a, farSide);
        if (exit_is_past_hit(uv - newRay.origin, hit.dist, didHit)) break;
    }
    if (!didHit) return false;
    mesh_hit_finish(a, obj, newRay.origin, newRay.dir, hitTri, world_origin, world_dirlen, hit);
    return true;
}

// ---- the walk on the derived layouts (what ships) -------------------------------------------------------------------------
// opencl_kernel.cl:200-308 once more, arithmetic unchanged; what is organised for the machine is WHEN memory is asked for — a
// leaf step of the reference's loop is a chain of dependent round trips (node, one per descent level, one per triangle, the
// neighbour), and with five waves on a SIMD the waves wait on exactly that chain (profiles/r02_*_pmc_summary.json: half of their
// life), so the chain is made shorter, not the traffic smaller:
//   * a node is read as ONE 64-B record (box, link, first triangle, count), a triangle as one 40-B record (A, B-A, C-A, id);
//   * a descent reads 4 bytes per level from the compact link array, and the parent's link says which children are leaves, so no
//     level is spent on finding that out;
//   * the exit face of a leaf does not depend on its triangles (getOppositeBoxSide works on the ray and the entry point alone):
//     it is found BEFORE the triangle loop, and the neighbour's index travels while the triangles are tested;
//   * the latency form (LATENCY; kernel 43: the blocking call, whose frame is as long as its longest wave, and small frames in flight):
//     triangle records are asked for one iteration ahead, and a leaf's first record together with its node record
//     (load_first_tri).  Ten more live registers: 44 B of scratch at five waves per SIMD, worth it where frames wait for
//     latency (bunny 4K one frame at a time 0.196 -> 0.186 ms, 1080p 0.166 -> 0.151), not where the chip is full of walks
//     (4K in flight 0.088 -> 0.095 ms per frame): profiles/r03_walk_ab.txt, r03_latency_walk_ab.txt.
// Measured against round 2's walk (profiles/r03_walk_ab.txt): bunny 4K 0.0949 -> 0.0903 ms per frame in flight, 0.201 -> 0.191
// one at a time; zero scratch instead of 12 B.  What was tried on top and lost is in the diagnostics build (rpt_diag_walks.hip.h).
// hi.w of a node record = leafBegin | min(leafCount, 255) << 24 (build_derived_geometry): the count of a leaf's list travels with the
// box, so a node visit of the throughput walk is two 16-B loads, not three instructions; a list of 255 or more reads the full count
// from its own field, and so does the latency walk always (PACKED_COUNT = false: see octree_walk).
#define RPT_NODE_BEGIN_MASK 0x00ffffff
struct NodeRec { v4f lo, hi; int count; };
template <bool PACKED_COUNT = true>
RPT_DEV NodeRec load_node_rec(const KernelArgs &a, int i) {
    const v4f *p = reinterpret_cast<const v4f *>(a.dnodes + i);
    NodeRec r;
    r.lo = p[0];
    r.hi = p[1];
    if (PACKED_COUNT) {
        r.count = (int)(__float_as_uint(r.hi.w) >> 24);
        if (r.count == 255) r.count = a.dnodes[i].leafCount;
    } else {
        r.count = a.dnodes[i].leafCount;
    }
    return r;
}
struct TriRec { v4f t0, t1; float e2z; int tri; };
// LATE_ID: the triangle's id is not read with every record tested (9 dwords instead of 10 through the L1's return path, which is what
// frames in flight wait for: profiles/r03_td_bound.txt) — the walk remembers the RECORD it hit and reads that one id at the end.
template <bool LATE_ID = false>
RPT_DEV TriRec load_tri_rec(const KernelArgs &a, int k) {
    const v4f *p = reinterpret_cast<const v4f *>(a.dtris + k);
    TriRec r;
    r.t0 = p[0];
    r.t1 = p[1];
    if (LATE_ID) {
        r.e2z = *reinterpret_cast<const float *>(p + 2);
        r.tri = k;
    } else {
        const float2 t2 = *reinterpret_cast<const float2 *>(p + 2);
        r.e2z = t2.x;
        r.tri = __float_as_int(t2.y);
    }
    return r;
}
// The first record of a node's list, by NODE index (48 B per node, zeros where the list is empty): its address is known as soon as
// the node's is, so the latency walk asks for it together with the node record — one exposed round trip less per non-empty leaf,
// 48 B more asked of the L1 per node visited.
template <bool LATE_ID = false>
RPT_DEV TriRec load_first_tri(const KernelArgs &a, int node) {
    const v4f *p = reinterpret_cast<const v4f *>(a.first_tris + node);
    TriRec r;
    r.t0 = p[0];
    r.t1 = p[1];
    if (LATE_ID) {
        r.e2z = *reinterpret_cast<const float *>(p + 2);
        r.tri = 0;          // (the walk puts the record's index in when it tests the record)
    } else {
        const float2 t2 = *reinterpret_cast<const float2 *>(p + 2);
        r.e2z = t2.x;
        r.tri = __float_as_int(t2.y);
    }
    return r;
}
template <bool EXACT_RCP = false>
RPT_DEV void test_tri_rec(const TriRec &r, const Ray &ray, Hit &hit, int &hitTri, bool &didHit) {
    float dist;
    f2 triUV;
    if (intersect_triangle_edges<EXACT_RCP>(mk3(r.t0.x, r.t0.y, r.t0.z), mk3(r.t0.w, r.t1.x, r.t1.y), mk3(r.t1.z, r.t1.w, r.e2z), ray, dist, triUV)) {
        if (0 <= dist && dist < hit.dist) {
            hitTri = r.tri;
            hit.dist = dist;
            hit.uv = triUV;
            didHit = true;
        }
    }
}

// from an inner node (link != -1) down to the leaf that holds uv (opencl_kernel.cl:256-261: the same child steps)
RPT_DEV int descend_to_leaf(const KernelArgs &a, int link, f3 &uv) {
    int idx;
    for (;;) {
        const int k = octree_child_step_fast(uv);
        idx = (link & RPT_LINK_CHILD_MASK) + k;
        if ((link >> (24 + k)) & 1) break;          // the link says this child is a leaf: no lookup
        link = a.links[idx];
    }
    return idx;
}

// The two forms the kernels use; both read the triangle's id late (load_tri_rec<true>: the walk remembers the RECORD it hit).
//   throughput (LATENCY = false; kernels 41 / 48): one record at a time, the leaf count packed with the box;
//   latency (LATENCY = true; kernels 43 / 49): records an iteration ahead, a leaf's first record with its node record, the count from
//   its own field (the packed count pays in the throughput walk — one instruction less per node visit, -0.5...-1 % — and costs the
//   latency walk 2-4.5 %, whose count then sits behind a shift and a compare instead of arriving beside the box:
//   profiles/r03_packed_count_ab.txt).
// EXACT_RCP: the triangle test's 1 / det without the IEEE scaling (intersect_triangle_edges); the host selects it per scene.
// EXITS: a leaf is left through its exit record (DExit: the neighbour's box, index or link and begin word from ONE address, asked for
// after the triangle loop) instead of nb[] and then the neighbour's node record; the "no neighbour" break moves behind that load.
// The throughput walk takes it; the latency walk does not: there the record arrives a hop before first_tris can be asked for, and
// kernel 43 lost 10 % on bunny 1080p in flight with it (profiles/r16_exit_hit_ab.txt).
// FACE_BITS: the exit plan without hoisted face ids (ExitPlanBits above); kernel 41's throughput walk only.
template <bool LATENCY, bool EXACT_RCP, bool FACE_BITS = false, bool EXITS = (RPT_EXIT_RECORDS != 0) && !LATENCY>
RPT_DEV bool octree_walk(const KernelArgs &a, const rpt_object &obj, int root, const Ray &newRay, f3 world_origin,
                         float world_dirlen, Hit &hit) {
    static_assert(!(EXITS && LATENCY), "exit records: the throughput walk only");
    static_assert(!(FACE_BITS && LATENCY), "the latency walk keeps its plan");
    int curr = root;
    NodeRec rec = load_node_rec<!LATENCY>(a, curr);
    f2 d;
    int closeSide, farSide;
    f3 nmin = mk3(rec.lo.x, rec.lo.y, rec.lo.z), nmax = mk3(rec.hi.x, rec.hi.y, rec.hi.z);
    if (!intersect_AABB(nmin, nmax, newRay, d, closeSide, farSide)) return false;
    f3 uv = newRay.origin + newRay.dir * d.x;
    if (d.x < 0) {   // ray starts inside the root: descend to the leaf holding the origin
        uv = (newRay.origin - nmin) / (nmax - nmin);
        if (__float_as_int(rec.lo.w) != -1) {
            curr = descend_to_leaf(a, __float_as_int(rec.lo.w), uv);
            rec = load_node_rec<!LATENCY>(a, curr);
        }
        nmin = mk3(rec.lo.x, rec.lo.y, rec.lo.z);
        nmax = mk3(rec.hi.x, rec.hi.y, rec.hi.z);
        if (!intersect_AABB(nmin, nmax, newRay, d, closeSide, farSide)) return false;
        uv = newRay.origin + newRay.dir * d.x;
    }
    const f3 planDir = normalize(newRay.dir / (nmax - nmin));
    const auto plan = [&] { if constexpr (FACE_BITS) return makeExitPlanBits(planDir); else return makeExitPlan(planDir); }();
    bool didHit = false;
    int hitTri = 0;
    TriRec first;
    if (LATENCY) first = load_first_tri<true>(a, curr);
    for (int steps = 1; steps <= RPT_MAX_LEAF_STEPS; steps++) {
        nmin = mk3(rec.lo.x, rec.lo.y, rec.lo.z);
        nmax = mk3(rec.hi.x, rec.hi.y, rec.hi.z);
        uv = (uv - nmin) / (nmax - nmin);
        if (__float_as_int(rec.lo.w) != -1) {
            // (only a walk's first step can stand on a root: nobody's neighbour link points at one)
            curr = descend_to_leaf(a, __float_as_int(rec.lo.w), uv);
            rec = load_node_rec<!LATENCY>(a, curr);
            if (LATENCY) first = load_first_tri<true>(a, curr);
            nmin = mk3(rec.lo.x, rec.lo.y, rec.lo.z);
            nmax = mk3(rec.hi.x, rec.hi.y, rec.hi.z);
        }
        int i = __float_as_int(rec.hi.w) & RPT_NODE_BEGIN_MASK;
        const int trisEnd = i + rec.count;
        farSide = getOppositeBoxSide(plan, uv);             // the way out, before the triangles
        int next = 0;
        if (!EXITS) next = a.dnodes[curr].nb[farSide];
        if (LATENCY) {
            if (i < trisEnd) {
                TriRec cur = first;
                for (; i < trisEnd; i++) {
                    TriRec nxt = cur;
                    if (i + 1 < trisEnd) nxt = load_tri_rec<true>(a, i + 1);
                    cur.tri = i;
                    test_tri_rec<EXACT_RCP>(cur, newRay, hit, hitTri, didHit);     // (the record was asked for an iteration ago: only the arithmetic is saved here)
                    cur = nxt;
                }
            }
        } else {
            for (; i < trisEnd; i++) test_tri_rec<EXACT_RCP>(load_tri_rec<true>(a, i), newRay, hit, hitTri, didHit);
        }
        uv = nmin + uv * (nmax - nmin);
        if (EXITS) {
            const v4f *p = reinterpret_cast<const v4f *>(a.exits + (curr * 6 + farSide));
            const v4f lo = p[0], hi = p[1];
            const int ea = __float_as_int(lo.w), eb = __float_as_int(hi.w);
            if (exit_is_past_hit(uv - newRay.origin, hit.dist, didHit) || ea == -1) break;
            const bool inner = eb == RPT_EXIT_INNER;
            curr = ea;                                      // (an inner neighbour: its link, until the descent above names the leaf)
            rec.lo = lo;
            rec.hi = hi;
            rec.lo.w = __int_as_float(inner ? ea : -1);
            rec.count = (int)((unsigned int)eb >> 24);      // (RPT_EXIT_INNER: 1, and the descent loads the leaf's own record)
            if (rec.count == 255) rec.count = a.dnodes[curr].leafCount;
            continue;
        }
        if (exit_is_past_hit(uv - newRay.origin, hit.dist, didHit) || next == -1) break;
        curr = next;
        rec = load_node_rec<!LATENCY>(a, curr);
        if (LATENCY) first = load_first_tri<true>(a, curr);
    }
    if (!didHit) return false;
    hitTri = a.dtris[hitTri].tri;
    mesh_hit_finish<RPT_HIT_RECORDS != 0>(a, obj, newRay.origin, newRay.dir, hitTri, world_origin, world_dirlen, hit);
    return true;
}

#ifdef RPT_DIAGNOSTICS
}  // namespace rptd
#include "rpt_diag_walks.hip.h"      /* librpt_hip_diag.so only: round 2's walk with its instrumentation, the experiment arms */
namespace rptd {
#endif

// ---- what a render kernel is: its policy, a type of static constexpr members that render_pixel_body and everything it calls read.
// KernelPolicy holds the defaults (kernel 48); each product kernel below derives its own; the diagnostics build adds DiagPolicy<N>
// (rpt_diag_kernels.hip.h).  rpt_api.hip's tables name one kernel per (camera, colour, form) and pin band_first(Form) against these types.
enum class Walk {
    reference,       // octree_core_ref on the reference's layouts (any valid octree)
    none,            // no octree walk compiled in: for Object[]s without a mesh
    throughput,      // octree_walk<false, ...>: one record at a time, the packed leaf count
    latency,         // octree_walk<true, ...>: records an iteration ahead, a leaf's first record with its node record
};
enum class Camera {
    pinhole,         // createCamRayDir: the reference's image plane z = 0.5
    equirect,        // equirectCamDir: the panorama tables (rpt_set_projection); the arguments are a PanoramaArgs
    lens,            // lensCamRayDir: the pinhole's image plane scaled by LensArgs::lens_scale (rpt_set_field_of_view); the arguments are a LensArgs
    raymap,          // raymapLoad: one direction per pixel from the context's map (rpt_set_raymap); the arguments are a RaymapArgs (events: RaymapEventArgs)
};
struct KernelPolicy {
    static constexpr Walk walk = Walk::throughput;
    static constexpr Camera camera = Camera::pinhole;
    static constexpr bool exact_rcp = false;     // the triangle test's 1 / det through rcp_exact (the host picks it per scene)
    static constexpr bool culled = true;         // the wave's object mask (wave_object_mask) and the shadow-segment culls
    static constexpr bool object_mask = true;    // ... of which the object mask, proven on the pinhole's image plane only (culled && object_mask)
    static constexpr bool tile_bits = true;      // ... which the tile bitmaps of the still meshes thin out further (clear_empty_tiles; needs culled && object_mask)
    static constexpr bool band_first = false;    // the band of tile rows that holds the meshes is dispatched first (KernelArgs::first_h)
    static constexpr bool one_wave = true;       // one wave (an 8x8 tile) per workgroup, not four (a 32x8 strip)
    static constexpr bool doppler = false;       // the Doppler twin (rpt_set_doppler; the arguments are a DopplerArgs)
    static constexpr bool drec = false;          // ... that also writes the per-pixel Doppler record (the debug kernel only)
    static constexpr bool environment = false;   // a pixel that hits nothing looks the sky image up (rpt_set_environment; the arguments are an EnvironmentArgs)
    static constexpr bool park_bystanders = false;   // kernels 41 and 48 alone: what is live across a shadow walk and not read by it waits in LDS (park_put / park_get), the exit plan keeps no face ids
    static constexpr bool windowed = false;      // every hit, occluder and light is held against its object's time window (rpt_set_object_windows; DObj::win_t0, win_t1)
    static constexpr int diag = 0;               // the measurement arm's number (diagnostics build only); 0 in every product policy
};
struct RefLayout : KernelPolicy { static constexpr Walk walk = Walk::reference; static constexpr bool culled = false; };        // 1
struct Unculled : KernelPolicy { static constexpr bool culled = false; };                                                       // 3, 47
struct Ballot : KernelPolicy {};                                                                                                // 48, 46, 50, 51
struct BallotExact : Ballot { static constexpr bool exact_rcp = true; };                                                        // (41's policy but for the parking: 241, 341, 941, ...)
struct BallotExactParked : BallotExact { static constexpr bool park_bystanders = true; };                                       // 41
struct BallotParked : Ballot { static constexpr bool park_bystanders = true; };                                                 // 48
struct BallotFirst : KernelPolicy { static constexpr Walk walk = Walk::latency; static constexpr bool band_first = true; };     // 49
struct BallotFirstExact : BallotFirst { static constexpr bool exact_rcp = true; };                                              // 43
struct Analytic : KernelPolicy { static constexpr Walk walk = Walk::none; static constexpr bool tile_bits = false; };           // 44 (no mesh, no bitmap)
template <class P> struct DopplerTwin : P { static constexpr bool doppler = true; };                                            // 2xx, 5xx
struct DopplerRecorded : DopplerTwin<Unculled> { static constexpr bool drec = true; };                                          // 240
// the panorama kernels (rpt_set_projection): the equirectangular camera, no object mask (its regions live on the pinhole's plane), the
// shadow-segment culls kept (they do not depend on the camera)
template <class P> struct Panorama : P { static constexpr Camera camera = Camera::equirect; static constexpr bool object_mask = false; };
struct PanoramaWalk : Panorama<BallotExact> {};                                                                                 // 341
struct PanoramaWalkIeee : Panorama<Ballot> {};                                                                                  // (341 outside the domain)
struct PanoramaAnalytic : Panorama<Analytic> {};                                                                                // 344
struct PanoramaUnculled : Panorama<Unculled> {};                                                                                // 303
struct PanoramaRecorded : Panorama<DopplerRecorded> {};                                                                         // 540
// the environment kernels (rpt_set_environment): one family for Doppler off and on — the twin's code with EnvironmentArgs::doppler as a
// run-time flag; with flags 0 S_f is the identity (doppler_colour returns its colour untouched), so the frame is the plain kernel's
template <class P> struct Environment : DopplerTwin<P> { static constexpr bool environment = true; };                           // 6xx, 7xx
// the lens kernels (rpt_set_field_of_view): the pinhole's kernels with the image plane — the camera ray's and the wave's tile in the object
// mask alike — scaled by LensArgs::lens_scale; everything else is the policy they derive from.  803 / 841 / 843 / 844: Lens<P> for the
// plain kernels; + 10: Lens<DopplerTwin<P>> for their Doppler twins; + 20: Lens<Environment<P>> for the environment forms
template <class P> struct Lens : P { static constexpr Camera camera = Camera::lens; };                                          // 8xx
// the ray-map kernels (rpt_set_raymap): a per-pixel direction read from the map; like the panorama no object mask (the regions live on the
// pinhole's plane) and with it no tile bitmaps, the shadow-segment culls kept.  1203 / 1241 / 1244: Raymap<P> for the plain kernels; + 10:
// DopplerTwin<Raymap<P>>; + 20: Environment<Raymap<P>>
template <class P> struct Raymap : P { static constexpr Camera camera = Camera::raymap; static constexpr bool object_mask = false; static constexpr bool tile_bits = false; };   // 12xx

// the windowed kernels (rpt_set_object_windows): the policy they wrap with the three window tests compiled in (trace, sample_light_occluded,
// events_pixel_body).  Wrapped are the lens kernels (which serve the pinhole at lens_scale 1.0f: the same bytes), the panorama's and the
// ray map's; the colour is the Doppler twin with DopplerArgs::doppler as a run-time flag (0: the plain kernel's frame, as in the sky
// family) or the sky.  2000 + the wrapped row's variant.  DESIGN.md "Time windows".
template <class P> struct Windowed : P { static constexpr bool windowed = true; };                                              // 2xxx

// The kernels a sky split may launch over the object box alone (rpt_api.hip: launch): the plain pinhole colour kernels
// with the wave's object mask in natural tile order — 41, 44 and the IEEE form 48.  They add KernelArgs::tile_x0 to the workgroup's
// column; every other kernel's code stays what it was: the band-first kernels 43 / 49, which serve the blocking call and small frames,
// where a split loses (§6.2d), and the relaxed build's two (variants 50 / 51).
#ifdef RPT_RELAXED_FP
template <class P> constexpr bool tile_origin_policy = false;
#else
template <class P> constexpr bool tile_origin_policy = P::one_wave && P::culled && P::object_mask && P::camera == Camera::pinhole && !P::doppler && !P::environment && !P::windowed && !P::band_first && P::diag == 0;
#endif

// in(W, t) of DESIGN.md "Time windows": written with two negated compares so that a NaN time, and the default (-inf, +inf), accept
RPT_DEV bool window_accepts(const DObj &pre, float t) { return !(t < pre.win_t0) && !(t >= pre.win_t1); }

template <class P>
RPT_DEV bool mesh_walk(const KernelArgs &a, const rpt_object &obj, int i, const Ray &newRay, f3 world_origin, float world_dirlen, Hit &hit) {
#ifdef RPT_DIAGNOSTICS
    if constexpr (P::diag != 0) return diag_walk<P::diag>(a, obj, a.dobjs[i].root, newRay, world_origin, world_dirlen, hit);
#endif
    if (P::walk == Walk::reference) return octree_core_ref(a, obj, newRay, world_origin, world_dirlen, hit);
    return octree_walk<P::walk == Walk::latency, P::exact_rcp, P::park_bystanders && P::walk == Walk::throughput>(a, obj, a.dobjs[i].root, newRay, world_origin, world_dirlen, hit);
}

RPT_DEV float max3(f3 v) { return cl_max(cl_max(v.x, v.y), v.z); }   // opencl_kernel.cl:310
RPT_DEV float cube_winding(f3 origin) {
    return max3(mk3(__builtin_fabsf(origin.x), __builtin_fabsf(origin.y), __builtin_fabsf(origin.z))) < 1.0f ? -1.0f : 1.0f;
}

// opencl_kernel.cl:312-333 from the object-space ray (dir normalised, scale = its former length)
RPT_DEV bool cube_core(const rpt_object &obj, f3 origin, float winding, f3 dir, float scale, Hit &hit) {
    f3 sgn = mk3(-cl_sign(dir.x), -cl_sign(dir.y), -cl_sign(dir.z));
    const f3 d = (sgn * winding - origin) / dir;
#define RPT_TEST(U, V, W) ((d.U >= 0.0f) && (__builtin_fabsf(origin.V + dir.V * d.U) < 1.0f) && (__builtin_fabsf(origin.W + dir.W * d.U) < 1.0f))
    if (RPT_TEST(x, y, z)) sgn = mk3(sgn.x, 0, 0);
    else if (RPT_TEST(y, z, x)) sgn = mk3(0, sgn.y, 0);
    else sgn = mk3(0, 0, RPT_TEST(z, x, y) ? sgn.z : 0);
#undef RPT_TEST
    const bool any = (sgn.x != 0) || (sgn.y != 0) || (sgn.z != 0);
    if (!any) return false;          // the reference fills hit with NaNs here and discards it
    const float dist = (sgn.x != 0) ? d.x : ((sgn.y != 0) ? d.y : d.z);
    const f3 objPt = origin + dir * dist;
    hit.dist = dist / scale;
    hit.normal = normalize(applyTranspose(obj.InvM, sgn));
    if (sgn.x != 0) { hit.uv.x = (objPt.y + 1) / 2; hit.uv.y = (objPt.z + 1) / 2; }
    else if (sgn.y != 0) { hit.uv.x = (objPt.x + 1) / 2; hit.uv.y = (objPt.z + 1) / 2; }
    else { hit.uv.x = (objPt.x + 1) / 2; hit.uv.y = (objPt.y + 1) / 2; }
    return true;
}

// opencl_kernel.cl:335-359 from the object-space ray; c = dot(rayToSphere,rayToSphere) - 1.
// The (u,v) of a sphere hit is only ever consumed by the texture fetch, so it is evaluated only
// for textured spheres (want_uv); the double-precision divide by M_PI is the reference's (M_PI is a
// double constant in OpenCL C).
RPT_DEV bool sphere_core(const rpt_object &obj, f3 rayToSphere, float c, f3 dir, float scale, Hit &hit, bool want_uv) {
    const float b = dot(rayToSphere, dir);
    float disc = b * b - c;
    if (disc < 0.0f) return false;
    disc = __builtin_sqrtf(disc);
    float dist;
    if ((b - disc) > RPT_EPSILON) dist = b - disc;
    else if ((b + disc) > RPT_EPSILON) dist = b + disc;
    else return false;
    const f3 objPt = -rayToSphere + dir * dist;
    hit.dist = dist / scale;
    hit.normal = normalize(applyTranspose(obj.InvM, objPt));
    if (want_uv) {
        hit.uv.x = (float)(0.5f + rpt_atan2f(objPt.z, objPt.x) / (2 * RPT_PI_D));
        hit.uv.y = (float)(rpt_asinf(objPt.y) / RPT_PI_D + 0.5f);
    } else {
        hit.uv.x = 0.0f;
        hit.uv.y = 0.0f;
    }
    return true;
}

// ---- The shadow-segment culls.  sample_light (opencl_kernel.cl:488-545) asks of every object but the light: is it hit at a
// distance below lightDist?  For a wave whose lanes ALL satisfy the predicates below the answer is "no" without the normalisation
// (a square root, three IEEE divisions) and the intersector.  The predicates are sufficient conditions in the kernel's own float
// arithmetic; u = 2^-24, first-order bounds with the constants rounded up (numerical cross-check: tests/test_float_error_bounds.py).
//
// Sphere and cube (unit shapes in object space).  Notation: o = origin, D = dir (both floats, as computed above), scale =
// fl(|D|), g = fl(D / scale) the direction the intersector works with, `dist` its float result, hit.dist = fl(dist / scale).
//  (i) WHERE the reported hit lies.  Let P = o + g dist, exactly.  cube_core: dist = fl(fl(+-1 - o_U) / g_U) >= 0 and
//      |fl(o_V + fl(g_V dist))| < 1 give |P_U -+ 1| <= 2.1u (1 + |o_U|), |P_V| < 1 + 2.1u + 1.1u |o_V|: P in [-m1, m1]^3 with
//      m1 = 1 + 4u (1 + |o|max).  sphere_core: with b = fl(o' . g), c = fl(fl(|o|^2) - 1), disc = fl(fl(b b) - c), sq = fl(sqrt disc),
//      dist = fl(b -+ sq) one finds |P|^2 = 1 + E,  E = 2 b beta + (c - c~) + u-terms of b^2, disc, sq^2 + 2 sq (beta + rho) +
//      theta dist^2  with |beta| <= 3.1u |o| (the dot product), |c - c~| <= 4.1u |o|^2 + u, |rho| <= u |dist|, |theta| <= 8.1u
//      (|g|^2 - 1), sq <= max(|o|, 1), |dist| <= 2 max(|o|, 1):  E <= 58u (1 + |o|^2), every |P_k| <= |P| <= 1 + 29u (1 + |o|^2).
//  (ii) THAT it lies on the tested segment.  g_k = D_k / scale (1 + d1), hit.dist = dist / scale (1 + d2), |d1|, |d2| <= u:
//      P_k = o_k + D_k tau_k with tau_k = hit.dist (1 + 2.1u) in [0, lightDist (1 + 2.1u)) — inside [0, s], s = fl(lightDist * 1.001
//      + 1e-4).  So P_k lies between o_k and E_k = o_k + D_k s, and the float end point e_k = fl(o_k + fl(D_k s)) obeys
//      |e_k - E_k| <= u (|o_k| + 2.1 |e_k|).
//  (iii) Hence, if o_k > m and e_k > m (or both < -m) for one k, every point of the segment has |x_k| > m (1 - 2.1u) - 1.1u |o_k|,
//      which excludes P as soon as   m >= 1 + 29u (1 + |o|^2) + 2.1u m + 1.1u |o|max   (the cube's 4u (1 + |o|max) is smaller):
//      m = 1 + 2e-6 (1 + |o|^2)  [2e-6 = 33.6u]  does it with room for its own three float roundings.  A NaN compares false: kept.
RPT_DEV bool unit_segment_apart(f3 origin, f3 dir, float seg_max) {
    const float s = seg_max * 1.001f + 1.0e-4f, m = 1.0f + 2.0e-6f * (1.0f + dot(origin, origin));
    const f3 e = origin + dir * s;
    return ((origin.x > m) & (e.x > m)) | ((origin.x < -m) & (e.x < -m)) |
           ((origin.y > m) & (e.y > m)) | ((origin.y < -m) & (e.y < -m)) |
           ((origin.z > m) & (e.z > m)) | ((origin.z < -m) & (e.z < -m));
}
// A mesh (only one whose octree lists nothing but triangles inside the root's box: the host says which — a second mesh's lists also
// carry the first one's triangles, Mesh.cpp:16-19).  The walk accepts a triangle where Moeller-Trumbore in float says so
// (opencl_kernel.cl:106-126: |det| >= 1e-7, 0 <= u <= 1, v >= 0, u + v <= 1, 0 <= dist < best) and re-measures the winner's distance in
// the rest frame: hit.dist = |M (o + g dist) - wo| / |dw| (:301-303; wo, dw = the rest-frame event and direction).
//  (i) WHERE.  With T = A + u e1 + v e2 (a point of the triangle, up to u max(|e1|, |e2|)) and Q = o + g dist, Cramer's rule carried
//      through the float operations gives   |Q - T| <= 27.2u tau |e1| |e2| / |det| + u (tau + 2.1 dist + 2.1 max(|e1|, |e2|))
//      (tau = |o - A|; every numerator and the determinant are 3-term dots of one cross product: 6.8u of their operands' norms each),
//      and |det| >= 1e-7 makes the first term <= 16.2 tau K, K = the largest |e1| |e2| of the mesh's triangles (host, at upload).
//      tau <= t1 + h1, t1 = the L1 distance of o from the box centre, h1 = the box's half extents summed: Q lies within
//      (16.2 K + 3.2u) (t1 + h1) + 4u L  of the root box (L = longest edge).
//  (ii) ON THE SEGMENT.  As above Q_k = o_k + D_k sigma_k, sigma_k = (dist / scale)(1 + u).  dist / scale is NOT hit.dist here:
//      with R3 = M3 InvM3 - I, rt = M3 InvM.t + M.t and kM = || |M3| |InvM3| ||_F the re-measured distance obeys
//      dist / scale <= (hit.dist (1 + 7u) + (c1 |wo| + c0) / |dw|) / (1 - c1),  c1 = ||R3||_F + 16u kM,  c0 = |rt| + 16u (|| |M3| |InvM.t| || + |M.t|).
//      The host checks c1 <= 4e-4 and hands over mcw = 1.01 c1 / dmin and ms0 = 1e-4 + 1.01 c0 / dmin (dmin: a lower bound of |dw|
//      over all unit light directions): then sigma_k <= s = fl(lightDist * 1.001 + (ms0 + mcw |wo|_1)).
//  (iii) Both end points beyond the same plane of the box grown by  (16.2 K + 3.2u)(t1 + h1) + 4u L  [= mconst + mslope t1; mh
//      already holds 8u max(|lo_k|, |hi_k|)]  + 2e-6 (|o_k| + |e_k| + |c_k|)  [the float end point, the subtraction of the centre and
//      the compares] exclude Q.  The argument needs 16.2 K small to be of any use: the host enables this cull only for meshes
//      with 16.2 K + 3.2u <= 0.25 (bunny.obj: 0.0046; pear.obj, whose triangles are up to half a unit long in a model five units
//      tall: 3.1 — for such a mesh a ray within 1e-3 rad of a triangle's plane can be given ANY distance by the float test, the
//      reference's included, and no margin short of the mesh's own size excludes that; it keeps mesh_ray_misses_root only).
RPT_DEV bool mesh_segment_apart(const DObj &pre, f3 wo, f3 origin, f3 dir, float seg_max) {
    const float s = seg_max * 1.001f + (pre.ms0 + pre.mcw * (__builtin_fabsf(wo.x) + __builtin_fabsf(wo.y) + __builtin_fabsf(wo.z)));
    const f3 e = origin + dir * s;
    const float px = origin.x - pre.cbx, py = origin.y - pre.cby, pz = origin.z - pre.cbz;     // (relative to the centre: the box is |x - c| <= mh)
    const float ex = e.x - pre.cbx, ey = e.y - pre.cby, ez = e.z - pre.cbz;
    const float gd = pre.mconst + pre.mslope * (__builtin_fabsf(px) + __builtin_fabsf(py) + __builtin_fabsf(pz));
    const float gx = pre.mh[0] + gd + 2.0e-6f * (__builtin_fabsf(origin.x) + __builtin_fabsf(e.x) + __builtin_fabsf(pre.cbx));
    const float gy = pre.mh[1] + gd + 2.0e-6f * (__builtin_fabsf(origin.y) + __builtin_fabsf(e.y) + __builtin_fabsf(pre.cby));
    const float gz = pre.mh[2] + gd + 2.0e-6f * (__builtin_fabsf(origin.z) + __builtin_fabsf(e.z) + __builtin_fabsf(pre.cbz));
    return ((px > gx) & (ex > gx)) | ((px < -gx) & (ex < -gx)) |
           ((py > gy) & (ey > gy)) | ((py < -gy) & (ey < -gy)) |
           ((pz > gz) & (ez > gz)) | ((pz < -gz) & (ez < -gz));
}
// ANY mesh, any ray: the walk reports nothing unless the float slab test of the root box passes (opencl_kernel.cl:128-170, 228-230),
// and a passing test means that the exact forward ray o + t g, t > 0, meets the box grown per axis by 3.1u |b - o_k| (the six plane
// distances are t = fl(fl(b - o_k) fl(1 / g_k)) = t_exact (1 + 3.1u); the slab logic leaves a float T > 0 between all near and far
// distances; the exact point o + g T lies that close to every slab — rpt_bounds_certify.hpp, section 2).  g_k = D_k / scale (1 + u):
// as a direction, D with every component perturbed by one rounding.  So the walk can be skipped where NO ray o + t D', t > 0,
// D'_k = D_k (1 +- u), meets the box |x_k - c_k| <= H_k, H_k = half extent + 4u (max(|lo_k|, |hi_k|) + |o_k|) — decided here without
// the normalisation and the six divisions by the separating axes of a ray and a box, in float with the roundings accounted for:
//   h_k = mh_k + 6e-7 |o_k| >= H_k (1 + 4u)     (mh_k holds 8u max(|lo_k|, |hi_k|); 6e-7 = 10u)
//   p_k = fl(c_k - o_k) = (c_k - o_k)(1 + u)
//   box axes:   p_k < -h_k and D_k >= 0, or p_k > h_k and D_k <= 0   (the origin beyond a side, moving away or along it)
//   cross axes: the LINE misses if |p_j D'_k - p_k D'_j| > H_j |D'_k| + H_k |D'_j|.  A = fl(fl(p_j D_k) - fl(p_k D_j)) is within
//               3.2u W + u |A| of the left side, W = |p_j D_k| + |p_k D_j|; S = fl(fl(h_j |D_k|) + fl(h_k |D_j|)) (1 + u) bounds
//               the right side: asked is  |A| > S * 1.000001 + 5e-7 W   (5e-7 = 8.4u > 3.2u + u + what S and W themselves round by).
// A NaN or an infinity compares false: the walk runs.
RPT_DEV bool mesh_ray_misses_root(const DObj &pre, f3 origin, f3 dir) {
    const float px = pre.cbx - origin.x, py = pre.cby - origin.y, pz = pre.cbz - origin.z;
    const float hx = pre.mh[0] + 6.0e-7f * __builtin_fabsf(origin.x), hy = pre.mh[1] + 6.0e-7f * __builtin_fabsf(origin.y), hz = pre.mh[2] + 6.0e-7f * __builtin_fabsf(origin.z);
    bool miss = ((px < -hx) & (dir.x >= 0.0f)) | ((px > hx) & (dir.x <= 0.0f)) |
                ((py < -hy) & (dir.y >= 0.0f)) | ((py > hy) & (dir.y <= 0.0f)) |
                ((pz < -hz) & (dir.z >= 0.0f)) | ((pz > hz) & (dir.z <= 0.0f));
    const float ax = __builtin_fabsf(dir.x), ay = __builtin_fabsf(dir.y), az = __builtin_fabsf(dir.z);
    {   // axis x cross D: components (y, z)
        const float m1 = py * dir.z, m2 = pz * dir.y;
        miss = miss | (__builtin_fabsf(m1 - m2) > (hy * az + hz * ay) * 1.000001f + 5.0e-7f * (__builtin_fabsf(m1) + __builtin_fabsf(m2)));
    }
    {   // axis y: (z, x)
        const float m1 = pz * dir.x, m2 = px * dir.z;
        miss = miss | (__builtin_fabsf(m1 - m2) > (hz * ax + hx * az) * 1.000001f + 5.0e-7f * (__builtin_fabsf(m1) + __builtin_fabsf(m2)));
    }
    {   // axis z: (x, y)
        const float m1 = px * dir.y, m2 = py * dir.x;
        miss = miss | (__builtin_fabsf(m1 - m2) > (hx * ay + hy * ax) * 1.000001f + 5.0e-7f * (__builtin_fabsf(m1) + __builtin_fabsf(m2)));
    }
    return miss;
}

// One object against one ray given as a 4-D event + 4-D direction in the object's rest frame
// (the general form: shadow rays, and primary rays of the RefLayout kernel).
// seg_max > 0 (shadow rays): the caller only asks whether the object is hit at a distance below seg_max (sample_light:
// dist < lightDist); if no lane of the wave can get "yes" (unit_segment_apart / mesh_segment_apart above, __ballot), the
// normalisation, its three IEEE divisions and the intersector are skipped for the whole wave.
// (Measured also: the slab test with v_rcp_f32 as a second stage, and the same for mesh roots as a ray test: no
// further gain on any scene — three quarter-rate reciprocals cost what they save)
template <class P>
RPT_DEV bool intersect_object(const KernelArgs &a, int i, f4 origin4, f4 dir4, Hit &hit, float seg_max = -1.0f) {
    const rpt_object &obj = a.objects[i];
    const f3 origin = transformPoint(obj.InvM, yzw(origin4));
    f3 dir = transformDirection(obj.InvM, yzw(dir4));
    if (P::culled && seg_max > 0.0f && obj.type != RPT_MESH) {
        if (__ballot(!unit_segment_apart(origin, dir, seg_max)) == 0ull) return false;
    }
    if (P::culled && seg_max > 0.0f && obj.type == RPT_MESH && a.dobjs[i].mh[0] >= 0.0f) {
        const DObj &pre = a.dobjs[i];
        bool idle = mesh_ray_misses_root(pre, origin, dir);
        if (pre.mslope >= 0.0f) idle = idle | mesh_segment_apart(pre, yzw(origin4), origin, dir, seg_max);      // (wave-uniform branch)
        if (__ballot(!idle) == 0ull) return false;
    }
    const float scale = length(dir);
    dir = dir / scale;
    switch (obj.type) {
    case RPT_SPHERE: {
        const f3 rayToSphere = -origin;
        return sphere_core(obj, rayToSphere, dot(rayToSphere, rayToSphere) - 1.0f, dir, scale, hit, obj.textureIndex != -1);
    }
    case RPT_CUBE:
        return cube_core(obj, origin, cube_winding(origin), dir, scale, hit);
    case RPT_MESH: {
        if (P::walk == Walk::none) return false;      // the analytic-only kernel is launched for scenes without mesh objects only
        Ray newRay;
        newRay.origin = origin;
        newRay.dir = dir;
        return mesh_walk<P>(a, obj, i, newRay, yzw(origin4), length(yzw(dir4)), hit);
    }
    default:
        return false;
    }
}

// Primary rays of the kernels on the derived layouts: the object-space origin and what depends on it alone come
// from the per-frame DObj record; only rows 1..3 of Lorentz * (interval, d) are formed (row 0, the
// time component, is needed for the flash test of the final hit only).
template <class P>
RPT_DEV bool intersect_object_primary(const KernelArgs &a, int i, f4 rayDir, Hit &hit) {
    const rpt_object &obj = a.objects[i];
    const DObj &pre = a.dobjs[i];
    const f3 d3 = mk3(dot(ld4(obj.Lorentz[1]), rayDir), dot(ld4(obj.Lorentz[2]), rayDir), dot(ld4(obj.Lorentz[3]), rayDir));
    f3 dir = transformDirection(obj.InvM, d3);
    const float scale = length(dir);
    dir = dir / scale;
    const f3 origin = mk3(pre.ox, pre.oy, pre.oz);
    switch (obj.type) {
    case RPT_SPHERE:
        return sphere_core(obj, -origin, pre.sphere_c, dir, scale, hit, obj.textureIndex != -1);
    case RPT_CUBE:
        return cube_core(obj, origin, pre.winding, dir, scale, hit);
    case RPT_MESH: {
        if (P::walk == Walk::none) return false;
        Ray newRay;
        newRay.origin = origin;
        newRay.dir = dir;
        const f3 cam3 = mk3(obj.stationaryCam.y, obj.stationaryCam.z, obj.stationaryCam.w);
        return mesh_walk<P>(a, obj, i, newRay, cam3, length(d3), hit);
    }
    default:
        return false;
    }
}

RPT_DEV float texel(const KernelArgs &a, long long addr) {
    addr = addr < 0 ? 0 : addr;
    addr = addr >= a.texture_bytes ? a.texture_bytes - 1 : addr;
    return a.textures[addr] / 255.0f;
}
RPT_DEV f3 texel3(const KernelArgs &a, int offset, int width, int x, int y) {
    const long long base = (long long)offset + 3 * ((long long)width * y + x);
    return mk3(texel(a, base + 0), texel(a, base + 1), texel(a, base + 2));
}

// bilinear RGB8 fetch of opencl_kernel.cl:427-471 (upper clamps only; the odd 4th tap is the reference's)
RPT_DEV f3 sample_texture(const KernelArgs &a, const rpt_object &ho, f2 huv) {
    const int width = ho.textureWidth;
    const int height = ho.textureHeight;
    const float u = width * huv.x;
    const float v = height * (1.0f - huv.y);
    int x = imin(f2i_sat(__builtin_floorf(u)), width - 1);
    int y = imin(f2i_sat(__builtin_floorf(v)), height - 1);
    const float u_ratio = u - x;
    const float v_ratio = v - y;
    const float u_opp = 1 - u_ratio;
    const float v_opp = 1 - v_ratio;
    const int offset = ho.textureIndex;
    f3 result = texel3(a, offset, width, x, y) * u_opp;
    x = iclamp(x + 1, 0, width - 1);
    result = result + texel3(a, offset, width, x, y) * u_ratio;
    result = result * v_opp;
    y = iclamp(y + 1, 0, height - 1);
    f3 result2 = texel3(a, offset, width, x, y) * u_ratio;
    x = iclamp(x - 1, 0, width - 1);
    result2 = result2 + texel3(a, offset, width, x, y) * u_opp;
    result2 = result2 * v_ratio;
    return result + result2;
}

// ---- parking (KernelPolicy::park_bystanders) ---------------------------------------------------------------------
// A shadow walk reads the shadow ray and the octree; the shading state around it — the hit, its colour, the sum so far, the camera
// ray — only waits, and at six waves per SIMD (80 registers) it would wait in scratch.  It waits here instead: slot k of lane l is
// park_lds[k][l], so a wave's 64 lanes touch 64 consecutive words (ds_write_b32 / ds_read_b32 without a bank conflict).  A product
// workgroup is ONE wave and a lane reads only what it wrote itself: no barrier.  volatile: the values must not be forwarded from store
// to load in registers, which is the very thing this is for.  Lanes outside the frame have returned before anything is parked.
// How many: with these 17 the compiler spills nothing; any ONE group below (object, direction, normal + distance, surface colour) may
// stay in registers and it still spills nothing, any two and it spills a dword — they all wait here, for a margin of one group.  The
// shadow ray itself (sample_light_occluded's origin, direction and length, live across its occluders) needs no slot.
// LDS: RPT_PARK_SLOTS x 256 B = 4352 B per workgroup; six waves on each of a CU's four SIMDs are 24 workgroups, 104 448 B of the CU's
// 163 840 B (160 KB): the registers stay the limit, not the LDS (the occupancy remark reads 6).
#define RPT_PARK_SLOTS 17
enum ParkSlot {
    PARK_HCOLOR = 0,         // 3: the hit's surface colour                                           (trace: across the light loop)
    PARK_COLOR = 3,          // 3: the sum so far
    PARK_NORMAL = 6,         // 3: hit.normal
    PARK_DIST = 9,           // 1: hit.dist
    PARK_ND = 10,            // 3: the camera ray's unit direction
    PARK_OBJECT = 13,        // 1: hit.object (its bits)
    PARK_L3 = 14,            // 3: lightDir3_ObjFrame of the light being sampled                       (trace: across one shadow ray)
};
// (the accesses name the LDS address space themselves: a volatile access through a generic pointer stays a flat instruction with a
// 64-bit address per slot)
// ONE-WAVE WORKGROUPS ONLY: a slot is indexed by the lane, threadIdx.x & 63, so in a workgroup of several waves the waves would share
// each other's slots, with no barrier between them.  Every function that parks static_asserts P::one_wave; call these from nowhere else.
__shared__ float park_lds[RPT_PARK_SLOTS][64];
typedef volatile __attribute__((address_space(3))) float park_word;
RPT_DEV void park_put(int k, float v) { *(park_word *)&park_lds[k][threadIdx.x & 63] = v; }
RPT_DEV float park_get(int k) { return *(park_word *)&park_lds[k][threadIdx.x & 63]; }
RPT_DEV void park_put3(int k, f3 v) { park_put(k, v.x); park_put(k + 1, v.y); park_put(k + 2, v.z); }
RPT_DEV f3 park_get3(int k) { const float x = park_get(k), y = park_get(k + 1), z = park_get(k + 2); return mk3(x, y, z); }

// opencl_kernel.cl:488-545: true when something other than the light blocks the segment
template <class P>
RPT_DEV bool sample_light_occluded(const KernelArgs &a, f4 origin4, f4 dir4, float lightDist, int lightIndex) {
    const f3 nd = normalize(yzw(dir4));
    const f4 lightDir0 = mk4((float)a.interval, nd.x, nd.y, nd.z);
    for (int i = 0; i < a.object_count; i++) {
        if (i != lightIndex) {
            Hit newHit;
            newHit.dist = 1e20f;
            const f4 newEvent0 = transformPoint4D(a.objects[i].Lorentz, origin4);
            const f4 lightDir = transformPoint4D(a.objects[i].Lorentz, lightDir0);
            if (intersect_object<P>(a, i, newEvent0, lightDir, newHit, lightDist)) {
                if constexpr (P::windowed) {     // the occluder's event in its own rest frame: the two products above, nothing new
                    if (newHit.dist < lightDist && window_accepts(a.dobjs[i], newEvent0.x + lightDir.x * newHit.dist)) return true;
                } else {
                    if (newHit.dist < lightDist) return true;
                }
            }
        }
    }
    return false;
}

// ---- Doppler shift and searchlight beaming (not in the reference; DESIGN.md "Doppler and beaming") ------------------------
// D = observed / emitted frequency.  Each RGB channel is a spectral sample at a fixed frequency relative to green (the CIE 1931
// RGB primaries 700.0 / 546.1 / 435.8 nm); the knots are computed in double and rounded to float once (here, at compile time).
// The emitted spectrum of a colour (r, g, b) is piecewise linear through (K0, 0), (NU_R, r), (1, g), (NU_B, b), (K4, 0) and 0
// outside; channel k observes it at NU_k / D.  Only + - * / and compares: tests/test_doppler_model.py restates it in numpy
// float32 and the probe (rpt_probe which = 6) must match that restatement bit for bit.
#define RPT_DOPPLER_RECORD 11
#define RPT_NU_R ((float)(546.1 / 700.0))
#define RPT_NU_B ((float)(546.1 / 435.8))
#define RPT_NU_K0 ((float)(2.0 * (546.1 / 700.0) - 1.0))
#define RPT_NU_K4 ((float)(2.0 * (546.1 / 435.8) - 1.0))

RPT_DEV float doppler_spectrum(float u, float r, float g, float b) {
    if (!(u > RPT_NU_K0) || !(u < RPT_NU_K4)) return 0.0f;      // beyond the outer knots (and NaN): infrared / ultraviolet
    float xa, xb, ya, yb;
    if (u < RPT_NU_R) { xa = RPT_NU_K0; xb = RPT_NU_R; ya = 0.0f; yb = r; }
    else if (u < 1.0f) { xa = RPT_NU_R; xb = 1.0f; ya = r; yb = g; }
    else if (u < RPT_NU_B) { xa = 1.0f; xb = RPT_NU_B; ya = g; yb = b; }
    else { xa = RPT_NU_B; xb = RPT_NU_K4; ya = b; yb = 0.0f; }
    const float t = (u - xa) / (xb - xa);
    return ya * (1.0f - t) + yb * t;                          // exact at both ends of the segment: continuous across every knot
}

// S_f(D, c): flags bit 0 = shift (the spectrum above), bit 1 = beaming (x D^3 with the shift: I_nu / nu^3 is invariant;
// x D^4 without it: the bolometric form, hue unchanged).  D == 1 returns c bit for bit by an explicit test.
RPT_DEV f3 doppler_colour(int flags, float D, f3 c) {
    if (D == 1.0f) return c;
    f3 o = c;
    if (flags & 1) {
        o.x = doppler_spectrum(RPT_NU_R / D, c.x, c.y, c.z);
        o.y = doppler_spectrum(1.0f / D, c.x, c.y, c.z);
        o.z = doppler_spectrum(RPT_NU_B / D, c.x, c.y, c.z);
        if (flags & 2) {
            const float d3 = (D * D) * D;
            o = o * d3;
        }
    } else if (flags & 2) {
        const float d2 = D * D;
        o = c * (d2 * d2);
    }
    return o;
}

// ---- The sky (rpt_set_environment; not in the reference; DESIGN.md "Environment map") -------------------------------------------------
// (u, v) of a unit direction d in the sky's rest frame: sphere_core's own two lines (the textured sphere's), with d.y clamped into
// asin's domain first (a normalised d can exceed 1 by an ulp; a NaN passes through and ends on texel (0, 0) below).
RPT_DEV f2 environment_uv(f3 d) {
    const float dy = d.y < -1.0f ? -1.0f : (d.y > 1.0f ? 1.0f : d.y);
    f2 uv;
    uv.x = (float)(0.5f + rpt_atan2f(d.z, d.x) / (2 * RPT_PI_D));
    uv.y = (float)(rpt_asinf(dy) / RPT_PI_D + 0.5f);
    return uv;
}
RPT_DEV f3 environment_texel(const uint32_t *texels, int width, int x, int y) {
    const uint32_t t = texels[(size_t)y * width + x];
    return mk3((t & 255u) / 255.0f, ((t >> 8) & 255u) / 255.0f, ((t >> 16) & 255u) / 255.0f);
}
// sample_texture's four taps in its order, on the sky image: the column neighbour WRAPS (x + 1 == W -> 0, x - 1 == -1 -> W - 1; u = 0 and
// u = 1 are the same meridian), rows clamp as there.  x and y are clamped into the image on BOTH sides before they address anything
// (f2i_sat: NaN -> 0), so no direction, finite or not, reads outside the width * height dwords.
RPT_DEV f3 environment_bilinear(const uint32_t *texels, int width, int height, f2 uv) {
    const float u = width * uv.x;
    const float v = height * (1.0f - uv.y);
    int x = iclamp(f2i_sat(__builtin_floorf(u)), 0, width - 1);
    int y = iclamp(f2i_sat(__builtin_floorf(v)), 0, height - 1);
    const float u_ratio = u - x;
    const float v_ratio = v - y;
    const float u_opp = 1 - u_ratio;
    const float v_opp = 1 - v_ratio;
    f3 result = environment_texel(texels, width, x, y) * u_opp;
    x = x + 1 >= width ? 0 : x + 1;
    result = result + environment_texel(texels, width, x, y) * u_ratio;
    result = result * v_opp;
    y = iclamp(y + 1, 0, height - 1);
    f3 result2 = environment_texel(texels, width, x, y) * u_ratio;
    x = x - 1 < 0 ? width - 1 : x - 1;
    result2 = result2 + environment_texel(texels, width, x, y) * u_opp;
    result2 = result2 * v_ratio;
    return result + result2;
}
// A primary ray that hit nothing: its look-back path (interval, n) goes through E into the sky's rest frame, the spatial part is the
// direction the image is looked up at, and with Doppler on the time parts give D_env = interval / k.x exactly as D_cam comes from an
// object's Lorentz[0] (interval 0: D_env := 1, nothing to shift).  No ambient factor, no lights, no flash.
RPT_DEV f3 environment_colour(const EnvironmentArgs &a, f3 camdir) {
    const f3 nd = normalize(camdir);             // (trace()'s own first line: the same float triple)
    const f4 rayDir = mk4((float)a.interval, nd.x, nd.y, nd.z);
    const f4 k = transformPoint4D(a.env_frame, rayDir);
    const f3 d = normalize(yzw(k));
    f3 c = environment_bilinear(a.env_texels, a.env_width, a.env_height, environment_uv(d));
    if (a.doppler != 0 && a.interval != 0) c = doppler_colour(a.doppler, (float)a.interval / k.x, c);
    return c;
}

// What the Doppler debug kernel records per hit pixel (rpt_set_debug_doppler)
struct DopplerRecord {
    float dcam, dlight;      // camera factor; light factor of the first light that contributed (1 if none)
    f3 ref, lit;             // the reference's colour (no Doppler); the colour after the light factors, before S(D_cam)
};

// trace()'s light loop for KernelPolicy::park_bystanders: the same operations on the same inputs in the same order, with every value
// that outlives a shadow ray kept in LDS.  What is a pure function of parked values — ndotl, the unit light direction, the falloff's
// length and self-dot — is formed again after the shadow ray from the parked lightDir3_ObjFrame and normal: the same bits.
template <class P>
RPT_DEV f3 trace_lights_parked(const KernelArgs &a, f3 nd, const Hit &hit, f3 hcolor, f3 color) {
    static_assert(!P::doppler && !P::windowed && !P::drec && P::one_wave, "parking: kernel 41's policy only");
    park_put3(PARK_HCOLOR, hcolor);
    park_put3(PARK_COLOR, color);
    park_put3(PARK_NORMAL, hit.normal);
    park_put(PARK_DIST, hit.dist);
    park_put3(PARK_ND, nd);
    park_put(PARK_OBJECT, __int_as_float(hit.object));
    for (int i = 0; i < a.object_count; i++) {
        const int object = __float_as_int(park_get(PARK_OBJECT));
        if (i != object && a.objects[i].light) {
            const rpt_object &ho = a.objects[object];
            const rpt_object &lo = a.objects[i];
            const f3 normal = park_get3(PARK_NORMAL), d3 = park_get3(PARK_ND);
            const f4 rayDir = mk4((float)a.interval, d3.x, d3.y, d3.z);
            const f4 cameraPos_ObjFrame = ld4(ho.stationaryCam);
            const f4 rayDir_ObjFrame = transformPoint4D(ho.Lorentz, rayDir);
            f4 hitPos_ObjFrame = cameraPos_ObjFrame + rayDir_ObjFrame * park_get(PARK_DIST);
            hitPos_ObjFrame = hitPos_ObjFrame + mk4(0, normal.x * 0.001f, normal.y * 0.001f, normal.z * 0.001f);
            const f4 hitPos = transformPoint4D(ho.InvLorentz, hitPos_ObjFrame);
            const f4 hitPos_LightFrame = transformPoint4D(lo.Lorentz, hitPos);
            const f3 lightPos3_LightFrame = mk3(lo.M[0].w, lo.M[1].w, lo.M[2].w);
            const f3 lightDir3_LightFrame = lightPos3_LightFrame - yzw(hitPos_LightFrame);
            const f4 lightDir_LightFrame = mk4(a.interval * length(lightDir3_LightFrame), lightDir3_LightFrame.x,
                                               lightDir3_LightFrame.y, lightDir3_LightFrame.z);
            const f4 lightDir = transformPoint4D(lo.InvLorentz, lightDir_LightFrame);
            const f4 lightDir_ObjFrame = transformPoint4D(ho.Lorentz, lightDir);
            const f3 lightDir3_ObjFrame = yzw(lightDir_ObjFrame);
            if (dot(normal, normalize(lightDir3_ObjFrame)) > 0) {
                park_put3(PARK_L3, lightDir3_ObjFrame);
                const f3 ld = normalize(yzw(lightDir));
                const f4 shadowDir = mk4((float)a.interval, ld.x, ld.y, ld.z);
                if (!sample_light_occluded<P>(a, hitPos, shadowDir, length(yzw(lightDir)), i)) {
                    const f3 l3 = park_get3(PARK_L3);
                    const float ndotl = dot(park_get3(PARK_NORMAL), normalize(l3));
                    const float k = ndotl / (1.0f + 0.1f * length(l3) + 0.01f * dot(l3, l3));
                    const f3 sum = park_get3(PARK_COLOR) + park_get3(PARK_HCOLOR) * k * ld3(lo.color);
                    park_put3(PARK_COLOR, sum);
                }
            }
        }
    }
    return park_get3(PARK_COLOR);
}

// opencl_kernel.cl:361-486 + 548-604: closest hit over the object list, surface colour, lights
// Returns false (and leaves `color` untouched) when the ray hits nothing: the caller then uses the
// per-frame background constants instead of tonemapping (0.15,0.15,0.25) again for every pixel.
// P::doppler (the twins of rpt_set_doppler): each light's colour goes through S_f(D_i) and the summed colour through S_f(D_cam);
// P::drec (the Doppler debug kernel only) also fills *rec.  With light propagation off (interval 0) nothing changes.
template <class P>
RPT_DEV bool trace(const KernelArgs &a, f3 camdir, unsigned long long object_mask, f3 &color_out, DopplerRecord *rec = nullptr) {
    const float inf = 1e20f;
    Hit hit;
    hit.dist = inf;
    hit.object = -1;
    const f3 nd = normalize(camdir);
    const f4 rayDir = mk4((float)a.interval, nd.x, nd.y, nd.z);

    for (int i = 0; i < a.object_count; i++) {
        // wave-uniform skip of objects whose bounding volume no ray of this tile can reach (a miss for every
        // lane in the reference too, so skipping it changes nothing)
        if (i < 64 && !((object_mask >> i) & 1ull)) continue;
        Hit newHit;
        newHit.dist = inf;
        bool got;
        if (P::walk == Walk::reference) got = intersect_object<P>(a, i, ld4(a.objects[i].stationaryCam), transformPoint4D(a.objects[i].Lorentz, rayDir), newHit);
        else got = intersect_object_primary<P>(a, i, rayDir, newHit);
        if (got) {
            if constexpr (P::windowed) {         // the flash term's expression below, on the candidate: the emission time in object i's rest frame
                if (newHit.dist < hit.dist && window_accepts(a.dobjs[i], a.objects[i].stationaryCam.x + dot(ld4(a.objects[i].Lorentz[0]), rayDir) * newHit.dist)) {
                    hit = newHit;
                    hit.object = i;
                }
            } else if (newHit.dist < hit.dist) {
                hit = newHit;
                hit.object = i;
            }
        }
    }
    if (hit.object < 0) return false;
#ifdef RPT_DIAGNOSTICS
    if (P::diag == 5) {   // stop after the closest hit (timing of the primary walk alone)
        color_out = mk3(hit.dist, hit.normal.x + hit.uv.x, hit.normal.y + hit.normal.z + hit.uv.y);
        return true;
    }
#endif

    const rpt_object &ho = a.objects[hit.object];
    f3 hcolor = ho.textureIndex != -1 ? sample_texture(a, ho, hit.uv) : ld3(ho.color);
    if (ho.flashPeriod > 0) {   // proper-time flash, opencl_kernel.cl:476-482: event.x of the winning hit
        const float event_x = ho.stationaryCam.x + dot(ld4(ho.Lorentz[0]), rayDir) * hit.dist;
        const float period = ho.flashPeriod;
        const float duration = ho.flashDuration;
        if (event_x - period * __builtin_floorf(event_x / period) < duration) hcolor = hcolor * 2;
    }

    f3 color = hcolor * (a.interval != 0 ? a.ambient : 1.0f);
    if (ho.light) color = color + hcolor;
    [[maybe_unused]] f3 color_ref = color;       // (P::drec only) the same sum with the reference's light colours
    [[maybe_unused]] float dlight = 1.0f;
    [[maybe_unused]] bool lit_any = false;
    if constexpr (P::park_bystanders) {
        if (a.interval != 0) color = trace_lights_parked<P>(a, nd, hit, hcolor, color);
    } else if (a.interval != 0) {
        for (int i = 0; i < a.object_count; i++) {
            if (i != hit.object && a.objects[i].light) {
                const rpt_object &lo = a.objects[i];
                const f4 cameraPos_ObjFrame = ld4(ho.stationaryCam);
                const f4 rayDir_ObjFrame = transformPoint4D(ho.Lorentz, rayDir);
                f4 hitPos_ObjFrame = cameraPos_ObjFrame + rayDir_ObjFrame * hit.dist;
                hitPos_ObjFrame = hitPos_ObjFrame + mk4(0, hit.normal.x * 0.001f, hit.normal.y * 0.001f, hit.normal.z * 0.001f);
                const f4 hitPos = transformPoint4D(ho.InvLorentz, hitPos_ObjFrame);
                const f4 hitPos_LightFrame = transformPoint4D(lo.Lorentz, hitPos);
                const f3 lightPos3_LightFrame = mk3(lo.M[0].w, lo.M[1].w, lo.M[2].w);
                const f3 lightDir3_LightFrame = lightPos3_LightFrame - yzw(hitPos_LightFrame);
                const f4 lightDir_LightFrame = mk4(a.interval * length(lightDir3_LightFrame), lightDir3_LightFrame.x,
                                                   lightDir3_LightFrame.y, lightDir3_LightFrame.z);
                if constexpr (P::windowed) {     // the emission event in the light's rest frame: a light outside its window is dark, and shoots no shadow ray
                    if (!window_accepts(a.dobjs[i], hitPos_LightFrame.x + lightDir_LightFrame.x)) continue;
                }
                const f4 lightDir = transformPoint4D(lo.InvLorentz, lightDir_LightFrame);
                const f4 lightDir_ObjFrame = transformPoint4D(ho.Lorentz, lightDir);
                const f3 lightDir3_ObjFrame = yzw(lightDir_ObjFrame);
                const f3 unitLightDir3 = normalize(lightDir3_ObjFrame);
                const float ndotl = dot(hit.normal, unitLightDir3);
                if (ndotl > 0) {
                    const f3 ld = normalize(yzw(lightDir));
                    const f4 shadowDir = mk4((float)a.interval, ld.x, ld.y, ld.z);
                    if (!sample_light_occluded<P>(a, hitPos, shadowDir, length(yzw(lightDir)), i)) {
                        const float k = ndotl / (1.0f + 0.1f * length(lightDir3_ObjFrame) +
                                                 0.01f * dot(lightDir3_ObjFrame, lightDir3_ObjFrame));
                        if constexpr (P::doppler) {
                            // light factor: time components of the light-to-surface vector in the surface's and the light's frame
                            const float di = lightDir_ObjFrame.x / lightDir_LightFrame.x;
                            if constexpr (P::drec) {
                                color_ref = color_ref + hcolor * k * ld3(lo.color);
                                if (!lit_any) dlight = di;
                                lit_any = true;
                            }
                            color = color + hcolor * k * doppler_colour(static_cast<const DopplerArgs &>(a).doppler, di, ld3(lo.color));
                        } else {
                            color = color + hcolor * k * ld3(lo.color);
                        }
                    }
                }
            }
        }
    }
    if constexpr (P::doppler) {
        float dcam = 1.0f;
        const f3 lit = color;
        if (a.interval != 0) {
            // camera factor: interval / (time component of the camera ray in the hit object's frame), the flash's float
            dcam = (float)a.interval / dot(ld4(ho.Lorentz[0]), rayDir);
            color = doppler_colour(static_cast<const DopplerArgs &>(a).doppler, dcam, color);
        }
        if constexpr (P::drec) {
            rec->dcam = dcam;
            rec->dlight = dlight;
            rec->ref = color_ref;
            rec->lit = lit;
        }
    }
    color_out = color;
    return true;
}

// opencl_kernel.cl:607-616
RPT_DEV float hable1(float x) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F;
}

RPT_DEV uint32_t to_u8(float c) {   // (unsigned char)(c * 255): saturating, NaN -> 0
    const float t = c * 255;
    if (!(t == t)) return 0u;
    if (t <= 0.0f) return 0u;
    if (t >= 255.0f) return 255u;
    return (uint32_t)(int)t;
}

// tonemap + pack of opencl_kernel.cl:649-657; returns the little-endian R,G,B,1 word
RPT_DEV uint32_t tonemap_pack(const KernelArgs &a, f3 color, f3 &mapped) {
    mapped.x = cl_min(hable1(color.x) / a.hable_wp[0], 1.0f);
    mapped.y = cl_min(hable1(color.y) / a.hable_wp[1], 1.0f);
    mapped.z = cl_min(hable1(color.z) / a.hable_wp[2], 1.0f);
    return to_u8(mapped.x) | (to_u8(mapped.y) << 8) | (to_u8(mapped.z) << 16) | (1u << 24);
}

// The wavefront's object mask, computed by the wavefront itself: lane i compares the image-plane rectangle of object i
// (rpt_screen_bounds.hpp: outside it no primary ray reaches the object; where it pays, an octagon: the rectangle with
// corners cut by two diagonal slabs) with the wave's 8x8-pixel tile, grown by a pixel
// and a half on every side, and one __ballot makes the 64 answers the mask — in SGPRs, wave-uniform, with no prepass
// kernel, no mask buffer and no dependent load behind it.  Pixel (x, y) looks through the plane point
// ((x/W - 0.5) * aspect, y/H - 0.5) (opencl_kernel.cl:57-63).  NaNs compare false, so a broken rectangle keeps its object.
// One 16-byte framebuffer pixel, written with a NON-TEMPORAL store (global_store_dwordx4 ... nt): the framebuffer is written once
// and never read by these kernels, and a 4K frame is 133 MB against 4 MB of L2 per XCD — written with the default policy the
// stream of pixels competes with the octree and the triangle records the walks live on.  Measured A/B/A/B
// (profiles/r02_nontemporal_store_ab.txt): bunny 4K 0.109 -> 0.098 ms per frame in flight, 0.218 -> 0.208 one at a time.
RPT_DEV void store_pixel(void *out16, size_t id, uint32_t x, uint32_t y, uint32_t z, uint32_t w) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    v4u pv;
    pv.x = x; pv.y = y; pv.z = z; pv.w = w;
    __builtin_nontemporal_store(pv, reinterpret_cast<v4u *>(out16) + id);
}

RPT_DEV unsigned long long wave_object_mask(const KernelArgs &a, int tile_x0, int tile_y0) {
    const int lane = threadIdx.x & 63;
    // one 16-B load per lane, issued unconditionally (lanes beyond the object count re-read rectangle 0), and four compares
    // without branches: one memory round trip, no divergence.  No early return for a scene without objects either: the buffer
    // behind `rects` always holds at least one record's worth of bytes (rpt_api.hip: reserve), and a branch here would put the
    // loads of `rects` and of the reciprocals behind it — one more dependent round trip in every wave.
    const int n = a.object_count;
    const int slot = (lane < n) ? lane : 0;
    const float4 r = a.rects[2 * slot];
    const float iw = a.inv_width, ih = a.inv_height;
    const float tu0 = (((float)tile_x0 - 1.5f) * iw - 0.5f) * a.aspect, tu1 = (((float)tile_x0 + 8.5f) * iw - 0.5f) * a.aspect;
    const float tv0 = ((float)tile_y0 - 1.5f) * ih - 0.5f, tv1 = ((float)tile_y0 + 8.5f) * ih - 0.5f;
    bool outside = (r.z < tu0) | (r.x > tu1) | (r.w < tv0) | (r.y > tv1);
    if (a.diagonals) {      // wave-uniform: the octagon's four diagonal sides (u + v and u - v over the tile's corners)
        const float4 g = a.rects[2 * slot + 1];
        outside = outside | (g.y < tu0 + tv0) | (g.x > tu1 + tv1) | (g.w < tu0 - tv1) | (g.z > tu1 - tv0);
    }
    const bool keep = (lane < n) & !outside;
    return __ballot(keep);
}

// The tile bitmaps (rpt_tile_bitmap.hpp, where the proof is): a mesh the mask keeps for this tile is dropped where its bitmap says
// that no primary ray of the tile can report a hit of it — the tiles between the mesh's silhouette and the octagon around its root box,
// whose lanes would all walk the octree through empty leaves and miss.  Called only by a wave whose mask is not empty, with lanes
// inside the frame (so the tile exists in the bitmap); everything here is wave-uniform: scalar loads of one dword per kept object.
RPT_DEV unsigned long long clear_empty_tiles(const KernelArgs &a, unsigned long long object_mask, int tile_x0, int tile_y0) {
    unsigned long long cand = object_mask & a.tile_bits_objects;
    if (cand == 0) return object_mask;
    const unsigned int tiles_x = (unsigned int)(a.width + 7) >> 3, tiles_y = (unsigned int)(a.height + 7) >> 3;
    const unsigned int t = (unsigned int)(tile_y0 >> 3) * tiles_x + (unsigned int)(tile_x0 >> 3);
    const unsigned int words = (tiles_x * tiles_y + 31u) >> 5;
    while (cand) {
        const int i = __builtin_ctzll(cand);
        cand &= cand - 1;
        const uint32_t w = a.tile_bits[(size_t)i * words + (t >> 5)];
        if (!((w >> (t & 31u)) & 1u)) object_mask &= ~(1ull << i);
    }
    return object_mask;
}

// ... for the kernels whose policy says so (KernelPolicy::tile_bits), and only in a wave whose mask is not empty: every other wave
// executes nothing new.  render_pixel_body and the probe of rpt_probe_tile_masks go through this one function.
template <class P>
RPT_DEV unsigned long long thin_object_mask(const KernelArgs &a, unsigned long long object_mask, int tile_x0, int tile_y0) {
    if constexpr (P::culled && P::object_mask && P::tile_bits && P::camera != Camera::equirect && P::diag == 0) {
        if (object_mask != 0) object_mask = clear_empty_tiles(a, object_mask, tile_x0, tile_y0);
    }
    return object_mask;
}

// The same under a lens (Camera::lens): pixel (x, y) looks through the plane point (fl(s fx2), fl(s fy2)), so the tile's four plane
// coordinates are scaled by s as well.  What the mask needs is that every pixel's plane point lies inside its tile's grown range; the
// regions themselves are statements about real plane points of the proven window, whatever rounding produced them
// (rpt_bounds_certify.hpp, section 1), and the host launches this kernel only while s <= 1 keeps every pixel inside that window.
// The skirt under s: a pixel x >= x0 of the tile has the exact coordinate U = s (x / W - 1/2) aspect, the tile's lower edge the exact
// E = s ((x0 - 1.5) / W - 1/2) aspect, U - E >= 1.5 s aspect / W.  The pixel's float chain (divide, subtract, multiply by aspect) is
// off by at most 3u aspect before the lens and the edge's (multiply by 1 / W rounded, subtract, multiply) by at most 4u aspect, u =
// 2^-24 — the existing skirt's case; the product with s scales both errors by s and adds one relative rounding of a value of at most
// s aspect / 2 to each: |fl - exact| <= 3.5u s aspect and 4.5u s aspect.  The pixel stays inside while 8u s aspect < 1.5 s aspect / W,
// i.e. W < 1.5 / 8u = 3.1 million: s cancels, so the bound of 2^20 pixels a side that launch() enforces covers every lens (no
// product underflows: s >= 0.005 and the coordinates are multiples of 2^-24 or 0).  The same in v with aspect = 1, and at the upper
// edges.  At s = 1.0f every product here is exact and the mask is wave_object_mask's.
RPT_DEV unsigned long long wave_object_mask_lens(const KernelArgs &a, float s, int tile_x0, int tile_y0) {
    const int lane = threadIdx.x & 63;
    const int n = a.object_count;
    const int slot = (lane < n) ? lane : 0;
    const float4 r = a.rects[2 * slot];
    const float iw = a.inv_width, ih = a.inv_height;
    const float tu0 = s * ((((float)tile_x0 - 1.5f) * iw - 0.5f) * a.aspect), tu1 = s * ((((float)tile_x0 + 8.5f) * iw - 0.5f) * a.aspect);
    const float tv0 = s * (((float)tile_y0 - 1.5f) * ih - 0.5f), tv1 = s * (((float)tile_y0 + 8.5f) * ih - 0.5f);
    bool outside = (r.z < tu0) | (r.x > tu1) | (r.w < tv0) | (r.y > tv1);
    if (a.diagonals) {
        const float4 g = a.rects[2 * slot + 1];
        outside = outside | (g.y < tu0 + tv0) | (g.x > tu1 + tv1) | (g.w < tu0 - tv1) | (g.z > tu1 - tv0);
    }
    const bool keep = (lane < n) & !outside;
    return __ballot(keep);
}

// ---------------------------------------------------------------------------------------------
// One thread per pixel, wave = 8x8 tile, workgroup = one wave or a 32x8 strip; what else the kernel does is its policy P
// (KernelPolicy above; the product kernels' policies are listed there, the measurement arms' in rpt_diag_kernels.hip.h).
template <class P>
RPT_DEV void render_pixel_body(const KernelArgs &a) {
    const int lane = threadIdx.x & 63;
    // The product kernels are launched ONE WAVE per workgroup (blockDim 64, grid.x = tiles per row): a wave slot is handed back when
    // its wave ends, not when the longest of four neighbours does — next to a tile that walks for 70 us sit tiles that only store
    // (profiles/r03_one_wave_workgroups_ab.txt: bunny 4K in flight -8 %, one at a time -3 %).  The measurement arms keep 4 x 64.
    // (a sky split's launch covers the object box alone: its workgroup 0 of a row renders tile column tile_x0, 0 in every other launch)
    const int column = tile_origin_policy<P> ? (int)blockIdx.x + a.tile_x0 : (int)blockIdx.x;
    const int wave = P::one_wave ? (column & 3) : (int)(threadIdx.x >> 6);
    const int strip = P::one_wave ? (column >> 2) : (int)blockIdx.x;      // 32-pixel-wide strip of that row
#ifdef RPT_DIAGNOSTICS
    const DiagWaveClock diag_clock0 = diag_wave_begin<P::diag>();
#endif
    int tile_row = (int)blockIdx.y;              // 8-row tiles of this context, natural order
    if (P::band_first && a.first_h > 0) {
        // Workgroups are handed out in the order of their linear index, i.e. row of strips by row of strips.  One frame at a
        // time, what ends the frame is the last of its long waves, so the band of tile rows that holds the meshes goes first
        // (whole rows, in their natural order: neighbours stay neighbours) and the other rows follow in order.
        const int y = (int)blockIdx.y, rh = a.first_h;
        tile_row = y < rh ? a.first_ty + y : (y - rh < a.first_ty ? y - rh : y);
    }
    // lane -> pixel of the wave's 8x8 tile: row by row.  Diagnostics library, arms 641 / 653: along the Z curve, so that the four lanes the
    // memory pipeline handles together are a 2x2 block of pixels, not a 4x1 run (level, +1 % in flight at 4K and 8K: r03_td_bound.txt)
#ifdef RPT_DIAGNOSTICS
    const bool zorder_lanes = P::diag == 641 || P::diag == 653;
    const int col_in_tile = zorder_lanes ? ((lane & 1) | ((lane >> 1) & 2) | ((lane >> 2) & 4)) : (lane & 7);
    const int row_in_tile = zorder_lanes ? (((lane >> 1) & 1) | ((lane >> 2) & 2) | ((lane >> 3) & 4)) : (lane >> 3);
    const int x_coord = strip * 32 + wave * 8 + col_in_tile;
#else
    const int row_in_tile = lane >> 3;
    const int x_coord = strip * 32 + wave * 8 + (lane & 7);
#endif
    const int local_row = tile_row * RPT_TILE_ROWS + row_in_tile;
    const int global_tile = (tile_row >> a.run_log2) * a.tile_step + a.first_tile + (tile_row & ((1 << a.run_log2) - 1));
    const int y_coord = global_tile * RPT_TILE_ROWS + row_in_tile;
    // the wave's object mask comes from a __ballot over ALL 64 lanes (lane i answers for object i), so it is formed
    // before the lanes of a partial tile leave
    unsigned long long object_mask = ~0ull;
    if constexpr (P::camera == Camera::lens) {
        if (P::culled && P::object_mask) object_mask = wave_object_mask_lens(a, static_cast<const LensArgs &>(a).lens_scale, strip * 32 + wave * 8, global_tile * RPT_TILE_ROWS);
    } else if (P::culled && P::object_mask) object_mask = wave_object_mask(a, strip * 32 + wave * 8, global_tile * RPT_TILE_ROWS);
#ifdef RPT_DIAGNOSTICS
    if (P::diag == 10) object_mask = a.tile_masks[__builtin_amdgcn_readfirstlane(tile_row * a.mask_tiles_x + (int)blockIdx.x * 4 + wave)];   // the prepass's per-tile mask
#endif
    if (x_coord >= a.width || y_coord >= a.height) return;   // the reference has no guard (UB)
    object_mask = thin_object_mask<P>(a, object_mask, strip * 32 + wave * 8, global_tile * RPT_TILE_ROWS);

    f3 color;
    f3 mapped = mk3(0.0f, 0.0f, 0.0f);
    bool traced = false;
    [[maybe_unused]] DopplerRecord drec;
    uint32_t packed = a.bg_packed;
    [[maybe_unused]] bool no_ray = false;        // the ray-map camera only: this pixel's entry of the map is (0, 0, 0)
    const bool masked = (P::culled && P::object_mask) || P::diag == 10;
    if constexpr (P::camera == Camera::raymap) {
        // The direction is asked for first, next to the scalar load of the arguments' first line (nothing above reads memory: this
        // policy has no object mask), so its round trip overlaps everything up to its first use.  A pixel without a ray is {x, y, rgba =
        // 0, 0, 0, 1} with a zero debug_rgb triple, whatever the colour mode; a wave none of whose lanes has a ray stores that and ends
        // without reading the scene, as a wave with an empty object mask does.
        static_assert(!P::object_mask && !P::drec && P::diag == 0, "the ray-map kernels have no object mask, no Doppler record and no measurement arm");
        const RaymapArgs &ra = static_cast<const RaymapArgs &>(a);
        const float4 p = raymapLoad(ra.raymap, ra.raymap_pitch, x_coord, y_coord);
        const bool has_ray = raymapHasRay(p);
        no_ray = !has_ray;
        if (__ballot(has_ray) != 0ull && has_ray) {
            const f3 camdir = normalize(mk3(p.x, p.y, p.z));
            traced = trace<P>(a, camdir, object_mask, color);
            if constexpr (P::environment) {
                if (!traced) color = environment_colour(static_cast<const EnvironmentArgs &>(a), camdir);
                packed = tonemap_pack(a, color, mapped);
            } else if (traced) {
                packed = tonemap_pack(a, color, mapped);
            }
        } else {
            packed = 1u << 24;
        }
    } else if constexpr (P::environment) {
        // every pixel has a colour of its own: the camera direction is formed for all, and a wave whose object mask is empty goes
        // straight to the sky (no object loop, no scene load)
        f3 camdir;
        if constexpr (P::camera == Camera::equirect) camdir = equirectCamDir(static_cast<const PanoramaArgs &>(a), x_coord, y_coord);
        else if constexpr (P::camera == Camera::lens) camdir = lensCamRayDir((float)x_coord, (float)y_coord, a.width, a.height, a.aspect, static_cast<const LensArgs &>(a).lens_scale);
        else camdir = createCamRayDir((float)x_coord, (float)y_coord, a.width, a.height, a.aspect);
        if (!masked || object_mask != 0 || a.object_count > 64) traced = trace<P>(a, camdir, object_mask, color);
        if (!traced) color = environment_colour(static_cast<const EnvironmentArgs &>(a), camdir);
        packed = tonemap_pack(a, color, mapped);
    } else if (!masked || object_mask != 0 || a.object_count > 64) {
        f3 camdir;
        if constexpr (P::camera == Camera::equirect) camdir = equirectCamDir(static_cast<const PanoramaArgs &>(a), x_coord, y_coord);
        else if constexpr (P::camera == Camera::lens) camdir = lensCamRayDir((float)x_coord, (float)y_coord, a.width, a.height, a.aspect, static_cast<const LensArgs &>(a).lens_scale);
        else camdir = createCamRayDir((float)x_coord, (float)y_coord, a.width, a.height, a.aspect);
        if (trace<P>(a, camdir, object_mask, color, P::drec ? &drec : nullptr)) {
            packed = tonemap_pack(a, color, mapped);
            traced = true;
        }
    }

    const size_t id = (size_t)y_coord * a.width + x_coord;
    if constexpr (P::drec) {
        // {D_cam, D_light, reference colour, after the light factors, final linear colour}; a miss pixel: all zero (D_cam = 0)
        if (float *const rec_out = static_cast<const DopplerArgs &>(a).debug_doppler) {
            float *r = rec_out + (size_t)RPT_DOPPLER_RECORD * id;
            const float v[RPT_DOPPLER_RECORD] = {drec.dcam, drec.dlight, drec.ref.x, drec.ref.y, drec.ref.z, drec.lit.x, drec.lit.y, drec.lit.z,
                                                 color.x, color.y, color.z};
            for (int k = 0; k < RPT_DOPPLER_RECORD; k++) r[k] = traced ? v[k] : 0.0f;
        }
    }
#ifdef RPT_DIAGNOSTICS
    if (P::diag == 785 && object_mask == 0ull) return;      // EXPERIMENT (wrong image): what do the sky tiles' stores cost the walks?
#endif
    if (a.out16) store_pixel(a.out16, id, __float_as_uint((float)x_coord), __float_as_uint((float)y_coord), packed, 0u);
    // (the 4-byte plane likewise: measured against the default policy on a rank's share of the frame, bunny 4K 0.0581 -> 0.0566 ms, shadows the same)
    if (a.plane) __builtin_nontemporal_store(packed, a.plane + (size_t)local_row * a.width + x_coord);
    if (a.debug_rgb) {
        if (!traced && !P::environment && !no_ray) mapped = mk3(a.bg_mapped[0], a.bg_mapped[1], a.bg_mapped[2]);      // (read here only: a miss pixel's store needs nothing beyond the first line of the arguments)
        a.debug_rgb[3 * id + 0] = mapped.x;
        a.debug_rgb[3 * id + 1] = mapped.y;
        a.debug_rgb[3 * id + 2] = mapped.z;
    }
#ifdef RPT_DIAGNOSTICS
    diag_wave_end<P::diag>(a, diag_clock0);
#endif
}

// opencl_kernel.cl:641-648 with MSAASAMPLES = a.msaa > 1 (a compile-time constant of the reference, 1 as shipped; rpt_set_msaa): a.msaa^2
// camera rays per pixel at (x + sx/n, y + sy/n), colours summed in the reference's order (a miss contributes the background of :565)
// and divided by n^2 before the tonemap.  A function of its own so that the one-sample kernels stay what they are.  Ballot: the
// wave's object mask as in render_pixel_body — the tile it is tested against is grown by a pixel and a half, the samples stay
// within one pixel; Unculled: no cull (what rpt_verify_frame compares with).
template <class P>
RPT_DEV void render_pixel_body_msaa(const KernelArgs &a) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)blockIdx.x & 3;              // one wave per workgroup, as the one-sample product kernels
    const int tile_row = (int)blockIdx.y;
    const int strip = (int)blockIdx.x >> 2;
    const int row_in_tile = lane >> 3;
    const int x_coord = strip * 32 + wave * 8 + (lane & 7);
    const int local_row = tile_row * RPT_TILE_ROWS + row_in_tile;
    const int global_tile = (tile_row >> a.run_log2) * a.tile_step + a.first_tile + (tile_row & ((1 << a.run_log2) - 1));
    const int y_coord = global_tile * RPT_TILE_ROWS + row_in_tile;
    unsigned long long object_mask = ~0ull;
    if (P::culled) object_mask = wave_object_mask(a, strip * 32 + wave * 8, global_tile * RPT_TILE_ROWS);
    if (x_coord >= a.width || y_coord >= a.height) return;
    const bool any = !P::culled || object_mask != 0 || a.object_count > 64;
    const int n = a.msaa;
    f3 sum = mk3(0.0f, 0.0f, 0.0f);
    for (int sy = 0; sy < n; sy++) {
        for (int sx = 0; sx < n; sx++) {
            f3 c = mk3(0.15f, 0.15f, 0.25f);
            if (any) {
                const f3 camdir = createCamRayDir((float)x_coord + (float)sx / (float)n, (float)y_coord + (float)sy / (float)n, a.width, a.height, a.aspect);
                f3 traced;
                if (trace<P>(a, camdir, object_mask, traced)) c = traced;
            }
            sum = sum + c;
        }
    }
    const float n2 = (float)(n * n);
    sum = mk3(sum.x / n2, sum.y / n2, sum.z / n2);
    f3 mapped;
    const uint32_t packed = tonemap_pack(a, sum, mapped);
    const size_t id = (size_t)y_coord * a.width + x_coord;
    if (a.out16) store_pixel(a.out16, id, __float_as_uint((float)x_coord), __float_as_uint((float)y_coord), packed, 0u);
    if (a.plane) __builtin_nontemporal_store(packed, a.plane + (size_t)local_row * a.width + x_coord);
    if (a.debug_rgb) {
        a.debug_rgb[3 * id + 0] = mapped.x;
        a.debug_rgb[3 * id + 1] = mapped.y;
        a.debug_rgb[3 * id + 2] = mapped.z;
    }
}

// ---- The event pass (rpt_render_events; not in the reference; DESIGN.md "Event pass") -----------------------------------------------
// A second kind of frame: per pixel the object the primary ray hits first, the distance, the emission event in that object's rest
// frame and the surface (u, v) — what trace() computes on its way to a colour and drops.  The arguments are LensArgs with the
// record pointer appended (every camera's kernels take them: doppler = 0, env_texels unused), so no other kernel's argument block
// changes.
struct EventArgs : LensArgs {
    rpt_event *events;              // [width * height] full-frame addressing, whatever the context's colour_plane says
};
// ... and the ray-map camera's event kernels (rpt_set_raymap): EventArgs with the map appended (RaymapArgs' two fields), a block of its own
// so that EventArgs, and every event kernel that takes it, stays what it was
struct RaymapEventArgs : EventArgs {
    const float4 *raymap;
    int raymap_pitch;
};

// sphere_core leaves (u, v) out for an untextured sphere (only the texture fetch reads it in a frame); the record holds Hit.uv of
// every winner, so for such a winner the sphere's test is repeated once, after the loop, with want_uv set: the same float
// operations on the same inputs as intersect_object_primary's, hence the same objPt, and the oracle's two lines on it.
RPT_DEV f2 primary_sphere_uv(const KernelArgs &a, int i, f4 rayDir) {
    const rpt_object &obj = a.objects[i];
    const DObj &pre = a.dobjs[i];
    const f3 d3 = mk3(dot(ld4(obj.Lorentz[1]), rayDir), dot(ld4(obj.Lorentz[2]), rayDir), dot(ld4(obj.Lorentz[3]), rayDir));
    f3 dir = transformDirection(obj.InvM, d3);
    const float scale = length(dir);
    dir = dir / scale;
    Hit h;
    h.dist = 1e20f;
    h.uv.x = h.uv.y = 0.0f;
    sphere_core(obj, -mk3(pre.ox, pre.oy, pre.oz), pre.sphere_c, dir, scale, h, true);
    return h.uv;
}

// One lane's 32-B record as two 16-byte NON-TEMPORAL stores (store_pixel's reason: written once, never read by these kernels; a
// 4K event frame is 265 MB against 4 MB of L2 per XCD).  A wave's 8 x 8 tile is eight runs of 256 contiguous bytes.
RPT_DEV void store_event(rpt_event *events, size_t id, int object, float dist, f4 ev, f2 uv) {
    typedef unsigned int v4u __attribute__((ext_vector_type(4)));
    v4u lo, hi;
    lo.x = (unsigned int)object; lo.y = __float_as_uint(dist); lo.z = __float_as_uint(ev.x); lo.w = __float_as_uint(ev.y);
    hi.x = __float_as_uint(ev.z); hi.y = __float_as_uint(ev.w); hi.z = __float_as_uint(uv.x); hi.w = __float_as_uint(uv.y);
    v4u *p = reinterpret_cast<v4u *>(events) + 2 * id;
    __builtin_nontemporal_store(lo, p);
    __builtin_nontemporal_store(hi, p + 1);
}

// render_pixel_body's geometry (one wave per workgroup, the 8 x 8 tile, the same row and tile arithmetic, the object mask formed
// before partial lanes leave, the same three camera-direction functions), then trace()'s closest-hit loop — the same
// intersect_object_primary<P>, the same strict <, the same object order, so ties break as in the frame — and after it only the
// four-component event.  No texture fetch, flash, lights, shadow rays or tonemap.  The loop is a SECOND COPY of trace()'s (not
// factored out of it): trace() and every render kernel stay the source, and the machine code, they were.
template <class P>
RPT_DEV void events_pixel_body(const EventArgs &a) {
    const int lane = threadIdx.x & 63;
    const int wave = (int)blockIdx.x & 3;
    const int strip = (int)blockIdx.x >> 2;
    const int tile_row = (int)blockIdx.y;
    const int row_in_tile = lane >> 3;
    const int x_coord = strip * 32 + wave * 8 + (lane & 7);
    const int global_tile = (tile_row >> a.run_log2) * a.tile_step + a.first_tile + (tile_row & ((1 << a.run_log2) - 1));
    const int y_coord = global_tile * RPT_TILE_ROWS + row_in_tile;
    unsigned long long object_mask = ~0ull;
    if constexpr (P::camera == Camera::lens) {
        if (P::culled && P::object_mask) object_mask = wave_object_mask_lens(a, a.lens_scale, strip * 32 + wave * 8, global_tile * RPT_TILE_ROWS);
    } else if (P::culled && P::object_mask) object_mask = wave_object_mask(a, strip * 32 + wave * 8, global_tile * RPT_TILE_ROWS);
    if (x_coord >= a.width || y_coord >= a.height) return;

    int object = -1;
    float dist = 0.0f;
    f4 ev = mk4(0.0f, 0.0f, 0.0f, 0.0f);
    f2 uv;
    uv.x = uv.y = 0.0f;
    const bool masked = P::culled && P::object_mask;
    [[maybe_unused]] float4 map_p;
    bool has_ray = true;
    if constexpr (P::camera == Camera::raymap) {        // (asked for first; a pixel without a ray is a miss record, and a wave without any reads no scene)
        const RaymapEventArgs &ra = static_cast<const RaymapEventArgs &>(a);
        map_p = raymapLoad(ra.raymap, ra.raymap_pitch, x_coord, y_coord);
        has_ray = raymapHasRay(map_p);
        has_ray = __ballot(has_ray) != 0ull && has_ray;
    }
    if (has_ray && (!masked || object_mask != 0 || a.object_count > 64)) {       // (a wave whose mask is empty stores miss records without reading the scene)
        f3 camdir;
        if constexpr (P::camera == Camera::raymap) camdir = normalize(mk3(map_p.x, map_p.y, map_p.z));
        else if constexpr (P::camera == Camera::equirect) camdir = equirectCamDir(a, x_coord, y_coord);
        else if constexpr (P::camera == Camera::lens) camdir = lensCamRayDir((float)x_coord, (float)y_coord, a.width, a.height, a.aspect, a.lens_scale);
        else camdir = createCamRayDir((float)x_coord, (float)y_coord, a.width, a.height, a.aspect);
        const float inf = 1e20f;
        Hit hit;
        hit.dist = inf;
        hit.uv.x = hit.uv.y = 0.0f;
        hit.object = -1;
        const f3 nd = normalize(camdir);
        const f4 rayDir = mk4((float)a.interval, nd.x, nd.y, nd.z);
        for (int i = 0; i < a.object_count; i++) {
            if (i < 64 && !((object_mask >> i) & 1ull)) continue;
            Hit newHit;
            newHit.dist = inf;
            if (intersect_object_primary<P>(a, i, rayDir, newHit)) {
                if constexpr (P::windowed) {     // (trace()'s own test: the winner's event[0] below is this float)
                    if (newHit.dist < hit.dist && window_accepts(a.dobjs[i], a.objects[i].stationaryCam.x + dot(ld4(a.objects[i].Lorentz[0]), rayDir) * newHit.dist)) {
                        hit = newHit;
                        hit.object = i;
                    }
                } else if (newHit.dist < hit.dist) {
                    hit = newHit;
                    hit.object = i;
                }
            }
        }
        if (hit.object >= 0) {
            const rpt_object &ho = a.objects[hit.object];
            if (ho.type == RPT_SPHERE && ho.textureIndex == -1) hit.uv = primary_sphere_uv(a, hit.object, rayDir);
            // opencl_kernel.cl:396: event = newEvent0 + lightDir * newHit.dist, lightDir = Lorentz * (interval, nd) (:386-388)
            const f4 lightDir = transformPoint4D(ho.Lorentz, rayDir);
            ev = ld4(ho.stationaryCam) + lightDir * hit.dist;
            object = hit.object;
            dist = hit.dist;
            uv = hit.uv;
        }
    }
    store_event(a.events, (size_t)y_coord * a.width + x_coord, object, dist, ev, uv);
}

#ifndef RPT_RELAXED_FP    /* rpt_relaxed.hip instantiates its own two kernels and nothing else from here on */
// Product kernels (rpt_set_variant; the number in the comment is the variant).
__global__ __launch_bounds__(64) void rpt_render_kernel_v0(const KernelArgs a) { render_pixel_body<RefLayout>(a); }                                                              // 1: any valid octree
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_unculled_w5(const KernelArgs a) { render_pixel_body<Unculled>(a); }         // 3: no cull (rpt_verify_frame; the escape hatch)
// the wave's object mask from the per-object screen rectangles by lane-parallel test + __ballot; SIX waves per SIMD without scratch: the
// shading state waits in LDS across the shadow walks (BallotExactParked).  The name's suffix is history: bench.py and
// the counter summaries are keyed by it.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_render_kernel_ballot_w5(const KernelArgs a) { render_pixel_body<BallotExactParked>(a); }    // 41 = rpt_render_async
// the same with the tile rows that hold the meshes dispatched first and the latency walk (44 B of scratch): latency, not throughput
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_ballot_first_w5(const KernelArgs a) { render_pixel_body<BallotFirstExact>(a); }    // 43 = the blocking rpt_render; rpt_render_async below RPT_LATENCY_KERNEL_MAX_PIXELS
// 41 and 43 above take the triangle test's 1 / det through rcp_exact (BallotExact / BallotFirstExact); these two keep the IEEE division, for scenes
// outside rcp_exact's domain (rpt_scene_exact_rcp) and as variants 48 / 49
// (48 goes with 41: six waves per SIMD and the parking, 80 registers and no scratch where five waves had 12 B; 49 stays what it was)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_render_kernel_ballot_ieee_w5(const KernelArgs a) { render_pixel_body<BallotParked>(a); }  // 48 (and 41 outside the domain)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_ballot_first_ieee_w5(const KernelArgs a) { render_pixel_body<BallotFirst>(a); }  // 49 (and 43 outside the domain)
// without the octree walk compiled in, for frames whose Object[] holds no mesh: 61 VGPRs, no scratch, EIGHT waves per SIMD
// (arch 1080p 0.0370 -> 0.0301 ms per frame in flight, cubes.txt 4K 0.0898 -> 0.0725)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_analytic_w8(const KernelArgs a) { render_pixel_body<Analytic>(a); }        // 44

// The sky fill of a split frame (rpt_api.hip: launch): every pixel of the frame OUTSIDE the object box, written as the
// render kernels write a pixel whose wave's object mask is empty — {(float)x, (float)y, bg_packed, 0}, store_pixel's non-temporal
// 16-byte store — by a kernel that reads no scene memory (its arguments are all it knows) and needs a dozen registers, so that its waves
// fit into the registers and the wave slots the walkers leave free on a SIMD (six walkers at 80 registers: 32 registers and two slots,
// two waves of the fill's 16; five at 96 left 32 and three).  The render kernels then run over the box alone.
// One wave per row of RPT_SKY_FILL_TILES 8x8 tiles: lane -> pixel of a tile row by row, as in the render kernels, so each store
// instruction of a wave is eight full 128-byte lines, and a wave's stores run along 64 x 16 B = 1 KB of each of its eight pixel rows.
// The box is whole tiles and every test of it is wave-uniform; a pixel beyond the frame's right or lower edge is never written.
#define RPT_SKY_FILL_TILES 8
struct SkyFillArgs {
    rpt_pixel *out16;               // the 16 B/pixel framebuffer, full-frame addressing
    int width, height;
    uint32_t bg_packed;             // KernelArgs::bg_packed
    int tx0, ty0, tx1, ty1;         // the object box [tx0, tx1) x [ty0, ty1) in 8x8 tiles: not written here; tx0 >= tx1: no box, the whole frame
};
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_sky_fill_kernel(const SkyFillArgs a) {
    const int lane = threadIdx.x & 63;
    const int ty = (int)blockIdx.y, tx_first = (int)blockIdx.x * RPT_SKY_FILL_TILES;
    const bool box_rows = ty >= a.ty0 && ty < a.ty1;
    if (box_rows && tx_first >= a.tx0 && tx_first + RPT_SKY_FILL_TILES <= a.tx1) return;       // the whole run lies in the box
    const int y = ty * RPT_TILE_ROWS + (lane >> 3);
    if (y >= a.height) return;
    const uint32_t fy = __float_as_uint((float)y);
    const size_t row = (size_t)y * a.width;
#pragma unroll
    for (int k = 0; k < RPT_SKY_FILL_TILES; k++) {
        const int tx = tx_first + k, x = tx * 8 + (lane & 7);
        const bool in_box = box_rows && tx >= a.tx0 && tx < a.tx1;
        if (!in_box && x < a.width) store_pixel(a.out16, row + x, __float_as_uint((float)x), fy, a.bg_packed, 0u);
    }
}

// MSAASAMPLES > 1 (rpt_set_msaa): culled and un-culled; rpt_last_variant reports them as 46 / 47
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_msaa_w5(const KernelArgs a) { render_pixel_body_msaa<Ballot>(a); }            // 46
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_msaa_unculled_w5(const KernelArgs a) { render_pixel_body_msaa<Unculled>(a); }    // 47

// Doppler twins (rpt_set_doppler != 0; not in the reference): the kernels above with the colour operator compiled in, launched with
// the same shapes and occupancies.  The variant numbers rpt_last_variant reports are the twinned kernel's + 200; 241 / 243 fall back
// to 248's / 249's code outside the exact reciprocal's domain as 41 / 43 do.  Variants 1, 50, 51 and MSAA > 1 have no twin.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_unculled_doppler_w5(const DopplerArgs a) { render_pixel_body<DopplerTwin<Unculled>>(a); }         // 203
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_ballot_doppler_w5(const DopplerArgs a) { render_pixel_body<DopplerTwin<BallotExact>>(a); }          // 241
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_ballot_first_doppler_w5(const DopplerArgs a) { render_pixel_body<DopplerTwin<BallotFirstExact>>(a); }    // 243
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_ballot_ieee_doppler_w5(const DopplerArgs a) { render_pixel_body<DopplerTwin<Ballot>>(a); }     // 248
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_ballot_first_ieee_doppler_w5(const DopplerArgs a) { render_pixel_body<DopplerTwin<BallotFirst>>(a); }  // 249
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_analytic_doppler_w8(const DopplerArgs a) { render_pixel_body<DopplerTwin<Analytic>>(a); }     // 244
// the Doppler debug kernel (rpt_set_debug_doppler): 203 that also writes the per-pixel record; launched instead of any twin while the hook is set
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_doppler_record_w5(const DopplerArgs a) { render_pixel_body<DopplerRecorded>(a); }   // 240

// Panorama kernels (rpt_set_projection with RPT_PROJECTION_EQUIRECT; not in the reference): the product kernels' shapes and occupancies
// with the equirectangular camera and without the object mask.  341 takes 1 / det through rcp_exact like 41, with its IEEE form for
// scenes outside the domain; 5xx are the Doppler twins, 540 the un-culled Doppler debug kernel.  DESIGN.md "Panorama camera".
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_pano_w5(const PanoramaArgs a) { render_pixel_body<PanoramaWalk>(a); }                       // 341
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_pano_ieee_w5(const PanoramaArgs a) { render_pixel_body<PanoramaWalkIeee>(a); }              // (341)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_pano_analytic_w8(const PanoramaArgs a) { render_pixel_body<PanoramaAnalytic>(a); }          // 344
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_pano_unculled_w5(const PanoramaArgs a) { render_pixel_body<PanoramaUnculled>(a); }          // 303
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_pano_doppler_w5(const PanoramaArgs a) { render_pixel_body<DopplerTwin<PanoramaWalk>>(a); }        // 541
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_pano_ieee_doppler_w5(const PanoramaArgs a) { render_pixel_body<DopplerTwin<PanoramaWalkIeee>>(a); } // (541)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_pano_analytic_doppler_w8(const PanoramaArgs a) { render_pixel_body<DopplerTwin<PanoramaAnalytic>>(a); } // 544
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_pano_unculled_doppler_w5(const PanoramaArgs a) { render_pixel_body<DopplerTwin<PanoramaUnculled>>(a); } // 503
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_pano_doppler_record_w5(const PanoramaArgs a) { render_pixel_body<PanoramaRecorded>(a); }      // 540

// Environment kernels (rpt_set_environment; not in the reference): the kernels variant 0 can select and the un-culled one, pinhole (6xx)
// and panorama (7xx), each serving Doppler off and on through the run-time flag.  DESIGN.md "Environment map".
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_unculled_w5(const EnvironmentArgs a) { render_pixel_body<Environment<Unculled>>(a); }                  // 603
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_ballot_w5(const EnvironmentArgs a) { render_pixel_body<Environment<BallotExact>>(a); }                 // 641
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_ballot_ieee_w5(const EnvironmentArgs a) { render_pixel_body<Environment<Ballot>>(a); }                 // (641)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_ballot_first_w5(const EnvironmentArgs a) { render_pixel_body<Environment<BallotFirstExact>>(a); }      // 643
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_ballot_first_ieee_w5(const EnvironmentArgs a) { render_pixel_body<Environment<BallotFirst>>(a); }      // (643)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_env_analytic_w8(const EnvironmentArgs a) { render_pixel_body<Environment<Analytic>>(a); }                  // 644
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_pano_unculled_w5(const EnvironmentArgs a) { render_pixel_body<Environment<PanoramaUnculled>>(a); }     // 703
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_pano_w5(const EnvironmentArgs a) { render_pixel_body<Environment<PanoramaWalk>>(a); }                  // 741
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_env_pano_ieee_w5(const EnvironmentArgs a) { render_pixel_body<Environment<PanoramaWalkIeee>>(a); }         // (741)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_env_pano_analytic_w8(const EnvironmentArgs a) { render_pixel_body<Environment<PanoramaAnalytic>>(a); }     // 744

// Lens kernels (rpt_set_field_of_view; not in the reference): what variant 0 can select (41 / 43 / 44, with the IEEE forms) and the un-culled
// kernel (3), with the image plane scaled; then their Doppler twins and their environment forms, as the families above.  Same launch shapes
// and occupancy attributes as the kernels they stand in for.  DESIGN.md "Free-look camera".
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_unculled_w5(const LensArgs a) { render_pixel_body<Lens<Unculled>>(a); }    // 803
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_ballot_w5(const LensArgs a) { render_pixel_body<Lens<BallotExact>>(a); }    // 841
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_ballot_ieee_w5(const LensArgs a) { render_pixel_body<Lens<Ballot>>(a); }    // (841)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_ballot_first_w5(const LensArgs a) { render_pixel_body<Lens<BallotFirstExact>>(a); }    // 843
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_ballot_first_ieee_w5(const LensArgs a) { render_pixel_body<Lens<BallotFirst>>(a); }    // (843)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_lens_analytic_w8(const LensArgs a) { render_pixel_body<Lens<Analytic>>(a); }    // 844
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_doppler_unculled_w5(const LensArgs a) { render_pixel_body<Lens<DopplerTwin<Unculled>>>(a); }    // 813
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_doppler_ballot_w5(const LensArgs a) { render_pixel_body<Lens<DopplerTwin<BallotExact>>>(a); }    // 851
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_doppler_ballot_ieee_w5(const LensArgs a) { render_pixel_body<Lens<DopplerTwin<Ballot>>>(a); }    // (851)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_doppler_ballot_first_w5(const LensArgs a) { render_pixel_body<Lens<DopplerTwin<BallotFirstExact>>>(a); }    // 853
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_doppler_ballot_first_ieee_w5(const LensArgs a) { render_pixel_body<Lens<DopplerTwin<BallotFirst>>>(a); }    // (853)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_lens_doppler_analytic_w8(const LensArgs a) { render_pixel_body<Lens<DopplerTwin<Analytic>>>(a); }    // 854
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_env_unculled_w5(const LensArgs a) { render_pixel_body<Lens<Environment<Unculled>>>(a); }    // 823
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_env_ballot_w5(const LensArgs a) { render_pixel_body<Lens<Environment<BallotExact>>>(a); }    // 861
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_env_ballot_ieee_w5(const LensArgs a) { render_pixel_body<Lens<Environment<Ballot>>>(a); }    // (861)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_env_ballot_first_w5(const LensArgs a) { render_pixel_body<Lens<Environment<BallotFirstExact>>>(a); }    // 863
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_lens_env_ballot_first_ieee_w5(const LensArgs a) { render_pixel_body<Lens<Environment<BallotFirst>>>(a); }    // (863)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_lens_env_analytic_w8(const LensArgs a) { render_pixel_body<Lens<Environment<Analytic>>>(a); }    // 864

// Ray-map kernels (rpt_set_raymap with RPT_PROJECTION_RAYMAP; not in the reference): the panorama kernels' shapes and occupancies with the
// direction of every pixel read from the context's map.  No band-first form and no forced-IEEE arms, as in panorama; the walk takes 1 / det
// through rcp_exact like 41, with its IEEE form for scenes outside the domain.  12xx plain, + 10 the Doppler twins, + 20 the environment
// forms.  DESIGN.md "Ray-map camera".
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_unculled_w5(const RaymapArgs a) { render_pixel_body<Raymap<Unculled>>(a); }    // 1203
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_walk_w5(const RaymapArgs a) { render_pixel_body<Raymap<BallotExact>>(a); }    // 1241
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_walk_ieee_w5(const RaymapArgs a) { render_pixel_body<Raymap<Ballot>>(a); }    // (1241)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_raymap_analytic_w8(const RaymapArgs a) { render_pixel_body<Raymap<Analytic>>(a); }    // 1244
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_doppler_unculled_w5(const RaymapArgs a) { render_pixel_body<DopplerTwin<Raymap<Unculled>>>(a); }    // 1213
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_doppler_walk_w5(const RaymapArgs a) { render_pixel_body<DopplerTwin<Raymap<BallotExact>>>(a); }    // 1251
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_doppler_walk_ieee_w5(const RaymapArgs a) { render_pixel_body<DopplerTwin<Raymap<Ballot>>>(a); }    // (1251)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_raymap_doppler_analytic_w8(const RaymapArgs a) { render_pixel_body<DopplerTwin<Raymap<Analytic>>>(a); }    // 1254
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_env_unculled_w5(const RaymapArgs a) { render_pixel_body<Environment<Raymap<Unculled>>>(a); }    // 1223
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_env_walk_w5(const RaymapArgs a) { render_pixel_body<Environment<Raymap<BallotExact>>>(a); }    // 1261
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_raymap_env_walk_ieee_w5(const RaymapArgs a) { render_pixel_body<Environment<Raymap<Ballot>>>(a); }    // (1261)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_raymap_env_analytic_w8(const RaymapArgs a) { render_pixel_body<Environment<Raymap<Analytic>>>(a); }    // 1264

// Event kernels (rpt_render_events; not in the reference): the product kernels' launch shape, the record instead of a colour.  The number
// is what rpt_last_events_variant reports.  Only the throughput walk is built; 941 / 911 / 921 take 1 / det through rcp_exact like 41,
// with an IEEE form each for scenes outside the domain.  The panorama needs no un-culled form: it has no object mask and the pass has no
// shadow rays, so nothing is culled there.  DESIGN.md "Event pass".
// Occupancy (make asm; profiles/r09_events_kernel_resources.txt): the walk forms need 79-81 VGPRs, 102-106 SGPRs and no scratch when
// asked for five waves per SIMD as the render kernels are — without the shading state they sit one 8-register granule below the
// 88-register step, so SIX waves fit (512 / 6 = 85 -> 80 VGPRs: 79-80 used, still no scratch); seven would need <= 72 and spill.  The
// forms without the walk need 44-46 VGPRs, 78 SGPRs, no scratch: EIGHT waves, the most a SIMD holds, as kernel 44.
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_unculled(const EventArgs a) { events_pixel_body<Unculled>(a); }    // 903
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_ballot(const EventArgs a) { events_pixel_body<BallotExact>(a); }    // 941
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_ballot_ieee(const EventArgs a) { events_pixel_body<Ballot>(a); }    // (941)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_events_kernel_analytic(const EventArgs a) { events_pixel_body<Analytic>(a); }    // 944
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_pano(const EventArgs a) { events_pixel_body<PanoramaWalk>(a); }    // 911
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_pano_ieee(const EventArgs a) { events_pixel_body<PanoramaWalkIeee>(a); }    // (911)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_events_kernel_pano_analytic(const EventArgs a) { events_pixel_body<PanoramaAnalytic>(a); }    // 914
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_lens_unculled(const EventArgs a) { events_pixel_body<Lens<Unculled>>(a); }    // 923
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_lens_ballot(const EventArgs a) { events_pixel_body<Lens<BallotExact>>(a); }    // 921
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_lens_ballot_ieee(const EventArgs a) { events_pixel_body<Lens<Ballot>>(a); }    // (921)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_events_kernel_lens_analytic(const EventArgs a) { events_pixel_body<Lens<Analytic>>(a); }    // 924

// ... and the ray-map camera's (no un-culled form either: nothing is masked)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_raymap(const RaymapEventArgs a) { events_pixel_body<Raymap<BallotExact>>(a); }    // 1291
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_raymap_ieee(const RaymapEventArgs a) { events_pixel_body<Raymap<Ballot>>(a); }    // (1291)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_events_kernel_raymap_analytic(const RaymapEventArgs a) { events_pixel_body<Raymap<Analytic>>(a); }    // 1294

// Windowed kernels (rpt_set_object_windows; not in the reference): Windowed<P> over the lens kernels (the pinhole's too, at lens_scale
// 1.0f), the panorama's and the ray map's, each as the Doppler twin with the run-time flag (plain: doppler = 0) and as the sky form; un-culled,
// the walk with its IEEE form, and without the walk.  No band-first form: such a choice gets the walk.  Same launch shapes, argument
// blocks and occupancy attributes as the kernels they wrap.  DESIGN.md "Time windows".
#define RPT_WINDOWED_FAMILY(name, ARGS, UNC, WALK, IEEE, ANA)                                                                                              \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_win_##name##_unculled_w5(const ARGS a) { render_pixel_body<Windowed<UNC>>(a); }    \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_win_##name##_walk_w5(const ARGS a) { render_pixel_body<Windowed<WALK>>(a); }       \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_render_kernel_win_##name##_walk_ieee_w5(const ARGS a) { render_pixel_body<Windowed<IEEE>>(a); }  \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_render_kernel_win_##name##_analytic_w8(const ARGS a) { render_pixel_body<Windowed<ANA>>(a); }
RPT_WINDOWED_FAMILY(lens, LensArgs, Lens<DopplerTwin<Unculled>>, Lens<DopplerTwin<BallotExact>>, Lens<DopplerTwin<Ballot>>, Lens<DopplerTwin<Analytic>>)                        // 2803.. / 2813..
RPT_WINDOWED_FAMILY(lens_env, LensArgs, Lens<Environment<Unculled>>, Lens<Environment<BallotExact>>, Lens<Environment<Ballot>>, Lens<Environment<Analytic>>)                    // 2823..
RPT_WINDOWED_FAMILY(pano, PanoramaArgs, DopplerTwin<PanoramaUnculled>, DopplerTwin<PanoramaWalk>, DopplerTwin<PanoramaWalkIeee>, DopplerTwin<PanoramaAnalytic>)                 // 2303.. / 2503..
RPT_WINDOWED_FAMILY(pano_env, EnvironmentArgs, Environment<PanoramaUnculled>, Environment<PanoramaWalk>, Environment<PanoramaWalkIeee>, Environment<PanoramaAnalytic>)          // 2703..
RPT_WINDOWED_FAMILY(raymap, RaymapArgs, DopplerTwin<Raymap<Unculled>>, DopplerTwin<Raymap<BallotExact>>, DopplerTwin<Raymap<Ballot>>, DopplerTwin<Raymap<Analytic>>)             // 3203.. / 3213..
RPT_WINDOWED_FAMILY(raymap_env, RaymapArgs, Environment<Raymap<Unculled>>, Environment<Raymap<BallotExact>>, Environment<Raymap<Ballot>>, Environment<Raymap<Analytic>>)         // 3223..
#undef RPT_WINDOWED_FAMILY
// ... and the windowed event kernels: the event kernels' policies wrapped (the lens forms serve the pinhole), their occupancies kept
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_win_lens_unculled(const EventArgs a) { events_pixel_body<Windowed<Lens<Unculled>>>(a); }    // 2903 / 2923
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_win_lens_walk(const EventArgs a) { events_pixel_body<Windowed<Lens<BallotExact>>>(a); }    // 2941 / 2921
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_win_lens_walk_ieee(const EventArgs a) { events_pixel_body<Windowed<Lens<Ballot>>>(a); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_events_kernel_win_lens_analytic(const EventArgs a) { events_pixel_body<Windowed<Lens<Analytic>>>(a); }    // 2944 / 2924
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_win_pano_walk(const EventArgs a) { events_pixel_body<Windowed<PanoramaWalk>>(a); }    // 2911
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_win_pano_walk_ieee(const EventArgs a) { events_pixel_body<Windowed<PanoramaWalkIeee>>(a); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_events_kernel_win_pano_analytic(const EventArgs a) { events_pixel_body<Windowed<PanoramaAnalytic>>(a); }    // 2914
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_win_raymap_walk(const RaymapEventArgs a) { events_pixel_body<Windowed<Raymap<BallotExact>>>(a); }    // 3291
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(6, 6))) void rpt_events_kernel_win_raymap_walk_ieee(const RaymapEventArgs a) { events_pixel_body<Windowed<Raymap<Ballot>>>(a); }
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_events_kernel_win_raymap_analytic(const RaymapEventArgs a) { events_pixel_body<Windowed<Raymap<Analytic>>>(a); }    // 3294

// ---- Adaptive anti-aliasing (rpt_set_adaptive_aa; not in the reference; DESIGN.md "Adaptive anti-aliasing") ------------------------------
// The second launch of an adaptive frame.  The first is the one-sample kernel a frame gets anyway (its source and its code untouched),
// told to write its packed colours into a context-owned 4 B/pixel plane beside the framebuffer; this kernel reads that plane, decides
// per pixel whether it lies on an edge, and re-renders the pixels that do with n x n camera rays in the order of opencl_kernel.cl:641-648.
// The arguments are LensArgs with the pass's own fields appended (every camera's and every colour family's refine kernel takes them),
// so no other kernel's argument block changes.
struct RefineArgs : LensArgs {
    const uint32_t *aa_plane;       // [height][width] the packed colours of the one-sample pass (read only here: a neighbour's tile reads them too)
    unsigned long long *aa_refined; // the context's counter of refined pixels: one atomic add per wave that refined anything
    const float2 *aa_cols;          // panorama: rpt_projection_tables at n width x n height, [n width] {sin, cos} of a sample column's longitude
    const float2 *aa_rows;          // ... and [n height] of a sample row's latitude
    int aa_n;                       // samples per axis, 2..8
    int aa_threshold;               // refine where a neighbour's 8-bit R, G or B differs by MORE than this: -1 = everywhere, 255 = nowhere
};

// the largest of |R - R'|, |G - G'|, |B - B'| of two packed colours
RPT_DEV int packed_rgb_distance(uint32_t p, uint32_t q) {
    int d = 0;
    for (int c = 0; c < 3; c++) {
        const int e = (int)((p >> (8 * c)) & 255u) - (int)((q >> (8 * c)) & 255u);
        const int m = e < 0 ? -e : e;
        d = m > d ? m : d;
    }
    return d;
}

RPT_DEV int max_int(int x, int y) { return x < y ? y : x; }

// the index of the k-th set bit of m (k counted from 0; k < popcount(m)): six halving steps on the population count
RPT_DEV int nth_set_bit(unsigned long long m, int k) {
    int pos = 0;
    for (int width = 32; width >= 1; width >>= 1) {
        const int below = __popcll((m >> pos) & ((1ull << width) - 1ull));
        if (k >= below) { k -= below; pos += width; }
    }
    return pos;
}

// One wave per 8 x 8 tile, as every render kernel (whole-frame contexts only: the host refuses rpt_set_rows, so local rows are the frame's).
//   1. Each lane compares its own packed colour with those of x +- 1 and y +- 1 IN THE PLANE (never the framebuffer this pass rewrites;
//      neighbours outside the frame are ignored); one __ballot makes the wave's refine set, and a wave whose set is empty ends there —
//      before it has read a rectangle, an object or a table.
//   2. The (pixel, sample) pairs of the set are spread over all 64 lanes, floor(64 / n^2) pixels per round: lane L of a round traces
//      sample L mod n^2 of the round's pixel number L / n^2, found by rank in the ballot (nth_set_bit) — a pixel is never a loop of n^2
//      traces in one lane while the others idle.  trace<P> and the wave's object mask are the one-sample kernels' own.
//   3. The n^2 colours of a pixel are handed to the lane that traced its sample 0 through 1 KB of LDS (one 16-B write per lane, n^2
//      16-B reads per owner; DESIGN.md says why not shuffles); that lane adds them IN THE REFERENCE'S ORDER — sy outer, sx inner, one
//      float addition after another: a tree or a DPP reduction would change the bits — divides by n^2, maps, packs and stores.
// The object mask and the sample positions.  Sample (sx, sy) of pixel (x, y) is at xs = fl((float)x + fl(sx / n)), 0 <= sx / n <= 7/8:
// x <= xs <= x + 1 (rounding is monotone), off its exact place by at most half an ulp of xs, i.e. 2^-5 pixel while the frame is at most
// 2^20 pixels wide (what launch() enforces before it culls).  wave_object_mask tests the tile grown by 1.5 pixels on every side, proven to
// hold every PIXEL's plane point against float rounding of at most 7u aspect on the plane (its comment: 3u from the pixel's chain, 4u from
// the edge's, u = 2^-24).  At the lower edges a sample is no lower than its pixel, so the pixel's margin of 1.5 pixels stands.  At the upper
// edges the last pixel's samples reach at most one pixel further, leaving 0.5 aspect / W of the skirt against 7u aspect + 2^-5 aspect / W:
// enough while W < 0.468 / 7u = 1.12 million, and W <= 2^20.  Under a lens (wave_object_mask_lens) both the skirt and every error above are
// scaled by s alike, with one more relative rounding on each side (3.5u s aspect and 4.5u s aspect): 8u W < 0.468, W < 0.98 million — so the
// host culls a lens refine pass only up to 2^19 pixels a side (launch(): un-culled above that).  The same in v with aspect = 1.  Wherever
// the one-sample pass ran un-culled (variant 3, a lens beyond 90 degrees, the panorama, which has no tile mask, a frame outside the
// proven window) the host launches the un-culled form of this kernel; more than 64 objects are tested everywhere, as in trace().
template <class P>
RPT_DEV void refine_pixel_body(const RefineArgs &a) {
    __shared__ float4 handover[64];
    const int lane = threadIdx.x & 63;
    const int wave = (int)blockIdx.x & 3;              // one wave per workgroup, as the one-sample product kernels
    const int strip = (int)blockIdx.x >> 2;
    const int tile_x0 = strip * 32 + wave * 8, tile_y0 = (int)blockIdx.y * RPT_TILE_ROWS;
    const int x_coord = tile_x0 + (lane & 7), y_coord = tile_y0 + (lane >> 3);
    bool refine = false;
    if (x_coord < a.width && y_coord < a.height) {
        const uint32_t *p = a.aa_plane + (size_t)y_coord * a.width + x_coord;
        const uint32_t mine = *p;
        int d = 0;
        if (x_coord > 0) d = max_int(d, packed_rgb_distance(mine, p[-1]));
        if (x_coord + 1 < a.width) d = max_int(d, packed_rgb_distance(mine, p[1]));
        if (y_coord > 0) d = max_int(d, packed_rgb_distance(mine, p[-(ptrdiff_t)a.width]));
        if (y_coord + 1 < a.height) d = max_int(d, packed_rgb_distance(mine, p[a.width]));
        refine = d > a.aa_threshold;
    }
    const unsigned long long set = __ballot(refine);
    if (set == 0ull) return;                           // wave-uniform: most waves of a frame end here
    const int count = __popcll(set);
    if (lane == 0) atomicAdd(a.aa_refined, (unsigned long long)count);

    // all 64 lanes are here (the exit above is the wave's), so the mask's __ballot sees every lane's object
    unsigned long long object_mask = ~0ull;
    if constexpr (P::camera == Camera::lens) {
        if (P::culled && P::object_mask) object_mask = wave_object_mask_lens(a, a.lens_scale, tile_x0, tile_y0);
    } else if (P::culled && P::object_mask) object_mask = wave_object_mask(a, tile_x0, tile_y0);
    const bool masked = P::culled && P::object_mask;
    const bool any = !masked || object_mask != 0 || a.object_count > 64;

    const int n = a.aa_n, n2 = n * n;
    const int per_round = 64 / n2;                     // 16, 7, 4, 2, 1, 1, 1 pixels for n = 2 .. 8
    const int slot = lane / n2, sample = lane - slot * n2;
    const int sy = sample / n, sx = sample - sy * n;
    for (int first = 0; first < count; first += per_round) {
        const int rank = first + slot;
        const bool active = slot < per_round && rank < count;
        int px = 0, py = 0;
        f3 c = mk3(0.15f, 0.15f, 0.25f);               // a miss contributes the background of opencl_kernel.cl:565
        if (active) {
            const int owner = nth_set_bit(set, rank);
            px = tile_x0 + (owner & 7);
            py = tile_y0 + (owner >> 3);
            if (any || P::environment) {
                f3 camdir;
                if constexpr (P::camera == Camera::equirect) {
                    const float2 col = a.aa_cols[n * px + sx], row = a.aa_rows[n * py + sy];
                    camdir = normalize(mk3(row.y * col.x, row.x, row.y * col.y));          // equirectCamDir on the n-times tables
                } else {
                    const float xs = (float)px + (float)sx / (float)n, ys = (float)py + (float)sy / (float)n;
                    if constexpr (P::camera == Camera::lens) camdir = lensCamRayDir(xs, ys, a.width, a.height, a.aspect, a.lens_scale);
                    else camdir = createCamRayDir(xs, ys, a.width, a.height, a.aspect);
                }
                f3 traced;
                if (any && trace<P>(a, camdir, object_mask, traced)) c = traced;
                else if constexpr (P::environment) c = environment_colour(a, camdir);       // the sky of the sample's own direction
            }
        }
        handover[lane] = make_float4(c.x, c.y, c.z, 0.0f);
        __syncthreads();
        if (active && sample == 0) {
            f3 sum = mk3(0.0f, 0.0f, 0.0f);
            for (int k = 0; k < n2; k++) {
                const float4 h = handover[lane + k];
                sum = sum + mk3(h.x, h.y, h.z);
            }
            const float fn2 = (float)n2;
            sum = mk3(sum.x / fn2, sum.y / fn2, sum.z / fn2);
            f3 mapped;
            const uint32_t packed = tonemap_pack(a, sum, mapped);
            const size_t id = (size_t)py * a.width + px;
            if (a.out16) store_pixel(a.out16, id, __float_as_uint((float)px), __float_as_uint((float)py), packed, 0u);
            if (a.debug_rgb) {
                a.debug_rgb[3 * id + 0] = mapped.x;
                a.debug_rgb[3 * id + 1] = mapped.y;
                a.debug_rgb[3 * id + 2] = mapped.z;
            }
        }
        __syncthreads();                               // the next round's writes wait for this round's reads
    }
}

// Refine kernels: the throughput forms only, as the event pass — the walk with the wave's object mask and the exact reciprocal (10x1), its
// IEEE form for scenes outside the domain, no walk compiled in (10x4), un-culled (10x3) — for each camera and colour family.  The tens
// digit: 0 pinhole, 1 its Doppler twin, 2 its environment form; 3 / 4 / 5 the same under a lens; 6 / 7 / 8 in panorama.  The number is
// what rpt_last_aa_variant reports.
#define RPT_REFINE_FAMILY(name, WRAP_OPEN, WRAP_CLOSE, UNCULLED, WALK, WALK_IEEE, ANALYTIC)                                                                                       \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_refine_kernel_##name##_unculled(const RefineArgs a) { refine_pixel_body<WRAP_OPEN UNCULLED WRAP_CLOSE >(a); }   \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_refine_kernel_##name##_walk(const RefineArgs a) { refine_pixel_body<WRAP_OPEN WALK WRAP_CLOSE >(a); }           \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(5, 5))) void rpt_refine_kernel_##name##_walk_ieee(const RefineArgs a) { refine_pixel_body<WRAP_OPEN WALK_IEEE WRAP_CLOSE >(a); } \
    __global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(8, 8))) void rpt_refine_kernel_##name##_analytic(const RefineArgs a) { refine_pixel_body<WRAP_OPEN ANALYTIC WRAP_CLOSE >(a); }
RPT_REFINE_FAMILY(plain, , , Unculled, BallotExact, Ballot, Analytic)                                                       // 1003, 1001, (1001), 1004
RPT_REFINE_FAMILY(doppler, DopplerTwin<, >, Unculled, BallotExact, Ballot, Analytic)                                        // 1013, 1011, (1011), 1014
RPT_REFINE_FAMILY(env, Environment<, >, Unculled, BallotExact, Ballot, Analytic)                                            // 1023, 1021, (1021), 1024
RPT_REFINE_FAMILY(lens, Lens<, >, Unculled, BallotExact, Ballot, Analytic)                                                  // 1033, 1031, (1031), 1034
RPT_REFINE_FAMILY(lens_doppler, Lens<DopplerTwin<, > >, Unculled, BallotExact, Ballot, Analytic)                             // 1043, 1041, (1041), 1044
RPT_REFINE_FAMILY(lens_env, Lens<Environment<, > >, Unculled, BallotExact, Ballot, Analytic)                                 // 1053, 1051, (1051), 1054
RPT_REFINE_FAMILY(pano, , , PanoramaUnculled, PanoramaWalk, PanoramaWalkIeee, PanoramaAnalytic)                             // 1063, 1061, (1061), 1064
RPT_REFINE_FAMILY(pano_doppler, DopplerTwin<, >, PanoramaUnculled, PanoramaWalk, PanoramaWalkIeee, PanoramaAnalytic)        // 1073, 1071, (1071), 1074
RPT_REFINE_FAMILY(pano_env, Environment<, >, PanoramaUnculled, PanoramaWalk, PanoramaWalkIeee, PanoramaAnalytic)            // 1083, 1081, (1081), 1084
#undef RPT_REFINE_FAMILY

// ---- Overlay pass (rpt_set_overlay / rpt_render_overlay; not in the reference; DESIGN.md "Overlay pass") ---------------------------------
// Lines drawn on the rendered frame from the event records: a bandwidth-bound stencil that reads the records and the framebuffer's packed
// colour and nothing else, so it serves every camera and colour mode and no render kernel knows of it.  The rules are in include/rpt.h.
#define RPT_OVERLAY_TILE_W 64
#define RPT_OVERLAY_TILE_H 8
#define RPT_OVERLAY_PITCH (RPT_OVERLAY_TILE_W + 1)                          /* a tile row and its right halo pixel */
#define RPT_OVERLAY_SLOTS ((RPT_OVERLAY_TILE_H + 1) * RPT_OVERLAY_PITCH)   /* ... and the halo row above the tile */
#define RPT_OVERLAY_OUTSIDE (-2147483647 - 1)    /* `object` of a pixel outside the frame; as a cell: "never on a line" */
// bits of OverlayArgs::layers above the five of include/rpt.h: the lattice axes with a non-zero step
#define RPT_OVERLAY_AXIS_SHIFT 8

struct OverlayArgs {
    const rpt_event *events;        // [height][width] records of the same view
    rpt_pixel *out16;               // the framebuffer: only the dword at byte 8 of a pixel is read and written
    unsigned long long *changed;    // the context's counter of pixels whose RGBA changed: one atomic add per workgroup that changed any
    const uint32_t *tmax_bits;      // tint_t_max == 0: the bit pattern of the frame's largest delay (overlay_tmax_kernel); else null
    int width, height;
    uint32_t layers;                // RPT_OVERLAY_* | the lattice axes in use << RPT_OVERLAY_AXIS_SHIFT
    float interval;                 // (float)interval
    float delay_inv, clock_inv, lattice_inv[3];     // 1.0f / step, formed on the host
    float tint_t_max;
    uint32_t outline_rgba, delay_rgba, clock_rgba, lattice_rgba;    // R | G << 8 | B << 16 | A << 24
    uint32_t tint_alpha;
};

// floorf(s * inv) as an integer, or RPT_OVERLAY_OUTSIDE where the product is not finite or is 2^30 or more in magnitude
RPT_DEV int overlay_cell(float s, float inv) {
    const float p = s * inv;
    if (!(fabsf(p) < 1073741824.0f)) return RPT_OVERLAY_OUTSIDE;       // (a NaN fails the comparison too)
    return (int)floorf(p);
}

// out = (c * a + old * (255 - a) + 127) / 255 on R, G and B; the alpha byte of `old` stays
RPT_DEV uint32_t overlay_blend(uint32_t old, uint32_t rgb, uint32_t alpha) {
    uint32_t out = old & 0xff000000u;
    for (int k = 0; k < 3; k++) {
        const uint32_t c = (rgb >> (8 * k)) & 255u, o = (old >> (8 * k)) & 255u;
        out |= ((c * alpha + o * (255u - alpha) + 127u) / 255u) << (8 * k);
    }
    return out;
}

// |interval * dist|, 0 where that is not finite: the delay of the tint and of its maximum
RPT_DEV float overlay_delay(float interval, float dist) {
    const float d = fabsf(interval * dist);
    return d <= 3.402823466e38f ? d : 0.0f;
}

// What the rules need of pixel (x, y), put into LDS slot `slot` of the planes that are in use: its object and the cell of every contour
// layer that is on.  Outside the frame: RPT_OVERLAY_OUTSIDE as the object (no rule looks further).  Returns the record's first 16 bytes.
RPT_DEV uint4 overlay_reduce_record(const OverlayArgs &a, int x, int y, int slot, int *objects, int (*cells)[RPT_OVERLAY_SLOTS]) {
    uint4 lo = make_uint4(0u, 0u, 0u, 0u);
    if (x >= a.width || y >= a.height) {
        objects[slot] = RPT_OVERLAY_OUTSIDE;
        return lo;
    }
    const uint4 *record = reinterpret_cast<const uint4 *>(a.events + ((size_t)y * a.width + x));
    lo = record[0];                                                    // object, dist, event[0], event[1]
    objects[slot] = (int)lo.x;
    if (a.layers & RPT_OVERLAY_ISO_DELAY) cells[0][slot] = overlay_cell(fabsf(a.interval * __uint_as_float(lo.y)), a.delay_inv);
    if (a.layers & RPT_OVERLAY_ISO_CLOCK) cells[1][slot] = overlay_cell(__uint_as_float(lo.z), a.clock_inv);
    if (a.layers & (1u << RPT_OVERLAY_AXIS_SHIFT)) cells[2][slot] = overlay_cell(__uint_as_float(lo.w), a.lattice_inv[0]);
    if (a.layers & (6u << RPT_OVERLAY_AXIS_SHIFT)) {                   // the second 16 bytes only where a y or z lattice needs them
        const uint4 hi = record[1];                                    // event[2], event[3], u, v
        if (a.layers & (2u << RPT_OVERLAY_AXIS_SHIFT)) cells[3][slot] = overlay_cell(__uint_as_float(hi.x), a.lattice_inv[1]);
        if (a.layers & (4u << RPT_OVERLAY_AXIS_SHIFT)) cells[4][slot] = overlay_cell(__uint_as_float(hi.y), a.lattice_inv[2]);
    }
    return lo;
}

// whether the pixel in `slot` is on a line of the contour plane `cell`: a neighbour (right: slot + 1, upper: slot + pitch) of the same
// object — a pixel outside the frame has none — whose cell differs, both cells being valid
RPT_DEV bool overlay_on_contour(const int *objects, const int *cell, int slot, int object) {
    const int mine = cell[slot];
    if (mine == RPT_OVERLAY_OUTSIDE) return false;
    bool on = false;
    for (int k = 0; k < 2; k++) {
        const int q = slot + (k ? RPT_OVERLAY_PITCH : 1);
        const int theirs = cell[q];
        on = on || (objects[q] == object && theirs != RPT_OVERLAY_OUTSIDE && theirs != mine);
    }
    return on;
}

// 1100: a workgroup of 512 lanes owns a 64 x 8 pixel tile, wave w its row w (a wave's two record loads cover 2 KB of consecutive bytes).
// Every lane reduces its own record into LDS; the first 64 lanes also reduce the row above the tile, the next 8 the column to its right
// (72 halo records per 512, most of them still in L2 from the neighbouring workgroup).  After one barrier each lane reads its right and
// upper neighbour from LDS and blends into its own pixel's RGBA dword: neighbours' colours are never read, so the update in place has no
// ordering hazard.  LDS: 6 planes of 9 x 65 ints, 14040 B.  Changed pixels: a ballot per wave, the eight waves' counts added in LDS, one
// global atomic per workgroup — one per wave, 130 000 on one address at 4K, was measured to cost more than the rest of the kernel.
__global__ __launch_bounds__(512) void rpt_overlay_kernel(const OverlayArgs a) {
    __shared__ int objects[RPT_OVERLAY_SLOTS];
    __shared__ int cells[5][RPT_OVERLAY_SLOTS];
    __shared__ unsigned int tile_changed;
    const int t = (int)threadIdx.x;
    if (t == 0) tile_changed = 0u;
    const int lx = t & (RPT_OVERLAY_TILE_W - 1), ly = t >> 6;
    const int x0 = (int)blockIdx.x * RPT_OVERLAY_TILE_W, y0 = (int)blockIdx.y * RPT_OVERLAY_TILE_H;
    const int x = x0 + lx, y = y0 + ly;
    const int slot = ly * RPT_OVERLAY_PITCH + lx;
    const uint4 lo = overlay_reduce_record(a, x, y, slot, objects, cells);
    if (t < RPT_OVERLAY_TILE_W) (void)overlay_reduce_record(a, x0 + t, y0 + RPT_OVERLAY_TILE_H, RPT_OVERLAY_TILE_H * RPT_OVERLAY_PITCH + t, objects, cells);
    else if (t < RPT_OVERLAY_TILE_W + RPT_OVERLAY_TILE_H)
        (void)overlay_reduce_record(a, x0 + RPT_OVERLAY_TILE_W, y0 + t - RPT_OVERLAY_TILE_W, (t - RPT_OVERLAY_TILE_W) * RPT_OVERLAY_PITCH + RPT_OVERLAY_TILE_W, objects, cells);
    __syncthreads();

    bool changed = false;
    if (x < a.width && y < a.height) {
        const int object = (int)lo.x;
        const bool hit = object >= 0;
        uint32_t *rgba = reinterpret_cast<uint32_t *>(a.out16 + ((size_t)y * a.width + x)) + 2;
        const uint32_t before = *rgba;
        uint32_t now = before;
        if ((a.layers & RPT_OVERLAY_DELAY_TINT) && hit) {
            const float t_max = a.tmax_bits ? __uint_as_float(*a.tmax_bits) : a.tint_t_max;
            const float d = overlay_delay(a.interval, __uint_as_float(lo.y));
            float xr = 0.0f;
            if (t_max > 0.0f) xr = fminf(fmaxf(d / t_max, 0.0f), 1.0f);
            const float x2 = 2.0f * xr;
            const float r = fminf(fmaxf(1.0f - x2, 0.0f), 1.0f);
            const float g = 1.0f - fabsf(x2 - 1.0f);
            const float b = fminf(fmaxf(x2 - 1.0f, 0.0f), 1.0f);
            const uint32_t rb = (uint32_t)rintf((0.25f + 0.75f * r) * 255.0f);
            const uint32_t gb = (uint32_t)rintf((0.25f + 0.75f * g) * 255.0f);
            const uint32_t bb = (uint32_t)rintf((0.25f + 0.75f * b) * 255.0f);
            now = overlay_blend(now, rb | (gb << 8) | (bb << 16), a.tint_alpha);
        }
        if (hit) {
            if (a.layers & RPT_OVERLAY_LATTICE) {
                bool on = false;
                for (int k = 0; k < 3; k++)
                    if (a.layers & ((1u << k) << RPT_OVERLAY_AXIS_SHIFT)) on = on || overlay_on_contour(objects, cells[2 + k], slot, object);
                if (on) now = overlay_blend(now, a.lattice_rgba, a.lattice_rgba >> 24);
            }
            if ((a.layers & RPT_OVERLAY_ISO_CLOCK) && overlay_on_contour(objects, cells[1], slot, object)) now = overlay_blend(now, a.clock_rgba, a.clock_rgba >> 24);
            if ((a.layers & RPT_OVERLAY_ISO_DELAY) && overlay_on_contour(objects, cells[0], slot, object)) now = overlay_blend(now, a.delay_rgba, a.delay_rgba >> 24);
        }
        if (a.layers & RPT_OVERLAY_OUTLINES) {
            const int right = objects[slot + 1], upper = objects[slot + RPT_OVERLAY_PITCH];
            if ((right != RPT_OVERLAY_OUTSIDE && right != object) || (upper != RPT_OVERLAY_OUTSIDE && upper != object))
                now = overlay_blend(now, a.outline_rgba, a.outline_rgba >> 24);
        }
        changed = now != before;
        if (changed) *rgba = now;
    }
    const unsigned long long set = __ballot(changed);
    if ((t & 63) == 0 && set) atomicAdd(&tile_changed, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && tile_changed) atomicAdd(a.changed, (unsigned long long)tile_changed);
}

// 1101: the frame's largest delay over hit pixels, for tint_t_max == 0.  A grid-stride loop over the records' first 8 bytes, the wave's
// maximum by six butterfly shuffles, then one atomic max per wave on the bit pattern — the delays are non-negative floats,
// whose order is that of their bit patterns as unsigned integers.  *out is zeroed by the host before the launch.
__global__ __launch_bounds__(256) void rpt_overlay_tmax_kernel(const rpt_event *events, size_t pixels, float interval, uint32_t *out) {
    float mine = 0.0f;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < pixels; i += (size_t)gridDim.x * 256) {
        const uint2 head = *reinterpret_cast<const uint2 *>(events + i);      // object, dist
        if ((int)head.x >= 0) mine = fmaxf(mine, overlay_delay(interval, __uint_as_float(head.y)));
    }
    for (int offset = 32; offset >= 1; offset >>= 1) mine = fmaxf(mine, __shfl_xor(mine, offset, 64));
    if ((threadIdx.x & 63) == 0 && mine > 0.0f) atomicMax(out, __float_as_uint(mine));
}

// ---- Readout pass (rpt_set_readouts / rpt_render_readouts; not in the reference; DESIGN.md "Readout pass") -------------------------------
// Seven-segment displays on the objects' surfaces that show the hit object's own time, offset + rate * event[0], per pixel.  A sibling
// of the overlay pass: the same tile, halo and counter, its own kernel; it reads the records and the framebuffer's packed colour and
// nothing else.  The rules are in include/rpt.h.
struct alignas(16) ReadoutDisplay {     // one per entry of Object[], derived from rpt_readout on the host (48 B: three 16-byte loads)
    float rate, offset, scale;          // scale = (float)10^decimals
    uint32_t digits;                    // digits | decimals << 8; digits == 0: no display
    float u0, v0, inv_w, inv_h;         // inv_w = 1.0f / (u1 - u0), inv_h = 1.0f / (v1 - v0)
    uint32_t on_rgba, off_rgba;         // R | G << 8 | B << 16 | A << 24
    uint32_t pad[2];
};
static_assert(sizeof(ReadoutDisplay) == 48, "ReadoutDisplay");

struct ReadoutArgs {
    const rpt_event *events;            // [height][width] records of the same view
    rpt_pixel *out16;                   // the framebuffer: only the dword at byte 8 of a pixel is read and written
    unsigned long long *changed;        // the context's counter of pixels whose RGBA changed: one atomic add per workgroup that changed any
    const ReadoutDisplay *displays;     // [count]
    unsigned long long low_mask;        // bit o: object o < 64 has a display (the others: displays[o].digits)
    int width, height;
    int count;                          // the Object[]'s
};

// whether object `o` of a record has a display: the kernel arguments answer for the first 64 objects, the table for the others
RPT_DEV bool readout_has_display(const ReadoutArgs &a, int o) {
    if (o < 0 || o >= a.count) return false;
    if (o < 64) return ((a.low_mask >> o) & 1ull) != 0ull;
    return (a.displays[o].digits & 255u) != 0u;
}

// What the rules need of pixel (x, y), put into LDS slot `slot`: its object, and (u, v) where that object has a display.  Outside the
// frame: RPT_OVERLAY_OUTSIDE as the object.  Returns the record's first 16 bytes; *shown = the pixel is in the frame and has a display.
RPT_DEV uint4 readout_stage_record(const ReadoutArgs &a, int x, int y, int slot, int *objects, float *us, float *vs, bool *shown) {
    uint4 lo = make_uint4(0u, 0u, 0u, 0u);
    *shown = false;
    if (x >= a.width || y >= a.height) {
        objects[slot] = RPT_OVERLAY_OUTSIDE;
        return lo;
    }
    const uint4 *record = reinterpret_cast<const uint4 *>(a.events + ((size_t)y * a.width + x));
    lo = record[0];                                                    // object, dist, event[0], event[1]
    objects[slot] = (int)lo.x;
    if (readout_has_display(a, (int)lo.x)) {
        const uint4 hi = record[1];                                    // event[2], event[3], u, v
        us[slot] = __uint_as_float(hi.z);
        vs[slot] = __uint_as_float(hi.w);
        *shown = true;
    }
    return lo;
}

// the seven-segment mask of a decimal digit, a = bit 0 .. g = bit 6: 0x3f 0x06 0x5b 0x4f 0x66 0x6d 0x7d 0x07 | 0x7f 0x6f
RPT_DEV uint32_t readout_digit_mask(uint32_t d) {
    return (uint32_t)((d < 8u ? 0x077d6d664f5b063full >> (8u * d) : 0x6f7full >> (8u * (d - 8u))) & 0x7full);
}

// the segments and the decimal point (bit 7) whose box holds (lx, t) of a character cell; the bounds are sixteenths, exact in float
RPT_DEV uint32_t readout_segments_at(float lx, float t) {
    const bool wide = lx >= 0.1875f && lx < 0.6875f, left = lx >= 0.125f && lx < 0.25f, right = lx >= 0.625f && lx < 0.75f;
    const bool lower = t >= 0.125f && t < 0.5f, upper = t >= 0.5f && t < 0.875f, foot = t >= 0.0625f && t < 0.1875f;
    uint32_t m = 0u;
    if (wide && t >= 0.8125f && t < 0.9375f) m |= 1u;         // a
    if (right && upper) m |= 2u;                              // b
    if (right && lower) m |= 4u;                              // c
    if (wide && foot) m |= 8u;                                // d
    if (left && lower) m |= 16u;                              // e
    if (left && upper) m |= 32u;                              // f
    if (wide && t >= 0.4375f && t < 0.5625f) m |= 64u;        // g
    if (lx >= 0.8125f && lx < 0.9375f && foot) m |= 128u;     // the decimal point
    return m;
}

// 1110: the overlay kernel's shape — a workgroup of 512 lanes owns a 64 x 8 pixel tile, wave w its row w; every lane stages its own
// record into LDS (object; u and v where the object has a display), the first 64 lanes also the row above the tile, the next 8 the
// column to its right; one barrier; then a lane whose object has a display forms its footprint from the right and the upper neighbour in
// LDS, tests its 16 sub-samples and blends into its own pixel's RGBA dword.  The work hangs on the lane's own "has a display": a wave
// without such a lane (most of them) has every lane off in that branch, so it has read 16 B per pixel and leaves — no sub-sample work, no
// framebuffer byte read or written — and still reaches both barriers.  LDS: 3 planes of 9 x 65 words and the counter, 7044 B as laid out.
// Changed pixels are counted as 1100 counts them.
__global__ __launch_bounds__(512) void rpt_readout_kernel(const ReadoutArgs a) {
    __shared__ int objects[RPT_OVERLAY_SLOTS];
    __shared__ float us[RPT_OVERLAY_SLOTS], vs[RPT_OVERLAY_SLOTS];
    __shared__ unsigned int tile_changed;
    const int t = (int)threadIdx.x;
    if (t == 0) tile_changed = 0u;
    const int lx = t & (RPT_OVERLAY_TILE_W - 1), ly = t >> 6;
    const int x0 = (int)blockIdx.x * RPT_OVERLAY_TILE_W, y0 = (int)blockIdx.y * RPT_OVERLAY_TILE_H;
    const int x = x0 + lx, y = y0 + ly;
    const int slot = ly * RPT_OVERLAY_PITCH + lx;
    bool shown, halo_shown;
    const uint4 lo = readout_stage_record(a, x, y, slot, objects, us, vs, &shown);
    if (t < RPT_OVERLAY_TILE_W) (void)readout_stage_record(a, x0 + t, y0 + RPT_OVERLAY_TILE_H, RPT_OVERLAY_TILE_H * RPT_OVERLAY_PITCH + t, objects, us, vs, &halo_shown);
    else if (t < RPT_OVERLAY_TILE_W + RPT_OVERLAY_TILE_H)
        (void)readout_stage_record(a, x0 + RPT_OVERLAY_TILE_W, y0 + t - RPT_OVERLAY_TILE_W, (t - RPT_OVERLAY_TILE_W) * RPT_OVERLAY_PITCH + RPT_OVERLAY_TILE_W, objects, us, vs, &halo_shown);
    __syncthreads();

    bool changed = false;
    if (shown) {      // (a wave none of whose lanes is shown has all lanes off here: it skips the body and goes on to the barrier below)
        const int object = (int)lo.x;
        const ReadoutDisplay d = a.displays[object];
        const int digits = (int)(d.digits & 255u), decimals = (int)(d.digits >> 8);
        // the value, and the nine cells' segment masks packed 7 bits a cell (cell k at bit 7 k)
        const float sv = (d.rate * __uint_as_float(lo.z) + d.offset) * d.scale;
        const bool neg = sv < 0.0f;
        bool over = !(fabsf(sv) < 1e9f);                               // (a NaN overflows too)
        uint32_t mag = over ? 0u : (uint32_t)(int)floorf(fabsf(sv));   // below 10^9
        uint32_t limit = 1u;
        for (int k = 0; k < digits - (neg ? 1 : 0); k++) limit *= 10u;
        over = over || mag >= limit;
        unsigned long long cells = 0ull;
        for (int k = digits - 1; k >= 0; k--) {
            cells |= (unsigned long long)readout_digit_mask(mag % 10u) << (7 * k);
            mag /= 10u;
        }
        if (neg) cells = (cells & ~0x7full) | 0x40ull;
        if (over) cells = 0x4081020408102040ull;                       // segment g alone in every cell: 0x40 << 7 k, k = 0..8
        const int point_cell = (decimals > 0 && !over) ? digits - 1 - decimals : -1;
        // the footprint: differences to the right and the upper neighbour where it is of the same object, else 0
        const float u = us[slot], v = vs[slot];
        float du_x = 0.0f, dv_x = 0.0f, du_y = 0.0f, dv_y = 0.0f;
        if (objects[slot + 1] == object) {
            du_x = us[slot + 1] - u;
            dv_x = vs[slot + 1] - v;
        }
        if (objects[slot + RPT_OVERLAY_PITCH] == object) {
            du_y = us[slot + RPT_OVERLAY_PITCH] - u;
            dv_y = vs[slot + RPT_OVERLAY_PITCH] - v;
        }
        const float fdigits = (float)digits;
        uint32_t n_in = 0u, n_on = 0u;
        for (int i = 0; i < 4; i++) {
            const float ai = -0.375f + 0.25f * (float)i;               // -0.375, -0.125, 0.125, 0.375: exact
            const float ui = u + ai * du_x, vi = v + ai * dv_x;
            for (int j = 0; j < 4; j++) {
                const float aj = -0.375f + 0.25f * (float)j;
                const float s = ((ui + aj * du_y) - d.u0) * d.inv_w;
                const float tt = ((vi + aj * dv_y) - d.v0) * d.inv_h;
                if (s >= 0.0f && s < 1.0f && tt >= 0.0f && tt < 1.0f) {
                    const float cs = s * fdigits;
                    int c = (int)floorf(cs);
                    c = c < digits - 1 ? c : digits - 1;
                    const uint32_t lit = ((uint32_t)(cells >> (7 * c)) & 0x7fu) | (c == point_cell ? 0x80u : 0u);
                    n_in++;
                    if (lit & readout_segments_at(cs - (float)c, tt)) n_on++;
                }
            }
        }
        uint32_t *rgba = reinterpret_cast<uint32_t *>(a.out16 + ((size_t)y * a.width + x)) + 2;
        const uint32_t before = *rgba;
        uint32_t now = overlay_blend(before, d.off_rgba, ((d.off_rgba >> 24) * n_in + 8u) / 16u);
        now = overlay_blend(now, d.on_rgba, ((d.on_rgba >> 24) * n_on + 8u) / 16u);
        changed = now != before;
        if (changed) *rgba = now;
    }
    const unsigned long long set = __ballot(changed);
    if ((t & 63) == 0 && set) atomicAdd(&tile_changed, (unsigned int)__popcll(set));
    __syncthreads();
    if (t == 0 && tile_changed) atomicAdd(a.changed, (unsigned long long)tile_changed);
}

#ifdef RPT_DIAGNOSTICS
}  // namespace rptd
#include "rpt_diag_kernels.hip.h"    /* librpt_hip_diag.so only: instrumented kernels, round 1's prepass, the A/B arms of rounds 2 and 3 */
namespace rptd {
#endif

// Root-side reassembly after the gather: plane of rank r, local tile k -> global tile r + k*n_ranks.
__global__ __launch_bounds__(256) void rpt_scatter_plane_kernel(const uint32_t *planes, rpt_pixel *out16, int width,
                                                               int height, int n_ranks, size_t plane_stride_words) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= width || y >= height) return;
    const int tile = y / RPT_TILE_ROWS;
    const int rank = tile % n_ranks;
    const int local_row = (tile / n_ranks) * RPT_TILE_ROWS + (y % RPT_TILE_ROWS);
    const uint32_t packed = planes[(size_t)rank * plane_stride_words + (size_t)local_row * width + x];
    uint4 px;
    px.x = __float_as_uint((float)x);
    px.y = __float_as_uint((float)y);
    px.z = packed;
    px.w = 0u;
    store_pixel(out16, (size_t)y * width + x, px.x, px.y, px.z, px.w);
}

// The exchange carries 3 bytes per pixel: the fourth byte of every packed colour is the constant 1
// (opencl_kernel.cl:657).  Four pixels (four words) of a colour plane become three words, R0 G0 B0 R1 | G1 B1 R2 G2 |
// B2 R3 G3 B3; a plane's pixel count is a multiple of 8 (whole 8-row tiles).
__global__ __launch_bounds__(256) void rpt_pack_plane3_kernel(const uint4 *plane4, uint32_t *plane3, size_t quads) {
    const size_t q = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (q >= quads) return;
    const uint4 p = plane4[q];
    plane3[3 * q + 0] = (p.x & 0xffffffu) | (p.y << 24);
    plane3[3 * q + 1] = ((p.y >> 8) & 0xffffu) | (p.z << 16);
    plane3[3 * q + 2] = ((p.z >> 16) & 0xffu) | (p.w << 8);
}

// Root-side reassembly of gathered 3-byte planes (rpt_scatter_plane_kernel for the packed form).
__global__ __launch_bounds__(256) void rpt_scatter_plane3_kernel(const uint8_t *planes, rpt_pixel *out16, int width, int height,
                                                                int n_ranks, size_t plane_stride_bytes) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= width || y >= height) return;
    const int tile = y / RPT_TILE_ROWS;
    const int rank = tile % n_ranks;
    const int local_row = (tile / n_ranks) * RPT_TILE_ROWS + (y % RPT_TILE_ROWS);
    const uint8_t *src = planes + (size_t)rank * plane_stride_bytes + 3 * ((size_t)local_row * width + x);
    uint4 px;
    px.x = __float_as_uint((float)x);
    px.y = __float_as_uint((float)y);
    px.z = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | (1u << 24);
    px.w = 0u;
    store_pixel(out16, (size_t)y * width + x, px.x, px.y, px.z, px.w);
}

// Reassembly for the weighted split (rpt_set_tile_pattern): per period of `period` tiles the root renders the first
// `root_run` straight into the framebuffer, helper j (1..n_ranks-1) the tile root_run + j - 1 into its 3-byte plane
// (local tile = period index).  Only the helpers' tiles are written here; the root's are already in place.
__global__ __launch_bounds__(256) void rpt_scatter_helper_planes3_kernel(const uint8_t *planes, rpt_pixel *out16, int width, int height,
                                                                        int period, int root_run, size_t plane_stride_bytes) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    const int y = blockIdx.y;
    if (x >= width || y >= height) return;
    const int tile = y / RPT_TILE_ROWS;
    const int slot = tile % period;
    if (slot < root_run) return;
    const int rank = slot - root_run + 1;
    const int local_row = (tile / period) * RPT_TILE_ROWS + (y % RPT_TILE_ROWS);
    const uint8_t *src = planes + (size_t)rank * plane_stride_bytes + 3 * ((size_t)local_row * width + x);
    uint4 px;
    px.x = __float_as_uint((float)x);
    px.y = __float_as_uint((float)y);
    px.z = (uint32_t)src[0] | ((uint32_t)src[1] << 8) | ((uint32_t)src[2] << 16) | (1u << 24);
    px.w = 0u;
    store_pixel(out16, (size_t)y * width + x, px.x, px.y, px.z, px.w);
}

// rpt_verify_frame: how many packed colours differ between two colour planes (one ballot + popcount per wave-iteration)
// rpt_probe_tile_masks: one wave per 8x8 tile of the whole frame forms the object mask as kernel 41 (under a lens: 841) does — the
// ballot over the regions, then thin_object_mask with the same policy — and writes it before and after the tile bitmaps.
__global__ __launch_bounds__(64) void rpt_probe_tile_masks_kernel(const LensArgs a, int lens, unsigned long long *out) {
    const int x0 = (int)blockIdx.x * 8, y0 = (int)blockIdx.y * RPT_TILE_ROWS;
    const unsigned long long before = lens ? wave_object_mask_lens(a, a.lens_scale, x0, y0) : wave_object_mask(a, x0, y0);
    const unsigned long long after = lens ? thin_object_mask<Lens<BallotExact>>(a, before, x0, y0) : thin_object_mask<BallotExact>(a, before, x0, y0);
    if (threadIdx.x == 0) {
        const size_t t = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        out[2 * t] = before;
        out[2 * t + 1] = after;
    }
}

__global__ __launch_bounds__(256) void rpt_count_differences_kernel(const uint32_t *p, const uint32_t *q, size_t words, unsigned long long *out) {
    unsigned long long mine = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < words; i += (size_t)gridDim.x * 256) mine += __popcll(__ballot(p[i] != q[i]));
    if ((threadIdx.x & 63) == 0 && mine) atomicAdd(out, mine);     // (every lane of a wave holds the wave's count: lane 0 reports it)
}

// Known-answer probes of single device functions.
__global__ void rpt_probe_kernel(int which, const float *in, float *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (which == 0) {
        const float *p = in + 15 * i;
        Ray r;
        r.origin = mk3(p[9], p[10], p[11]);
        r.dir = mk3(p[12], p[13], p[14]);
        float dist = 0;
        f2 uv = {0, 0};
        const bool h = intersect_triangle(mk3(p[0], p[1], p[2]), mk3(p[3], p[4], p[5]), mk3(p[6], p[7], p[8]), r, dist, uv);
        out[4 * i + 0] = h ? 1.0f : 0.0f;
        out[4 * i + 1] = h ? dist : 0;
        out[4 * i + 2] = h ? uv.x : 0;
        out[4 * i + 3] = h ? uv.y : 0;
    } else if (which == 1) {
        const float *p = in + 12 * i;
        Ray r;
        r.origin = mk3(p[6], p[7], p[8]);
        r.dir = mk3(p[9], p[10], p[11]);
        f2 d = {0, 0};
        int cs = 0, fs = 0;
        const bool h = intersect_AABB(mk3(p[0], p[1], p[2]), mk3(p[3], p[4], p[5]), r, d, cs, fs);
        out[5 * i + 0] = h ? 1.0f : 0.0f;
        out[5 * i + 1] = h ? d.x : 0;
        out[5 * i + 2] = h ? d.y : 0;
        out[5 * i + 3] = h ? (float)cs : 0;
        out[5 * i + 4] = h ? (float)fs : 0;
    } else if (which == 2) {
        const float *p = in + 4 * i;
        const int w = (int)p[2], hgt = (int)p[3];
        const f3 dir = createCamRayDir(p[0], p[1], w, hgt, (float)w / (float)hgt);
        out[3 * i + 0] = dir.x;
        out[3 * i + 1] = dir.y;
        out[3 * i + 2] = dir.z;
    } else if (which == 3) {
        out[3 * i + 0] = hable1(in[3 * i + 0]);
        out[3 * i + 1] = hable1(in[3 * i + 1]);
        out[3 * i + 2] = hable1(in[3 * i + 2]);
    } else if (which == 4) {    // asin(a), atan2(b, c) of the textured-sphere (u,v)
        out[2 * i + 0] = rpt_asinf(in[3 * i + 0]);
        out[2 * i + 1] = rpt_atan2f(in[3 * i + 1], in[3 * i + 2]);
    } else {    // the walk's two pure steps: exit face of a leaf, child selection (general and fast form)
        const float *p = in + 6 * i;
        f3 uv = mk3(p[3], p[4], p[5]);
        const int side = getOppositeBoxSide(makeExitPlan(mk3(p[0], p[1], p[2])), uv);
        out[12 * i + 0] = (float)side; out[12 * i + 1] = uv.x; out[12 * i + 2] = uv.y; out[12 * i + 3] = uv.z;
        f3 a = mk3(p[3], p[4], p[5]), b = a;
        const int ca = octree_child_step(a), cb = octree_child_step_fast(b);
        out[12 * i + 4] = (float)ca; out[12 * i + 5] = a.x; out[12 * i + 6] = a.y; out[12 * i + 7] = a.z;
        out[12 * i + 8] = (float)cb; out[12 * i + 9] = b.x; out[12 * i + 10] = b.y; out[12 * i + 11] = b.z;
    }
}

// rpt_probe which = 6: S_f of the Doppler kernels on n inputs {D, r, g, b, flags} -> 3 floats (a kernel of its own: rpt_probe_kernel stays as it was)
__global__ __launch_bounds__(256) void rpt_probe_doppler_kernel(const float *in, float *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const float *p = in + 5 * i;
    const f3 o = doppler_colour((int)p[4], p[0], mk3(p[1], p[2], p[3]));
    out[3 * i + 0] = o.x;
    out[3 * i + 1] = o.y;
    out[3 * i + 2] = o.z;
}

// rpt_probe which = 7: the sky lookup alone on n directions {d.x, d.y, d.z} of the sky's rest frame (normalised here, as the render path
// normalises E's output) -> {u, v, r, g, b}
__global__ __launch_bounds__(256) void rpt_probe_environment_kernel(const uint32_t *texels, int width, int height, const float *in, float *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const f2 uv = environment_uv(normalize(mk3(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2])));
    const f3 c = environment_bilinear(texels, width, height, uv);
    float *o = out + 5 * (size_t)i;
    o[0] = uv.x; o[1] = uv.y; o[2] = c.x; o[3] = c.y; o[4] = c.z;
}

// The exact reciprocal against IEEE 1 / s (rpt_probe_reciprocal): every float s whose bit pattern lies in [lo_bits, lo_bits + per_sign),
// with both signs.  counts = {values compared, mismatches of rcp_newton<1>, <2>, <3> (rpt_device_math.hip.h), samples written}; the
// first max_samples mismatching s go to samples as {s, bit mask of the forms that missed (1, 2, 4)}.
__global__ __launch_bounds__(256) void rpt_probe_reciprocal_kernel(uint32_t lo_bits, unsigned long long per_sign, unsigned long long *counts, float *samples, int max_samples) {
    unsigned long long n_cmp = 0, bad1 = 0, bad2 = 0, bad3 = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long i = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; i < 2ull * per_sign; i += stride) {
        const uint32_t sign = i < per_sign ? 0u : 0x80000000u;
        const float s = __uint_as_float(sign | (lo_bits + (uint32_t)(i < per_sign ? i : i - per_sign)));
        const uint32_t ref = __float_as_uint(1.0f / s);
        const int miss = (__float_as_uint(rcp_newton<1>(s)) != ref ? 1 : 0) | (__float_as_uint(rcp_newton<2>(s)) != ref ? 2 : 0) |
                         (__float_as_uint(rcp_newton<3>(s)) != ref ? 4 : 0);
        n_cmp++;
        bad1 += miss & 1;
        bad2 += (miss >> 1) & 1;
        bad3 += (miss >> 2) & 1;
        if (miss && samples) {
            const unsigned long long slot = atomicAdd(&counts[4], 1ull);
            if (slot < (unsigned long long)max_samples) { samples[2 * slot] = s; samples[2 * slot + 1] = (float)miss; }
        }
    }
    atomicAdd(&counts[0], n_cmp); atomicAdd(&counts[1], bad1); atomicAdd(&counts[2], bad2); atomicAdd(&counts[3], bad3);
}

// Known-answer probes at OBJECT level (rpt_probe_object; the oracle's counterpart is rpt_oracle_object_rays): which =
//   0: one 4-D ray {origin4, dir4} in the rest frame of object `object` through intersect_object, the general form every shadow ray
//      and the RefLayout kernel's primary rays take: out 8 = {hit, dist, normal.xyz, uv.xy, 0}   (opencl_kernel.cl:312-359, 200-308)
//   1: sample_light on a shadow ray {origin4, dir4, lightDist} of the camera frame with light `object`: out 2 = {occluded as the
//      un-culled kernel decides it, occluded as the culled kernels decide it (segment culls, __ballot over the wave)}   (:488-545)
//   2: the transforms on {x, y, z, w}: out 16 = transformPoint(InvM), transformPoint4D(Lorentz), transformDirection(InvM),
//      applyTranspose(InvM) of object `object`   (:75-104)
//   3: a primary ray with camera direction {x, y, z} (normalised here as trace() does) through intersect_object_primary, the form
//      the default kernels use (origin and constants from the per-frame DObj record): out 8 as in 0
__global__ __launch_bounds__(64) void rpt_probe_object_kernel(const KernelArgs a, int which, int object, const float *in, float *out, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int j = i < n ? i : n - 1;          // (idle lanes repeat the last ray: the culled forms ballot over whole waves)
    if (which == 0 || which == 3) {
        Hit hit;
        hit.dist = 1e20f;
        hit.normal = mk3(0.0f, 0.0f, 0.0f);
        hit.uv.x = hit.uv.y = 0.0f;
        hit.object = -1;
        bool h;
        if (which == 0) {
            const float *p = in + 8 * (size_t)j;
            h = intersect_object<Unculled>(a, object, mk4(p[0], p[1], p[2], p[3]), mk4(p[4], p[5], p[6], p[7]), hit);
        } else {
            const float *p = in + 3 * (size_t)j;
            const f3 nd = normalize(mk3(p[0], p[1], p[2]));
            h = intersect_object_primary<Ballot>(a, object, mk4((float)a.interval, nd.x, nd.y, nd.z), hit);
        }
        if (i < n) {
            float *o = out + 8 * (size_t)i;
            o[0] = h ? 1.0f : 0.0f;
            o[1] = h ? hit.dist : 0.0f;
            o[2] = h ? hit.normal.x : 0.0f; o[3] = h ? hit.normal.y : 0.0f; o[4] = h ? hit.normal.z : 0.0f;
            o[5] = h ? hit.uv.x : 0.0f; o[6] = h ? hit.uv.y : 0.0f;
            o[7] = 0.0f;
        }
    } else if (which == 1) {
        const float *p = in + 9 * (size_t)j;
        const f4 o4 = mk4(p[0], p[1], p[2], p[3]), d4 = mk4(p[4], p[5], p[6], p[7]);
        const bool plain = sample_light_occluded<Unculled>(a, o4, d4, p[8], object);
        const bool culled = sample_light_occluded<Ballot>(a, o4, d4, p[8], object);
        if (i < n) { out[2 * (size_t)i] = plain ? 1.0f : 0.0f; out[2 * (size_t)i + 1] = culled ? 1.0f : 0.0f; }
    } else if (i < n) {
        const float *p = in + 4 * (size_t)i;
        float *o = out + 16 * (size_t)i;
        const rpt_object &obj = a.objects[object];
        const f3 v = mk3(p[0], p[1], p[2]);
        const f3 t0 = transformPoint(obj.InvM, v);
        const f4 t1 = transformPoint4D(obj.Lorentz, mk4(p[0], p[1], p[2], p[3]));
        const f3 t2 = transformDirection(obj.InvM, v);
        const f3 t3 = applyTranspose(obj.InvM, v);
        o[0] = t0.x; o[1] = t0.y; o[2] = t0.z; o[3] = 0.0f;
        o[4] = t1.x; o[5] = t1.y; o[6] = t1.z; o[7] = t1.w;
        o[8] = t2.x; o[9] = t2.y; o[10] = t2.z; o[11] = 0.0f;
        o[12] = t3.x; o[13] = t3.y; o[14] = t3.z; o[15] = 0.0f;
    }
}

// Known-answer probe of the octree walk at RAY level: every ray (object-space origin and direction) through the three walks the
// product library holds — the reference's layouts (octree_core_ref), the throughput walk (octree_walk<false, ...>) and the latency
// walk (octree_walk<true, ...>) — with the hit re-measured from the origin (0, 0, 0) at unit direction length.  8 floats per walk
// and ray: hit flag, dist, normal.xyz, uv.xy, 0.
// exact = 1: the two derived-layout walks in the EXACT_RCP form kernels 41 / 43 launch on this scene (its triangles are in the domain)
__global__ __launch_bounds__(256) void rpt_probe_walk_kernel(const KernelArgs a, int object, const float *rays, float *out, int n, int exact) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.origin = mk3(rays[6 * i + 0], rays[6 * i + 1], rays[6 * i + 2]);
    r.dir = mk3(rays[6 * i + 3], rays[6 * i + 4], rays[6 * i + 5]);
    const rpt_object &obj = a.objects[object];
    const int root = a.dobjs[object].root;
    for (int w = 0; w < 3; w++) {
        Hit hit;
        hit.dist = 1e20f;
        hit.normal = mk3(0.0f, 0.0f, 0.0f);
        hit.uv.x = hit.uv.y = 0.0f;
        hit.object = -1;
        const f3 o0 = mk3(0.0f, 0.0f, 0.0f);
        const bool h = w == 0 ? octree_core_ref(a, obj, r, o0, 1.0f, hit)
                     : w == 1 ? (exact ? octree_walk<false, true>(a, obj, root, r, o0, 1.0f, hit)
                                       : octree_walk<false, false>(a, obj, root, r, o0, 1.0f, hit))
                              : (exact ? octree_walk<true, true>(a, obj, root, r, o0, 1.0f, hit)
                                       : octree_walk<true, false>(a, obj, root, r, o0, 1.0f, hit));
        float *o = out + ((size_t)i * 3 + w) * 8;
        o[0] = h ? 1.0f : 0.0f;
        o[1] = h ? hit.dist : 0.0f;
        o[2] = h ? hit.normal.x : 0.0f;
        o[3] = h ? hit.normal.y : 0.0f;
        o[4] = h ? hit.normal.z : 0.0f;
        o[5] = h ? hit.uv.x : 0.0f;
        o[6] = h ? hit.uv.y : 0.0f;
        o[7] = 0.0f;
    }
}

#endif  /* !RPT_RELAXED_FP */

}  // namespace rptd
