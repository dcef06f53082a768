// rpt_api.hip — C-ABI of librpt_hip.so (include/rpt.h): context, scene upload with validation,
// per-frame Object[] refresh, launch and read-back.  Host glue only; the device code is in
// rpt_kernels.hip.h.  Replaces the reference's CLSetup.cpp / main.cpp:33-59 enqueue sequence.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <chrono>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "../../include/rpt.h"
#include "rpt_kernels.hip.h"       /* (+ rpt_diag_walks / rpt_diag_kernels / rpt_persistent under RPT_DIAGNOSTICS) */
#include "rpt_octree_build.hip.h"
#include "rpt_screen_bounds.hpp"
#include "rpt_bounds_certify.hpp"
#include "rpt_tile_bitmap.hpp"
#include "rpt_sky_split.hpp"
#include "rpt_workers.hpp"
#include "rpt_stars.hip.h"          /* the splat passes, behind the render kernels; each header includes the ones it builds on */
#include "rpt_stars_host.hpp"
#include "rpt_particles.hip.h"      /* splat_taps and point_splat: the segments, the ballistic pass and the rockets use them */
#include "rpt_particles_host.hpp"
#include "rpt_thermal.hip.h"        /* T_f, the thermal probe and kernels 1122 and 1132 */
#include "rpt_thermal_host.hpp"
#include "rpt_segments.hip.h"
#include "rpt_segments_host.hpp"
#include "rpt_dust.hip.h"
#include "rpt_dust_host.hpp"
#include "rpt_ballistics.hip.h"
#include "rpt_ballistics_host.hpp"
#include "rpt_rockets.hip.h"
#include "rpt_rockets_host.hpp"
#include "rpt_glare.hip.h"          /* the opt-in glare stage between a splat pass's splat and its resolve: kernels 1170 and 1171 */

#pragma clang fp contract(off)

// rpt_relaxed.hip: the opt-in build of the same kernels with OpenCL's default arithmetic (variants 50 / 51)
extern "C" int rpt_launch_relaxed_kernel(int waves_per_simd, const void *args, size_t args_bytes, unsigned grid_x, unsigned grid_y, void *stream);

#define RPT_STAGING_SLOTS 4
#ifdef RPT_DIAGNOSTICS      /* RPT_HOST_PROFILE=1: where the host time of rpt_set_objects goes, summed per context and printed by rpt_destroy */
#include <chrono>
#define RPT_HOST_MARK(K) do { const auto now_ = std::chrono::steady_clock::now(); if (K) ctx->host_us[K] += std::chrono::duration<double, std::micro>(now_ - ctx->host_t).count(); ctx->host_t = now_; if ((K) == 5) ctx->host_calls++; } while (0)
#else
#define RPT_HOST_MARK(K) do { } while (0)
#endif
#define RPT_RECT_BATCH_MIN 3      /* screen bounds to recompute in one rpt_set_objects before the helper threads are asked (rpt_workers.hpp); 8 until the bounds were proven as well (round 4: twice the work per object) */

namespace {

struct DeviceBuffer {
    void *ptr = nullptr;
    size_t bytes = 0;      // bytes in use
    size_t capacity = 0;
};

void release(DeviceBuffer &b);

// A device buffer that is (re)written from the host in stream order: staged_host() hands out pinned memory that is safe to rewrite,
// staged_copy() enqueues the copy and records `copied`.  A frame still in flight reads what it was launched with, a later one the new bytes.
struct StagedUpload {
    DeviceBuffer device;
    void *host = nullptr;                             // pinned: what the last upload was copied from
    size_t host_capacity = 0;
    hipEvent_t copied = nullptr;                      // recorded after that copy: `host` is rewritten only once it has passed
};

// The way back: a pass's counters, one or two 64-bit words, left on the device and read later without blocking the caller.
// tally_ready() on first use, tally_zero() on the stream before the pass, tally_home() behind it (the copy, `copied`, pending);
// tally_collect() takes the pinned words over once `copied` has passed, tally_off() is a pass switched off: nothing pending, all zero.
struct Tally {
    DeviceBuffer device;                              // the words of the pass in flight, then `spare` bytes of the pass's own that are zeroed with them
    unsigned long long *host = nullptr;               // pinned: the words of the last pass whose copy has run
    hipEvent_t copied = nullptr;                      // recorded after that copy
    unsigned long long value[4] = {0, 0, 0, 0};       // what rpt_last_* reports: `host` as last read with `copied` passed (the particle pass has four words)
    size_t words = 1, spare = 0;                      // (as tally_ready was given them)
    bool pending = false;                             // a copy has been enqueued since `value` was read
};
enum { TALLY_AA, TALLY_OVERLAY, TALLY_READOUTS, TALLY_STARS, TALLY_PARTICLES, TALLY_SEGMENTS, TALLY_BALLISTICS, TALLY_ROCKETS, TALLY_COUNT };     // rpt_ctx::tally

// A splat pass (the stars, the particles, the segments, the ballistic particles, the rockets): its records on the device, the temperatures beside them, and the marks of a
// timed pass, and the two options every pass but the stars has.  What one pass alone has (the segments' pieces, the particles' lighting) stays with the context.
struct SplatPass {
    int count = 0;                                    // 0 = no catalogue, no set: the pass is off
    int flags = 0;                                    // rpt_set_particle_options, _ballistic_, _rocket_, _segment_: the inverse square (the same bit in all four)
    float depth_bias = 0.0f;
    int largest_object = -1;                          // the largest Object[] index the set names, held against object_count at every launch; -1 for the stars, who name none
    StagedUpload table;                               // rpt_star / rpt_particle / rpt_segment / rpt_ballistic / rpt_rocket per record, in the caller's order; written once per rpt_set_*
    // rpt_set_star_temperatures / rpt_set_particle_temperatures: x_G per source, parallel to the records; 0 entries =
    // none set, and the pass launches kernel 1120 / 1130 as before.  The segments have none
    int thermal_count = 0;
    StagedUpload thermal_table;                       // one float per source, written once per rpt_set_*_temperatures
    bool timed = false;                               // rpt_set_*_measurement
    hipEvent_t marks[3] = {nullptr, nullptr, nullptr};    // timed passes: before the splat, between the kernels, after the resolve
    bool marked = false;                              // the last pass recorded them
};
enum { SPLAT_STARS, SPLAT_PARTICLES, SPLAT_SEGMENTS, SPLAT_BALLISTICS, SPLAT_ROCKETS, SPLAT_COUNT };     // rpt_ctx::splat

// What the last frame of one kind (colour, event) was enqueued for, as a pass over both asks (frames_of_this_view)
struct FrameMark {
    unsigned long long generation = 0;                // rpt_ctx::view_generation then; 0 = no such frame yet
    int width = 0, height = 0;
    void *buffer = nullptr;                           // the framebuffer (null: a colour plane) / the records it was rendered into
    bool rendered() const { return generation != 0; }
};

// The equirectangular camera's tables (rpt_projection_tables) on the device, and what they were built for (n = 0: nothing yet)
struct ProjectionTables {
    StagedUpload upload;                              // [n (width + height)] float2: the column table, then the row table
    int n = 0, width = 0, height = 0;
    float params[3] = {0, 0, 0};
};

// The resident scene geometry: immutable between two rpt_upload_scene calls, so contexts that keep several frames
// in flight share ONE copy (rpt_share_scene); the last context holding it frees it.
struct Geometry {
    int device = 0;
    DeviceBuffer vertices, normals, uvs, triangles, octrees, octreeTris, textures;
    DeviceBuffer dnodes, dtris, dlinks;       // derived layouts (rpt_kernels.hip.h)
    DeviceBuffer dfirst;                      // first triangle record of every node's list, by node index (the latency walk)
    DeviceBuffer dexits, dhits;               // exit records by (node, side), hit records by triangle id (rpt_kernels.hip.h: DExit, DHit)
    bool compact_ok = false;                  // derived octree layout usable (children consecutive)
    bool exact_rcp_ok = false;                // every triangle a walk tests lies in the exact reciprocal's domain (rpt_scene_exact_rcp)
    unsigned long long generation = 0;        // unique per upload (the rectangle cache of a context names its geometry by this, not by address)
    std::vector<int> node_new_index;          // reference node index -> index in the derived, breadth-first numbering
    int top_count = 0;                        // derived nodes [0, top_count) are the forest's top levels (<= RPT_TOP_MAX)
    std::vector<float> host_node_bounds;      // min.xyz,max.xyz per octree node (culling spheres of mesh roots)
    std::vector<float> node_tri_K, node_tri_L;       // per node: the largest |e1| |e2| and the longest edge of the triangles its list names (mesh_segment_apart's margin)
    std::vector<uint8_t> node_holds_its_triangles;   // per node: every triangle of its list lies inside its box (true of a mesh's root
                                                     // unless its list also holds an earlier mesh's triangles, Mesh.cpp:16-19)
    std::map<int, std::vector<float>> mesh_boxes;    // per mesh root (reference node index): the sub-tree boxes of rpt_tile_bitmap.hpp, six floats each
    std::map<int, std::vector<float>> mesh_tri_boxes;    // ... and its triangle boxes, one per distinct listed triangle (none: over the cap, or the stage is not for this mesh)
    // Tile bitmaps built against this geometry, for the contexts that share it (rpt_share_scene: four frames in flight ask for the same
    // bitmap one after the other).  The key is what rpt_tile_bitmap.hpp says a bitmap is a function of, next to the boxes above: the
    // object's bytes, the interval, the frame's size, the lens scale and the diagonals flag — and which stages the asking context runs.
    // One mutex; one entry per object slot a context can have a bitmap for (64: contexts ask for their still meshes in the same order, so
    // fewer entries than still meshes would evict what the next context is about to ask for), the oldest replaced, 16 KB each at 4K; the
    // build happens UNDER the lock, so a second context asking for the same key waits and then copies.  A new upload is a new Geometry: the
    // cache goes with its generation.  bitmap_builds / bitmap_copies count the misses and the hits (rpt_tile_bitmap_shared_state).
    struct BitmapEntry {
        uint8_t object[sizeof(rpt_object)];
        int interval, width, height;
        float lens;
        bool diagonals, triangles, built;             // built: false = this key gets no bitmap (remembered too)
        std::vector<uint32_t> bits;
    };
    static constexpr size_t BITMAP_CACHE_ENTRIES = 64;
    std::mutex bitmap_cache_lock;
    std::vector<BitmapEntry> bitmap_cache;
    size_t bitmap_cache_next = 0;                     // the slot the next new key replaces once all are taken
    unsigned long long bitmap_builds = 0, bitmap_copies = 0;
    size_t vertex_count = 0, normal_count = 0, uv_count = 0, triangle_words = 0, octree_count = 0, octree_tri_count = 0;
    ~Geometry() {
        bool any = false;
        for (const DeviceBuffer *b : {&vertices, &normals, &uvs, &triangles, &octrees, &octreeTris, &textures, &dnodes, &dtris, &dlinks, &dfirst, &dexits, &dhits}) any = any || b->ptr;
        if (!any) return;                        // (a host-only copy, rpt_tile_bitmap_host: nothing of the device's to free)
        (void)hipSetDevice(device);
        for (DeviceBuffer *b : {&vertices, &normals, &uvs, &triangles, &octrees, &octreeTris, &textures, &dnodes, &dtris, &dlinks, &dfirst, &dexits, &dhits}) release(*b);
    }
};

}  // namespace

struct rpt_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    hipEvent_t ev_begin = nullptr, ev_end = nullptr;
    hipEvent_t last_event = nullptr;                  // the event recorded last on `stream` (a launch's end or a staging copy's)
    std::string error;

    DeviceBuffer objects;
    std::shared_ptr<Geometry> geo;                    // never null
    DeviceBuffer counters, wave_times;
    DeviceBuffer tile_masks;                          // per-tile object masks of the prepass
    DeviceBuffer verify_planes;                       // rpt_verify_frame: two scratch colour planes + the difference count
    DeviceBuffer claim_counters;                      // persistent kernels: two sets of per-queue claim counters (rpt_persistent.hip.h)
    int cu_count = 0;
    unsigned int claim_epoch = 0;
    std::vector<uint8_t> host_objects;                // last Object[] (DObj depends on `interval`: rebuilt when it changes)
    DeviceBuffer dobjs;
    std::vector<rptb::Rect> rects;                    // last frame's per-object rectangles (reused for unchanged objects)
    int rect_interval = 0x7fffffff;
    unsigned long long rect_geo_generation = ~0ull;   // Geometry::generation the cached rectangles were computed against
    DeviceBuffer owned_out, owned_plane, owned_rgb;
    void *pinned_objects = nullptr;                   // RPT_STAGING_SLOTS pinned slots of Object[] + DObj[]
    size_t pinned_capacity = 0;
    hipEvent_t staging_done[4] = {nullptr, nullptr, nullptr, nullptr};
    unsigned int staging_used = 0, staging_next = 0;
    int object_count = 0;
    bool scene_uploaded = false;

    float white_point[3] = {1, 1, 1};
    float ambient = 1.0f;
    int width = 0, height = 0, interval = -1;
    bool params_set = false;

    void *external_out = nullptr;
    void *external_plane = nullptr;
    void *external_rgb = nullptr;
    std::vector<hipEvent_t> timing_events;   // pairs: begin,end per frame
    int timing_frames = -1;                  // -1 = timing region not active
    bool want_owned_rgb = false;
    int first_tile = 0, tile_step = 1, run_log2 = 0;
    bool colour_plane = false;
    int variant = 0;
    int last_variant = 0;                             // the kernel the last launch was made with (rpt_last_variant)
    bool last_sky_split = false;                      // ... as a sky split (launch(); rpt_last_sky_split), with this box of 8x8 tiles: x0, y0, x1, y1
    int last_sky_box[4] = {0, 0, 0, 0};
    // rpt_set_object_windows (not in the reference): {t0, t1} per object, per context, never shared; empty = none (today's kernels)
    std::vector<float> windows;
    bool last_exact_rcp = false;                      // ... and whether its walk took 1 / det through rcp_exact (rpt_last_exact_rcp)
    int msaa = 1;                                     // MSAASAMPLES (rpt_set_msaa)
    int serial = 0;                                   // creation index of this context in the process (diagnostics output)
#ifdef RPT_DIAGNOSTICS
    std::chrono::steady_clock::time_point host_t;     // RPT_HOST_MARK
    double host_us[6] = {0, 0, 0, 0, 0, 0};
    long host_calls = 0;
#endif
    float last_ms = 0.0f;
    bool has_mesh = true;                             // the current Object[] holds a mesh object (rpt_set_objects); picks the kernel
    // rpt_set_doppler (not in the reference): RPT_DOPPLER_SHIFT | RPT_DOPPLER_BEAMING, 0 = off; per context, never shared
    int doppler = 0;
    void *external_doppler = nullptr;                 // rpt_set_debug_doppler: the record's buffer (or the library's, want_owned_doppler)
    bool want_owned_doppler = false;
    bool doppler_recorded = false;                    // the last launch was the Doppler debug kernel (the record is the last frame's)
    DeviceBuffer owned_doppler;
    // rpt_set_projection (not in the reference): RPT_PROJECTION_*, per context, never shared
    int projection = RPT_PROJECTION_PINHOLE;
    float projection_params[3] = {0, 0, 0};           // {h_fov, v_fov, yaw} of the equirectangular camera
    ProjectionTables pano;                            // the frame's tables
    // rpt_set_raymap (not in the reference): the ray-map camera's directions, per context, never shared
    bool raymap_on = false;
    int raymap_width = 0, raymap_height = 0, raymap_pitch = 0;
    StagedUpload raymap;                              // [raymap_pitch * raymap_height] float4 {p.x, p.y, p.z, 0}, pitch = width rounded up to 8
    // rpt_set_environment / rpt_set_environment_frame (not in the reference): the sky image, per context, never shared
    bool env_on = false;
    int env_width = 0, env_height = 0;
    float env_frame[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};     // E, row-major, t first; a kernel ARGUMENT (a frame in flight keeps its own)
    StagedUpload env;                                 // [env_width * env_height] dwords R | G << 8 | B << 16
    // rpt_set_orientation / rpt_set_field_of_view (not in the reference): the free-look camera, per context, never shared
    bool oriented = false;                            // R != I: host_objects (and the device's Object[]) are the RE-BASED objects
    double R[3][3] = {{1, 0, 0}, {0, 1, 0}, {0, 0, 1}};
    std::vector<uint8_t> caller_objects;              // while oriented: the caller's last Object[] as it was given (else host_objects is that)
    std::vector<uint8_t> given_scratch, turned_scratch;   // rpt_set_objects with an orientation: reused from frame to frame (no allocation per call)
    float v_fov = 0.0f;                               // 0 = the reference's lens
    float lens_scale = 1.0f;                          // (float)tan(v_fov / 2)
    // rpt_set_events_output / rpt_render_events (not in the reference): the event pass, per context, never shared
    void *external_events = nullptr;                  // the caller's record buffer (width * height * 32 B), or null: owned_events
    DeviceBuffer owned_events;                        // allocated on first use
    hipEvent_t ev_events = nullptr;                   // recorded after every event pass (what last_event names then); created on first use
    int last_events_variant = 0;                      // the event kernel the last pass ran with (rpt_last_events_variant)
    bool last_events_exact_rcp = false;               // ... and whether its walk took 1 / det through rcp_exact (rpt_last_events_exact_rcp)
    FrameMark event_frame;                            // the last event frame, as rpt_pick and rpt_read_events address it
    int events_first_tile = 0, events_tile_step = 1, events_run_log2 = 0;     // ... and the rows of it this context wrote
    // rpt_set_adaptive_aa (not in the reference): adaptive anti-aliasing, per context, never shared
    int aa_n = 1, aa_threshold = 8;                   // samples per axis (1 = off) and the criterion's threshold
    DeviceBuffer aa_plane;                            // pass A's packed colours, 4 B/pixel: what pass B decides from
    int last_aa_variant = 0;                          // the refine kernel of the last colour frame (rpt_last_aa_variant)
    ProjectionTables aa_pano;                         // panorama: the tables at aa_n times the frame's size, for the refine pass
    // rpt_set_overlay / rpt_render_overlay (not in the reference): the overlay pass, per context, never shared
    rpt_overlay_desc overlay = {};                    // layers == 0: off
    unsigned long long view_generation = 1;           // bumped by every call that changes the view (objects, params, projection, orientation, lens)
    FrameMark colour_frame;                           // the last colour frame (rendered() is what the read-back calls ask)
    // what the passes report, by TALLY_*: the refined pixels of an adaptive frame (rpt_last_aa_refined); the overlay's changed pixels and,
    // as spare bytes, the bit pattern of the frame's largest delay (rpt_last_overlay_pixels); the readouts' changed pixels
    // (rpt_last_readout_pixels); {stars with a tap inside the frame, changed pixels} (rpt_last_stars); {particles seen, changed pixels}
    // (rpt_last_particles); {pieces drawn, changed pixels} (rpt_last_segments); {records seen, changed pixels} (rpt_last_ballistics, rpt_last_rockets)
    Tally tally[TALLY_COUNT];
    // rpt_set_readouts / rpt_render_readouts (not in the reference): the readout pass, per context, never shared
    std::vector<rpt_readout> readouts;                // one per entry of Object[]; empty = none set
    unsigned long long readout_low_mask = 0;          // bit o: object o < 64 has a display
    StagedUpload readout_table;                       // rptd::ReadoutDisplay per object, written once per rpt_set_readouts
    // rpt_set_stars, rpt_set_particles, rpt_set_segments and their rpt_render_* (not in the reference): the splat
    // passes, by SPLAT_*, per context, never shared.  All three sum through splat_acc: it is all zero outside any pass, and the passes of
    // one context are ordered by its stream
    SplatPass splat[SPLAT_COUNT];
    DeviceBuffer splat_acc;                           // 24 B per pixel of the largest frame so far: the fixed-point sums, all zero outside a pass
    // rpt_set_glare (not in the reference): the integers of rules G0 and G1 as kernels 1170 and 1171 take them, and the
    // planes of h_k beside splat_acc, reserved at the first glared pass.  Per context, never shared
    int glare_layers = 0;                             // 0: off, and a splat pass launches its own resolve kernel
    unsigned int glare_weight[1 + RPT_GLARE_LAYERS_MAX] = {65536u, 0u, 0u, 0u};
    int glare_radius[RPT_GLARE_LAYERS_MAX] = {0, 0, 0};
    unsigned int glare_taps[RPT_GLARE_LAYERS_MAX][RPT_GLARE_RADIUS_MAX + 1] = {};
    DeviceBuffer glare_planes;                        // layers x 24 B per pixel of the largest glared frame so far; 1170 writes every word 1171 reads
    int particle_lighting = 0;                        // rpt_set_particle_lighting: RPT_PARTICLES_LIT | _SHADOWED | _AMBIENT
    int segment_pieces = rptg::kDefaultPieces;        // rpt_set_segment_options
    // the tile bitmaps of the still meshes (rpt_tile_bitmap.hpp): slot i = object i, bitmap_words() dwords each; per context, never shared
    StagedUpload tile_bits;
    unsigned long long bits_still = 0;                // objects whose record was byte-identical in the last two rpt_set_objects calls
    unsigned long long bits_tried = 0;                // ... of which a build has been attempted for the key below
    unsigned long long bits_has = 0;                  // ... of which a bitmap is on the device (behind everything enqueued so far)
    int bits_width = 0, bits_height = 0, bits_slots = 0;      // the key: what the bitmaps on the device were built for
    float bits_lens = 0.0f;
    bool bits_diagonals = false;
    unsigned long long bits_builds = 0;               // bitmaps that went live in this context so far (rpt_tile_bitmap_state), built here or copied from the scene's cache
    double bits_last_build_us = 0.0;                  // host time this context spent on the last of them
    bool tile_triangles = true;                       // RPT_TILE_TRIANGLES=0 at rpt_create: the sub-tree stage alone
    int sky_split_share = 50;                         // the sky split's largest box, in percent of the frame's tiles (RPT_SKY_SPLIT_SHARE at rpt_create; 0: never split)
    long long sky_split_min_pixels = 6000000;      // ... and frames of more pixels than this are split (RPT_SKY_SPLIT_MIN_PIXELS at rpt_create)
};

namespace {

int fail(rpt_ctx *ctx, int code, const std::string &msg) {
    if (ctx) ctx->error = msg;
    return code;
}

#define RPT_HIP(ctx, call)                                                                           \
    do {                                                                                             \
        hipError_t e_ = (call);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(ctx, RPT_ERR_DEVICE, std::string(#call) + ": " + hipGetErrorString(e_));     \
    } while (0)

int reserve(rpt_ctx *ctx, DeviceBuffer &b, size_t bytes) {
    if (bytes > b.capacity || !b.ptr) {      // (!ptr: an empty array still gets a valid, never dereferenced, pointer)
        if (b.ptr) RPT_HIP(ctx, hipFree(b.ptr));
        b.ptr = nullptr;
        b.capacity = 0;
        // at least 16 B so that an empty array still has a valid (never dereferenced) pointer
        const size_t cap = bytes < 16 ? 16 : bytes;
        RPT_HIP(ctx, hipMalloc(&b.ptr, cap));
        b.capacity = cap;
    }
    b.bytes = bytes;
    return RPT_OK;
}

int upload(rpt_ctx *ctx, DeviceBuffer &b, const void *src, size_t bytes) {
    if (int rc = reserve(ctx, b, bytes)) return rc;
    if (bytes) RPT_HIP(ctx, hipMemcpy(b.ptr, src, bytes, hipMemcpyHostToDevice));
    return RPT_OK;
}

void release(DeviceBuffer &b) {
    if (b.ptr) (void)hipFree(b.ptr);
    b = DeviceBuffer();
}

// `bytes` of u's pinned memory that may be rewritten now, and a device buffer that holds as many: waits for the previous copy, and for
// the stream before a device buffer that a frame in flight may still read is replaced by a larger one.
int staged_host(rpt_ctx *ctx, StagedUpload &u, size_t bytes, void **host) {
    if (!u.copied) RPT_HIP(ctx, hipEventCreateWithFlags(&u.copied, hipEventDisableTiming));
    else RPT_HIP(ctx, hipEventSynchronize(u.copied));
    if (bytes > u.host_capacity) {
        if (u.host) RPT_HIP(ctx, hipHostFree(u.host));
        u.host = nullptr;
        u.host_capacity = 0;
        RPT_HIP(ctx, hipHostMalloc(&u.host, bytes, hipHostMallocDefault));
        u.host_capacity = bytes;
    }
    if (bytes > u.device.capacity) RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));     // (the old buffer may still be read)
    if (int rc = reserve(ctx, u.device, bytes)) return rc;
    *host = u.host;
    return RPT_OK;
}

// ... and its way to the device, behind everything enqueued so far
int staged_copy(rpt_ctx *ctx, StagedUpload &u) {
    RPT_HIP(ctx, hipMemcpyAsync(u.device.ptr, u.host, u.device.bytes, hipMemcpyHostToDevice, ctx->stream));
    RPT_HIP(ctx, hipEventRecord(u.copied, ctx->stream));
    return RPT_OK;
}

void release(StagedUpload &u) {
    release(u.device);
    if (u.host) (void)hipHostFree(u.host);
    if (u.copied) (void)hipEventDestroy(u.copied);
    u = StagedUpload();
}

// First use: `words` 64-bit words on the device with `spare` bytes behind them, as many pinned words, and the event
int tally_ready(rpt_ctx *ctx, Tally &t, size_t words, size_t spare = 0) {
    t.words = words;
    t.spare = spare;
    if (int rc = reserve(ctx, t.device, words * 8 + spare)) return rc;
    if (!t.host) RPT_HIP(ctx, hipHostMalloc((void **)&t.host, words * 8, hipHostMallocDefault));
    if (!t.copied) RPT_HIP(ctx, hipEventCreateWithFlags(&t.copied, hipEventDisableTiming));
    return RPT_OK;
}

// ... all zero on the stream before the pass, the spare bytes too
int tally_zero(rpt_ctx *ctx, Tally &t) {
    RPT_HIP(ctx, hipMemsetAsync(t.device.ptr, 0, t.words * 8 + t.spare, ctx->stream));
    return RPT_OK;
}

// ... and the words' way home behind the pass, in stream order
int tally_home(rpt_ctx *ctx, Tally &t) {
    RPT_HIP(ctx, hipMemcpyAsync(t.host, t.device.ptr, t.words * 8, hipMemcpyDeviceToHost, ctx->stream));
    RPT_HIP(ctx, hipEventRecord(t.copied, ctx->stream));
    t.pending = true;
    return RPT_OK;
}

void tally_collect(Tally &t) {
    if (t.pending && t.copied && hipEventQuery(t.copied) == hipSuccess) {
        for (size_t k = 0; k < t.words; k++) t.value[k] = t.host[k];
        t.pending = false;
    }
}

void tally_off(Tally &t) {
    t.pending = false;
    for (unsigned long long &v : t.value) v = 0;
}

// A rpt_last_* call: the first `words` words as last collected, after one more look where a copy is still on its way
int tally_read(rpt_ctx *ctx, int which, unsigned long long *out, int words) {
    if (!ctx || !out) return RPT_ERR_ARG;
    Tally &t = ctx->tally[which];
    if (t.pending) {
        RPT_HIP(ctx, hipSetDevice(ctx->device));
        tally_collect(t);
    }
    for (int k = 0; k < words; k++) out[k] = t.value[k];
    return RPT_OK;
}

void release(Tally &t) {
    release(t.device);
    if (t.host) (void)hipHostFree(t.host);
    if (t.copied) (void)hipEventDestroy(t.copied);
    t = Tally();
}

// opencl_kernel.cl:607-616 on the host (same fp32 expression; this file is built without contraction)
float hable_host(float x) {
    const float A = 0.15f, B = 0.50f, C = 0.10f, D = 0.20f, E = 0.02f, F = 0.30f;
    return ((x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F)) - E / F;
}

uint32_t to_u8_host(float c) {   // same definition as the kernel's to_u8
    const float t = c * 255;
    if (!(t == t)) return 0u;
    if (t <= 0.0f) return 0u;
    if (t >= 255.0f) return 255u;
    return (uint32_t)(int)t;
}

// Every index the kernel will follow must stay inside its array: a GPU fault can reset the node.
int validate_geometry(rpt_ctx *ctx, const rpt_scene_desc &s) {
    if (s.triangle_words % RPT_TRI_STRIDE) return fail(ctx, RPT_ERR_SCENE, "triangles: word count is not a multiple of 9");
    const size_t n_tris = s.triangle_words / RPT_TRI_STRIDE;
    for (size_t t = 0; t < n_tris; t++)
        for (int k = 0; k < 3; k++) {
            const uint32_t *w = s.triangles + 9 * t + 3 * k;
            if (w[0] >= s.vertex_count) return fail(ctx, RPT_ERR_SCENE, "triangles: vertex index out of range");
            if (w[1] >= s.uv_count) return fail(ctx, RPT_ERR_SCENE, "triangles: uv index out of range (pad uvs to >= 1 entry for vt-less meshes)");
            if (w[2] >= s.normal_count) return fail(ctx, RPT_ERR_SCENE, "triangles: normal index out of range");
        }
    for (size_t i = 0; i < s.octree_tri_count; i++)
        if (s.octreeTris[i] < 0 || (size_t)s.octreeTris[i] >= n_tris) return fail(ctx, RPT_ERR_SCENE, "octreeTris: triangle index out of range");
    const long long n_nodes = (long long)s.octree_count;
    for (size_t i = 0; i < s.octree_count; i++) {
        const rpt_octree &n = s.octrees[i];
        if (n.trisCount < 0 || n.trisIndex < 0 || (size_t)n.trisIndex + (size_t)n.trisCount > s.octree_tri_count)
            return fail(ctx, RPT_ERR_SCENE, "octree: triangle range out of bounds");
        for (int c = 0; c < 8; c++) {
            if (n.children[c] < -1 || n.children[c] >= n_nodes) return fail(ctx, RPT_ERR_SCENE, "octree: child index out of range");
            if (n.children[0] != -1 && n.children[c] == -1) return fail(ctx, RPT_ERR_SCENE, "octree: interior node with a missing child");
        }
        for (int c = 0; c < 6; c++)
            if (n.neighbors[c] < -1 || n.neighbors[c] >= n_nodes) return fail(ctx, RPT_ERR_SCENE, "octree: neighbour index out of range");
    }
    // the child links must form a forest (no cycles), or the descent loops would not terminate
    std::vector<uint8_t> state(s.octree_count, 0);   // 0 unvisited, 1 on the DFS stack, 2 done
    std::vector<std::pair<int, int>> stack;
    for (size_t r = 0; r < s.octree_count; r++) {
        if (state[r]) continue;
        stack.push_back({(int)r, 0});
        state[r] = 1;
        while (!stack.empty()) {
            auto &top = stack.back();
            const rpt_octree &n = s.octrees[top.first];
            if (n.children[0] == -1 || top.second == 8) {
                state[top.first] = 2;
                stack.pop_back();
                continue;
            }
            const int c = n.children[top.second++];
            if (state[c] == 1) return fail(ctx, RPT_ERR_SCENE, "octree: child links form a cycle");
            if (state[c] == 0) {
                state[c] = 1;
                stack.push_back({c, 0});
            }
        }
    }
    return RPT_OK;
}

// Derived octree layout: one 64-B DNode per node and one 48-B DTri per leaf triangle reference.
// Only the numbers the reference stores (and B-A, C-A, which intersect_triangle would form from
// them with the same IEEE subtraction) go in, so traversal results are unchanged.
// Nodes are renumbered breadth first over the whole forest — every root, then every node of level 1, and so on — so that
// (a) the eight children of a node stay consecutive (they are one block in the reference's numbering too, Octree.cpp:191-269)
// and (b) the top levels of every octree are the first `top_count` records: the persistent kernels keep those nodes' links
// in LDS.  Geometry::node_new_index maps the reference's node index (Object::meshIndex) to the derived one (DObj::root).
// The exit records (DExit) and the hit records (DHit) are derived here too, from the finished DNodes and from triangles[] /
// normals[] / uvs[]: copies of floats and words the library already holds, nothing computed.
// derive_layouts is the host half (rpt_derived_layout_host hands its arrays out as they are); false = this scene has no derived
// layout, and keeps the reference-layout kernel.  `s` is valid (validate_geometry) and has at least one octree node.
struct DerivedLayouts {
    std::vector<rptd::DNode> nodes;
    std::vector<int32_t> links;
    std::vector<rptd::DTri> tris, first;
    std::vector<rptd::DExit> exits;
    std::vector<rptd::DHit> hits;
};

bool derive_layouts(Geometry &g, const rpt_scene_desc &s, DerivedLayouts &L) {
    const size_t n = s.octree_count;
    if (n > (size_t)RPT_LINK_CHILD_MASK) return false;                 // a link holds 24 bits of child index
    std::vector<uint8_t> is_child(n, 0);
    for (size_t i = 0; i < n; i++) {
        const rpt_octree &o = s.octrees[i];
        if (o.children[0] == -1) continue;
        for (int c = 0; c < 8; c++) {
            if (o.children[c] != o.children[0] + c) return false;     // not consecutive: keep the general kernel
            if (is_child[(size_t)o.children[c]]) return false;        // a node with two parents: not a forest of trees
            is_child[(size_t)o.children[c]] = 1;
        }
    }
    std::vector<int> order;                                            // derived index -> reference index
    order.reserve(n);
    std::vector<int> &new_index = g.node_new_index;
    new_index.assign(n, -1);
    std::vector<int> level, next;
    for (size_t i = 0; i < n; i++) if (!is_child[i]) level.push_back((int)i);
    while (!level.empty()) {
        next.clear();
        for (int i : level) {
            new_index[(size_t)i] = (int)order.size();
            order.push_back(i);
            if (s.octrees[i].children[0] != -1)
                for (int c = 0; c < 8; c++) next.push_back(s.octrees[i].children[c]);
        }
        if (order.size() <= (size_t)RPT_TOP_MAX) g.top_count = (int)order.size();    // whole levels only
        level.swap(next);
    }
    if (order.size() != n) return false;                              // (cannot happen after validate_geometry: every node is a root or a child)
    std::vector<rptd::DNode> &nodes = L.nodes;
    std::vector<int32_t> &links = L.links;
    std::vector<rptd::DTri> &tris = L.tris;
    nodes.assign(n, rptd::DNode());
    links.assign(n, 0);
    tris.clear();
    for (size_t k = 0; k < n; k++) {
        const rpt_octree &o = s.octrees[order[k]];
        rptd::DNode &d = nodes[k];
        std::memset(&d, 0, sizeof d);
        d.minx = o.min.x; d.miny = o.min.y; d.minz = o.min.z;
        d.maxx = o.max.x; d.maxy = o.max.y; d.maxz = o.max.z;
        d.link = -1;
        if (o.children[0] != -1) {
            unsigned int leaf_mask = 0;
            for (int c = 0; c < 8; c++) leaf_mask |= (s.octrees[o.children[c]].children[0] == -1 ? 1u : 0u) << c;
            d.link = (int)((unsigned int)new_index[(size_t)o.children[0]] | (leaf_mask << 24));
            if (d.link == -1) return false;                            // (first child 0xffffff with eight leaf children: reserved for "leaf")
        }
        links[k] = d.link;
        for (int c = 0; c < 6; c++) d.nb[c] = o.neighbors[c] == -1 ? -1 : new_index[(size_t)o.neighbors[c]];
        d.leafBegin = (int)tris.size();
        d.leafCount = 0;
        if (o.children[0] == -1) {
            d.leafCount = o.trisCount;
            for (int t0 = o.trisIndex; t0 < o.trisIndex + o.trisCount; t0++) {
                const int t = s.octreeTris[t0];
                const rpt_float3 &A = s.vertices[s.triangles[9 * t + 0]];
                const rpt_float3 &B = s.vertices[s.triangles[9 * t + 3]];
                const rpt_float3 &C = s.vertices[s.triangles[9 * t + 6]];
                rptd::DTri r;
                std::memset(&r, 0, sizeof r);
                r.ax = A.x; r.ay = A.y; r.az = A.z;
                r.e1x = B.x - A.x; r.e1y = B.y - A.y; r.e1z = B.z - A.z;
                r.e2x = C.x - A.x; r.e2y = C.y - A.y; r.e2z = C.z - A.z;
                r.tri = t;
                tris.push_back(r);
            }
        }
    }
    if (tris.size() > (size_t)RPT_NODE_BEGIN_MASK) return false;      // (16.7 M triangle references: the general kernel takes such a scene)
    {   // the first record of every list again, by node index (load_first_tri) — before leafBegin gets the count packed into it
        std::vector<rptd::DTri> &first = L.first;
        first.resize(n);
        std::memset(first.data(), 0, first.size() * sizeof(rptd::DTri));
        for (size_t k = 0; k < n; k++) if (nodes[k].leafCount > 0) first[k] = tris[(size_t)nodes[k].leafBegin];
    }
    for (size_t k = 0; k < n; k++)          // leafBegin | min(leafCount, 255) << 24: see load_node_rec
        nodes[k].leafBegin = (int)((unsigned int)nodes[k].leafBegin | ((unsigned int)(nodes[k].leafCount < 255 ? nodes[k].leafCount : 255) << 24));
    // the exit records: (k, side) -> the box, and the index and begin word (a leaf) or the link (inner), of nodes[nodes[k].nb[side]]
    L.exits.resize(6 * n);
    for (size_t k = 0; k < n; k++)
        for (int c = 0; c < 6; c++) {
            rptd::DExit &e = L.exits[6 * k + (size_t)c];
            std::memset(&e, 0, sizeof e);
            e.a = -1;
            e.b = RPT_EXIT_INNER;
            const int nb = nodes[k].nb[c];
            if (nb == -1) continue;
            const rptd::DNode &d = nodes[(size_t)nb];
            e.minx = d.minx; e.miny = d.miny; e.minz = d.minz;
            e.maxx = d.maxx; e.maxy = d.maxy; e.maxz = d.maxz;
            if (d.link == -1) {
                e.a = nb;
                e.b = d.leafBegin;
                // (cannot happen: a count below 255 is the list's own, and the list ends inside the 0xffffff records checked above)
                if (e.b == RPT_EXIT_INNER || nb < 0 || nb > RPT_LINK_CHILD_MASK) return false;
            } else {
                e.a = d.link;                                           // (never -1: checked where the link was made)
            }
        }
    // the hit records: the floats that triangles[9 t + 3 c + 2] / [+ 1] name in normals[] / uvs[]
    const size_t n_tris = s.triangle_words / RPT_TRI_STRIDE;
    L.hits.resize(n_tris);
    for (size_t t = 0; t < n_tris; t++) {
        rptd::DHit &h = L.hits[t];
        std::memset(&h, 0, sizeof h);
        float *nrm[3] = {h.nA, h.nB, h.nC}, *tex[3] = {h.uvA, h.uvB, h.uvC};
        for (int c = 0; c < 3; c++) {
            const rpt_float3 &nv = s.normals[s.triangles[9 * t + 3 * (size_t)c + 2]];
            const rpt_float2 &tv = s.uvs[s.triangles[9 * t + 3 * (size_t)c + 1]];
            nrm[c][0] = nv.x; nrm[c][1] = nv.y; nrm[c][2] = nv.z;
            tex[c][0] = tv.x; tex[c][1] = tv.y;
        }
    }
    return true;
}

int build_derived_geometry(rpt_ctx *ctx, const rpt_scene_desc &s) {
    Geometry &g = *ctx->geo;
    g.compact_ok = false;
    g.top_count = 0;
    g.node_new_index.clear();
    if (s.octree_count == 0) {
        g.compact_ok = true;
        if (int rc = reserve(ctx, g.dnodes, 0)) return rc;
        if (int rc = reserve(ctx, g.dlinks, 0)) return rc;
        return reserve(ctx, g.dtris, 0);
    }
    DerivedLayouts L;
    if (!derive_layouts(g, s, L)) return RPT_OK;
    if (int rc = upload(ctx, g.dfirst, L.first.data(), L.first.size() * sizeof(rptd::DTri))) return rc;
    // (16 B of slack behind the triangle records: the cooperative 16-B staging loads of the persistent kernels never start past the
    // last record, but keep the buffer's end away from them all the same)
    if (int rc = upload(ctx, g.dnodes, L.nodes.data(), L.nodes.size() * sizeof(rptd::DNode))) return rc;
    if (int rc = upload(ctx, g.dlinks, L.links.data(), L.links.size() * sizeof(int32_t))) return rc;
    if (int rc = upload(ctx, g.dtris, L.tris.data(), L.tris.size() * sizeof(rptd::DTri))) return rc;
    if (int rc = upload(ctx, g.dexits, L.exits.data(), L.exits.size() * sizeof(rptd::DExit))) return rc;
    if (int rc = upload(ctx, g.dhits, L.hits.data(), L.hits.size() * sizeof(rptd::DHit))) return rc;
    g.compact_ok = true;
    return RPT_OK;
}

// What the host keeps of a scene's meshes: every node's box, which nodes hold their triangles inside it, how large those triangles
// are, and the sub-tree and triangle boxes of the meshes the scene's objects name.  Host only (rpt_upload_scene; rpt_tile_bitmap_host); `s` is valid
// (validate_geometry) and g.compact_ok is set.
void host_mesh_facts(Geometry &g, const rpt_scene_desc *s, int max_boxes, int max_triangles) {
    g.host_node_bounds.resize(s->octree_count * 6);
    for (size_t i = 0; i < s->octree_count; i++) {
        float *b = &g.host_node_bounds[6 * i];
        b[0] = s->octrees[i].min.x; b[1] = s->octrees[i].min.y; b[2] = s->octrees[i].min.z;
        b[3] = s->octrees[i].max.x; b[4] = s->octrees[i].max.y; b[5] = s->octrees[i].max.z;
    }
    // Which nodes hold all of their triangles inside their own box?  (Asked of mesh roots by the shadow-segment cull: a hit on a
    // triangle is a point of that triangle.)  Indices were validated above.
    // ... and how large are those triangles?  K = max |e1| |e2|, L = the longest edge, with e1 = fl(B - A), e2 = fl(C - A) as the walk
    // uses them: the float error of an accepted triangle hit is bounded through them (mesh_segment_apart, rpt_kernels.hip.h).
    g.node_holds_its_triangles.assign(s->octree_count, 0);
    g.node_tri_K.assign(s->octree_count, 0.0f);
    g.node_tri_L.assign(s->octree_count, 0.0f);
    for (size_t i = 0; i < s->octree_count; i++) {
        const rpt_octree &o = s->octrees[i];
        bool inside = o.trisCount >= 0;
        double K = 0.0, L = 0.0;
        for (int k = o.trisIndex; inside && k < o.trisIndex + o.trisCount; k++) {
            const int t = s->octreeTris[k];
            const rpt_float3 *vv[3];
            for (int c = 0; c < 3 && inside; c++) {
                const rpt_float3 &v = s->vertices[s->triangles[9 * t + 3 * c]];
                vv[c] = &v;
                inside = v.x >= o.min.x && v.x <= o.max.x && v.y >= o.min.y && v.y <= o.max.y && v.z >= o.min.z && v.z <= o.max.z;
            }
            if (!inside) break;
            const float e1[3] = {vv[1]->x - vv[0]->x, vv[1]->y - vv[0]->y, vv[1]->z - vv[0]->z}, e2[3] = {vv[2]->x - vv[0]->x, vv[2]->y - vv[0]->y, vv[2]->z - vv[0]->z};
            const double l1 = std::sqrt((double)e1[0] * e1[0] + (double)e1[1] * e1[1] + (double)e1[2] * e1[2]);
            const double l2 = std::sqrt((double)e2[0] * e2[0] + (double)e2[1] * e2[1] + (double)e2[2] * e2[2]);
            K = std::max(K, l1 * l2);
            L = std::max(L, std::max(l1, l2));
        }
        g.node_holds_its_triangles[i] = inside ? 1 : 0;
        g.node_tri_K[i] = std::nextafter((float)K, INFINITY);
        g.node_tri_L[i] = std::nextafter((float)L, INFINITY);
    }
    // the sub-tree boxes of every mesh the scene's objects name (rpt_tile_bitmap.hpp; a mesh that only a later Object[] names gets none)
    for (size_t i = 0; i < s->object_count && g.compact_ok; i++) {
        const rpt_object &o = s->objects[i];
        if (o.type != RPT_MESH || o.meshIndex < 0 || (size_t)o.meshIndex >= s->octree_count || g.mesh_boxes.count(o.meshIndex)) continue;
        if (!g.node_holds_its_triangles[(size_t)o.meshIndex] || !(16.2 * (double)g.node_tri_K[(size_t)o.meshIndex] <= 0.25)) continue;
        std::vector<float> boxes;
        if (!rptb::tiles::subtree_boxes(*s, o.meshIndex, max_boxes, boxes)) continue;
        g.mesh_boxes[o.meshIndex].swap(boxes);
        // ... and its triangle boxes (the same rule, the same restriction to lists inside the root's box; over the cap: none)
        std::vector<float> tri_boxes;
        if (max_triangles > 0 && rptb::tiles::triangle_boxes(*s, o.meshIndex, max_triangles, tri_boxes)) g.mesh_tri_boxes[o.meshIndex].swap(tri_boxes);
    }
}

// The constants of mesh_segment_apart (rpt_kernels.hip.h, where the derivation is): may a shadow ray's segment to the light be
// dropped for mesh object `o` when it stays beyond a plane of the root box, and with which margins?  Everything the argument
// assumes about THIS object in THIS frame is checked here, in double, on the float matrices the kernel reads; if anything fails
// the object is simply never culled (mslope < 0).
void mesh_segment_cull_record(const rpt_ctx *ctx, const rpt_object &o, rptd::DObj &d) {
    d.mslope = -1.0f;
    d.mcw = d.mconst = d.ms0 = 0.0f;
    d.mh[0] = d.mh[1] = d.mh[2] = -1.0f;
    d.win_t1 = 0.0f;
    if (o.type != RPT_MESH || !ctx->geo->compact_ok) return;
    const size_t mi = (size_t)o.meshIndex;
    if (o.meshIndex < 0 || mi * 6 + 5 >= ctx->geo->host_node_bounds.size() || mi >= ctx->geo->node_tri_K.size()) return;
    const float *nb = &ctx->geo->host_node_bounds[mi * 6];
    const double U = 5.9604644775390625e-8;
    // mesh_ray_misses_root: half extents about the centre the kernel reads, grown by 8u max(|lo|, |hi|)
    const float cen[3] = {d.cbx, d.cby, d.cbz};
    double h1 = 0.0;
    float mh[3];
    for (int k = 0; k < 3; k++) {
        if (!std::isfinite(nb[k]) || !std::isfinite(nb[k + 3]) || !std::isfinite(cen[k]) || !(nb[k] <= nb[k + 3])) return;
        const double h = std::max((double)nb[k + 3] - cen[k], (double)cen[k] - nb[k]);
        h1 += h;
        mh[k] = std::nextafter((float)(h + 8.0 * U * std::max(std::fabs((double)nb[k]), std::fabs((double)nb[k + 3])) + 1.0e-30), INFINITY);
        if (!std::isfinite(mh[k])) return;
    }
    for (int k = 0; k < 3; k++) d.mh[k] = mh[k];
    // mesh_segment_apart: only for a mesh whose lists stay inside its root box, with light propagation on (interval 0: no light is
    // ever sampled, opencl_kernel.cl:572), and only if everything the derivation assumes holds for these matrices
    if (d.mesh_in_box == 0.0f || ctx->interval != -1) return;
    const double K = ctx->geo->node_tri_K[mi], L = ctx->geo->node_tri_L[mi];
    double M3[3][3], I3[3][3], Mt[3], It[3], Ls[3][3], L0[3];
    for (int r = 0; r < 3; r++) {
        M3[r][0] = o.M[r].x; M3[r][1] = o.M[r].y; M3[r][2] = o.M[r].z; Mt[r] = o.M[r].w;
        I3[r][0] = o.InvM[r].x; I3[r][1] = o.InvM[r].y; I3[r][2] = o.InvM[r].z; It[r] = o.InvM[r].w;
        L0[r] = o.Lorentz[r + 1].x; Ls[r][0] = o.Lorentz[r + 1].y; Ls[r][1] = o.Lorentz[r + 1].z; Ls[r][2] = o.Lorentz[r + 1].w;
    }
    // c1 = ||M3 InvM3 - I||_F + 16u || |M3| |InvM3| ||_F,  c0 = |M3 InvM.t + M.t| + 16u (|| |M3| |InvM.t| || + |M.t|)
    double r3 = 0.0, km = 0.0, rt = 0.0, mit = 0.0, mt = 0.0;
    for (int i = 0; i < 3; i++) {
        double t = Mt[i], ta = 0.0;
        for (int j = 0; j < 3; j++) {
            double v = 0.0, va = 0.0;
            for (int k = 0; k < 3; k++) { v += M3[i][k] * I3[k][j]; va += std::fabs(M3[i][k]) * std::fabs(I3[k][j]); }
            v -= i == j ? 1.0 : 0.0;
            r3 += v * v;
            km += va * va;
            t += M3[i][j] * It[j];
            ta += std::fabs(M3[i][j]) * std::fabs(It[j]);
        }
        rt += t * t;
        mit += ta * ta;
        mt += Mt[i] * Mt[i];
    }
    const double c1 = std::sqrt(r3) + 16.0 * U * std::sqrt(km), c0 = std::sqrt(rt) + 16.0 * U * (std::sqrt(mit) + std::sqrt(mt));
    // dmin: |dw| >= (1 - |Ls^-1 L0|) / ||Ls^-1||_F for every unit light direction (dw = Ls nd - L0); halved for dw's own rounding
    double Li[3][3];
    if (!rptb::detail::invert3(Ls, Li)) return;
    double cvec[3], fro = 0.0, labs = 0.0;
    for (int i = 0; i < 3; i++) {
        cvec[i] = Li[i][0] * L0[0] + Li[i][1] * L0[1] + Li[i][2] * L0[2];
        for (int j = 0; j < 3; j++) { fro += Li[i][j] * Li[i][j]; labs += Ls[i][j] * Ls[i][j]; }
        labs += L0[i] * L0[i];
    }
    const double cn = std::sqrt(cvec[0] * cvec[0] + cvec[1] * cvec[1] + cvec[2] * cvec[2]);
    if (!(cn < 1.0 - 1.0e-6) || !(fro > 0.0)) return;
    const double dmin = 0.5 * (1.0 - cn) / std::sqrt(fro);
    if (!(16.0 * U * std::sqrt(labs) <= dmin)) return;                       // the float noise of dw itself
    const double slope = 16.2 * K + 3.2 * U;
    if (!(c1 <= 4.0e-4) || !(c0 <= 0.1 * dmin) || !(slope <= 0.25) || !std::isfinite(c1) || !std::isfinite(c0) || !std::isfinite(L) || !std::isfinite(h1)) return;
    d.mconst = std::nextafter((float)(slope * h1 * 1.001 + 4.0 * U * L + 1.0e-30), INFINITY);
    d.mslope = std::nextafter((float)(slope * 1.001), INFINITY);
    d.mcw = std::nextafter((float)(1.01 * c1 / dmin), INFINITY);
    d.ms0 = std::nextafter((float)(1.0e-4 + 1.01 * c0 / dmin), INFINITY);
}

// Per-frame DObj records: the primary-ray origin in each object's space and what follows from it
// (opencl_kernel.cl:314,318 / 336,341), with the kernel's operation order.
void build_dobjs(const rpt_ctx *ctx, const rpt_object *objs, int count, rptd::DObj *out) {
    for (int i = 0; i < count; i++) {
        const rpt_object &o = objs[i];
        const float vx = o.stationaryCam.y, vy = o.stationaryCam.z, vz = o.stationaryCam.w;
        float p[3];
        for (int r = 0; r < 3; r++) p[r] = o.InvM[r].x * vx + o.InvM[r].y * vy + o.InvM[r].z * vz + o.InvM[r].w * 1.0f;
        rptd::DObj d;
        std::memset(&d, 0, sizeof d);
        d.ox = p[0]; d.oy = p[1]; d.oz = p[2];
        const float rx = -p[0], ry = -p[1], rz = -p[2];
        d.sphere_c = (rx * rx + ry * ry + rz * rz) - 1.0f;
        const float ax = std::fabs(p[0]), ay = std::fabs(p[1]), az = std::fabs(p[2]);
        const float m1 = ax < ay ? ay : ax;
        const float m2 = m1 < az ? az : m1;
        d.winding = m2 < 1.0f ? -1.0f : 1.0f;
        // ---- culling data (approximate on purpose; see rpt_tile_bin_kernel) ----
        // object-space direction of a primary ray with camera direction nd: InvM3 * (interval * L[1..3][0] + L[1..3][1..3] * nd)
        const float interval = (float)ctx->interval;
        bool finite = true;
        for (int r = 0; r < 3; r++) {
            const float m[3] = {o.InvM[r].x, o.InvM[r].y, o.InvM[r].z};
            for (int c = 0; c < 3; c++) {
                const float lc[3] = {(&o.Lorentz[1].x)[c + 1], (&o.Lorentz[2].x)[c + 1], (&o.Lorentz[3].x)[c + 1]};
                d.B[3 * r + c] = m[0] * lc[0] + m[1] * lc[1] + m[2] * lc[2];
                finite = finite && std::isfinite(d.B[3 * r + c]);
            }
            d.b[r] = interval * (m[0] * o.Lorentz[1].x + m[1] * o.Lorentz[2].x + m[2] * o.Lorentz[3].x);
            finite = finite && std::isfinite(d.b[r]) && std::isfinite(p[r]);
        }
        d.cbx = d.cby = d.cbz = 0.0f;
        float radius = -1.0f;
        // (sphere: the float discriminant b^2 - c is off by up to ~1.5e-6 |oc|^2, see sphere_rect in rpt_screen_bounds.hpp)
        if (o.type == RPT_SPHERE) radius = std::sqrt(1.0f + 1.5e-6f * (d.sphere_c + 1.0f));
        else if (o.type == RPT_CUBE) radius = 1.7320508f;
        else if (o.type == RPT_MESH && (size_t)o.meshIndex * 6 + 5 < ctx->geo->host_node_bounds.size()) {
            const float *nb = &ctx->geo->host_node_bounds[(size_t)o.meshIndex * 6];
            d.cbx = 0.5f * (nb[0] + nb[3]); d.cby = 0.5f * (nb[1] + nb[4]); d.cbz = 0.5f * (nb[2] + nb[5]);
            const float ex = nb[3] - nb[0], ey = nb[4] - nb[1], ez = nb[5] - nb[2];
            radius = 0.5f * std::sqrt(ex * ex + ey * ey + ez * ez);
        }
        // a relative gamma beyond 20: the float evaluation of the boosted direction is too noisy for this approximate test
        finite = finite && std::isfinite(o.Lorentz[0].x) && std::fabs(o.Lorentz[0].x) <= 20.0f;
        d.rb = (finite && radius >= 0.0f && std::isfinite(radius)) ? radius * 1.02f + 1.0e-5f : -1.0f;
        d.root = (o.type == RPT_MESH && ctx->geo->compact_ok && o.meshIndex >= 0 && (size_t)o.meshIndex < ctx->geo->node_new_index.size())
                     ? ctx->geo->node_new_index[(size_t)o.meshIndex] : 0;
        d.mesh_in_box = (o.type == RPT_MESH && o.meshIndex >= 0 && (size_t)o.meshIndex < ctx->geo->node_holds_its_triangles.size() &&
                         ctx->geo->node_holds_its_triangles[(size_t)o.meshIndex] && ctx->geo->compact_ok) ? 1.0f : 0.0f;
        mesh_segment_cull_record(ctx, o, d);
        out[i] = d;
    }
}

// Per-frame image-plane rectangle of every object (rpt_screen_bounds.hpp) for the in-kernel lane-parallel cull.  A
// rectangle is a pure function of the object's 320 bytes, the interval and (meshes) the root bounds: an object whose
// record is byte-identical to the previous frame's (a camera at rest, a paused scene) keeps its rectangle.
struct RectBatch {
    rpt_ctx *ctx;
    const rpt_object *objs;
    rptb::Rect *out;
    int todo[64];
};
void rect_batch_item(void *arg, int k) {
    RectBatch &b = *(RectBatch *)arg;
    const int i = b.todo[k];
    const rpt_object &o = b.objs[i];
    const float *root = nullptr;
    if (o.type == RPT_MESH && o.meshIndex >= 0 && (size_t)o.meshIndex * 6 + 5 < b.ctx->geo->host_node_bounds.size())
        root = &b.ctx->geo->host_node_bounds[(size_t)o.meshIndex * 6];
    b.out[i] = b.ctx->rects[i] = rptb::certified_object_rect(o, b.ctx->interval, root);      // proposed by sampling, PROVEN or dropped (rpt_bounds_certify.hpp)
}
void build_rects(rpt_ctx *ctx, const rpt_object *objs, int count, rptb::Rect *out) {
    const bool comparable = ctx->rect_interval == ctx->interval && ctx->rect_geo_generation == ctx->geo->generation &&
                            ctx->rects.size() == (size_t)count && ctx->host_objects.size() == (size_t)count * sizeof(rpt_object);
    const rpt_object *prev = comparable ? (const rpt_object *)ctx->host_objects.data() : nullptr;
    ctx->rects.resize((size_t)count);
    RectBatch batch;
    batch.ctx = ctx;
    batch.objs = objs;
    batch.out = out;
    int n_todo = 0;
    for (int i = 0; i < count; i++) {
        if (i >= 64) { out[i] = ctx->rects[i] = rptb::full_rect(); continue; }      // the wave's mask has 64 bits: later objects are always tested
        if (prev && std::memcmp(&prev[i], &objs[i], sizeof objs[i]) == 0) { out[i] = ctx->rects[i]; continue; }
        batch.todo[n_todo++] = i;
    }
    // the bounds that have to be recomputed: a few on the submitting thread, a batch shared with the helper threads (rpt_workers.hpp;
    // cubes.txt, 34 moving objects: profiles/r03_host_threads.txt)
    if (n_todo >= RPT_RECT_BATCH_MIN) rpth::Workers::instance().parallel_for(n_todo, rect_batch_item, &batch);
    else for (int k = 0; k < n_todo; k++) rect_batch_item(&batch, k);
    ctx->rect_interval = ctx->interval;
    ctx->rect_geo_generation = ctx->geo->generation;
}

// Which objects stand still?  (Before build_rects, which moves the cache's key.)  A tile bitmap (rpt_tile_bitmap.hpp) is built for an
// object only once its record has been byte-identical in two consecutive calls, and is dropped with the first call in which it is not:
// an animated frame pays a memcmp it pays for the rectangles anyway and keeps today's mask, a still view pays for the build once.
void note_still_objects(rpt_ctx *ctx, const rpt_object *objs, int count) {
    const bool comparable = ctx->rect_interval == ctx->interval && ctx->rect_geo_generation == ctx->geo->generation &&
                            ctx->rects.size() == (size_t)count && ctx->host_objects.size() == (size_t)count * sizeof(rpt_object);
    const rpt_object *prev = comparable ? (const rpt_object *)ctx->host_objects.data() : nullptr;
    unsigned long long still = 0;
    for (int i = 0; prev && i < count && i < 64; i++)
        if (std::memcmp(&prev[i], &objs[i], sizeof objs[i]) == 0) still |= 1ull << i;
    ctx->bits_still = still;
    ctx->bits_tried &= still;
    ctx->bits_has &= still;
}

// ---- the free-look camera's orientation (rpt_set_orientation, rpt_orient_objects) ---------------------------------------------------
// R = Ry(yaw) Rx(pitch) Rz(roll) in double from the float angles (include/rpt.h has the three matrices and a worked example of each).
// false: a non-finite angle.  NULL = three zeros = the exact identity (sin 0 = 0, cos 0 = 1).
bool orientation_matrix(const float *ypr, double R[3][3]) {
    const double y = ypr ? (double)ypr[0] : 0.0, p = ypr ? (double)ypr[1] : 0.0, r = ypr ? (double)ypr[2] : 0.0;
    if (!std::isfinite(y) || !std::isfinite(p) || !std::isfinite(r)) return false;
    const double cy = std::cos(y), sy = std::sin(y), cp = std::cos(p), sp = std::sin(p), cr = std::cos(r), sr = std::sin(r);
    const double Ry[3][3] = {{cy, 0, sy}, {0, 1, 0}, {-sy, 0, cy}}, Rx[3][3] = {{1, 0, 0}, {0, cp, sp}, {0, -sp, cp}}, Rz[3][3] = {{cr, sr, 0}, {-sr, cr, 0}, {0, 0, 1}};
    double T[3][3];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) T[i][j] = Rx[i][0] * Rz[0][j] + Rx[i][1] * Rz[1][j] + Rx[i][2] * Rz[2][j];
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) R[i][j] = Ry[i][0] * T[0][j] + Ry[i][1] * T[1][j] + Ry[i][2] * T[2][j];
    return true;
}

bool is_identity(const double R[3][3]) {
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++)
            if (R[i][j] != (i == j ? 1.0 : 0.0)) return false;
    return true;
}

// out = m diag(1, R) for a matrix of Object.Lorentz's layout (four rows, t first): column 0 kept, entry (r, 1 + c) the three-term sum in
// double of the row's float space entries times R's column c, rounded to float once.  out may be m.
void rebase_columns(const rpt_float4 m[4], const double R[3][3], rpt_float4 out[4]) {
    for (int r = 0; r < 4; r++) {
        const double l[3] = {m[r].y, m[r].z, m[r].w};
        float o[3];
        for (int c = 0; c < 3; c++) o[c] = (float)(l[0] * R[0][c] + l[1] * R[1][c] + l[2] * R[2][c]);
        out[r].x = m[r].x; out[r].y = o[0]; out[r].z = o[1]; out[r].w = o[2];
    }
}

// out = diag(1, R^T) m: row 0 kept, entry (1 + r, c) the three-term sum in double of R's column r times the float entries of column c
void rebase_rows(const rpt_float4 m[4], const double R[3][3], rpt_float4 out[4]) {
    float o[3][4];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 4; c++)
            o[r][c] = (float)(R[0][r] * (double)(&m[1].x)[c] + R[1][r] * (double)(&m[2].x)[c] + R[2][r] * (double)(&m[3].x)[c]);
    out[0] = m[0];
    for (int r = 0; r < 3; r++) { out[r + 1].x = o[r][0]; out[r + 1].y = o[r][1]; out[r + 1].z = o[r][2]; out[r + 1].w = o[r][3]; }
}

// The change of basis of the camera frame on `count` objects: Lorentz' = Lorentz diag(1, R), InvLorentz' = diag(1, R^T) InvLorentz, every
// other byte copied.  The exact identity copies everything (so -0.0f and non-finite entries keep their bytes).  out may be in.
void orient_objects(const rpt_object *in, int count, const double R[3][3], rpt_object *out) {
    if (out != in) std::memmove(out, in, (size_t)count * sizeof(rpt_object));
    if (is_identity(R)) return;
    for (int i = 0; i < count; i++) {
        rebase_columns(out[i].Lorentz, R, out[i].Lorentz);
        rebase_rows(out[i].InvLorentz, R, out[i].InvLorentz);
    }
}

int validate_objects(rpt_ctx *ctx, const rpt_object *objs, int count) {
    for (int i = 0; i < count; i++) {
        const rpt_object &o = objs[i];
        if (o.type < RPT_SPHERE || o.type > RPT_MESH) return fail(ctx, RPT_ERR_SCENE, "object: unknown type");
        if (o.type == RPT_MESH && (o.meshIndex < 0 || (size_t)o.meshIndex >= ctx->geo->octree_count))
            return fail(ctx, RPT_ERR_SCENE, "object: meshIndex is not an octree node");
        if (o.textureIndex != -1) {
            if (o.textureIndex < 0 || o.textureWidth <= 0 || o.textureHeight <= 0 ||
                (unsigned long long)o.textureIndex + 3ull * (unsigned long long)o.textureWidth * (unsigned long long)o.textureHeight > ctx->geo->textures.bytes)
                return fail(ctx, RPT_ERR_SCENE, "object: texture lies outside the texture pool");
        }
    }
    return RPT_OK;
}

int local_tile_count(const rpt_ctx *ctx);

int ensure_outputs(rpt_ctx *ctx) {
    const size_t px = (size_t)ctx->width * ctx->height;
    if (ctx->colour_plane) {
        const int local_tiles = local_tile_count(ctx);
        if (!ctx->external_plane)
            if (int rc = reserve(ctx, ctx->owned_plane, (size_t)local_tiles * RPT_TILE_ROWS * ctx->width * 4)) return rc;
    } else if (!ctx->external_out) {
        if (px * 16 > ctx->owned_out.capacity || ctx->owned_out.bytes != px * 16) {
            if (int rc = reserve(ctx, ctx->owned_out, px * 16)) return rc;
            RPT_HIP(ctx, hipMemsetAsync(ctx->owned_out.ptr, 0, px * 16, ctx->stream));
        }
    }
    if (ctx->want_owned_rgb) {
        if (int rc = reserve(ctx, ctx->owned_rgb, px * 12)) return rc;
    }
    if (ctx->want_owned_doppler && ctx->doppler) {
        if (int rc = reserve(ctx, ctx->owned_doppler, px * RPT_DOPPLER_RECORD * sizeof(float))) return rc;
    }
    return RPT_OK;
}

// local tiles of this context: local tile t is global tile (t >> run_log2) * tile_step + first_tile + (t & (run - 1))
int local_tile_count(const rpt_ctx *ctx) {
    const int tiles = (ctx->height + RPT_TILE_ROWS - 1) / RPT_TILE_ROWS;
    const int run = 1 << ctx->run_log2;
    if (ctx->first_tile >= tiles) return 0;
    const int full_periods = (tiles - ctx->first_tile) / ctx->tile_step;          // periods whose whole run may lie inside
    const int rest = tiles - ctx->first_tile - full_periods * ctx->tile_step;    // tiles of the last, partial period
    return full_periods * run + (rest < run ? rest : run);
}

// The band of tile rows that holds the meshes' screen rectangles (whole-frame contexts only), grown by one row each way:
// where the frame's longest waves live.  false: no such band.
bool mesh_band(const rpt_ctx *ctx, float aspect, int tile_rows, int &ty0, int &ty1) {
    if (!(ctx->first_tile == 0 && ctx->tile_step == 1 && ctx->run_log2 == 0 && ctx->rects.size() == (size_t)ctx->object_count)) return false;
    float v0 = 3e38f, v1 = -3e38f;
    const rpt_object *objs = (const rpt_object *)ctx->host_objects.data();
    for (int i = 0; i < ctx->object_count; i++)
        if (objs[i].type == RPT_MESH && ctx->rects[i].u0 <= ctx->rects[i].u1) {
            v0 = std::min(v0, ctx->rects[i].v0);
            v1 = std::max(v1, ctx->rects[i].v1);
        }
    if (!(v0 <= v1)) return false;
    // under a lens row y looks through v = s (y / H - 1/2).  The band only ORDERS the dispatch of the band-first kernels (a wrong band
    // renders the same pixels later), and the un-culled lens kernel a wide lens falls back to is not band-first: nothing depends on it
    if (ctx->v_fov != 0.0f) { v0 /= ctx->lens_scale; v1 /= ctx->lens_scale; }
    const float H = (float)ctx->height;
    auto clampi = [](float x, int lo, int hi) { return x < (float)lo ? lo : (x > (float)hi ? hi : (int)x); };
    ty0 = clampi(std::floor((v0 + 0.5f) * H / 8.0f) - 1, 0, tile_rows - 1);
    ty1 = clampi(std::floor((v1 + 0.5f) * H / 8.0f) + 1, 0, tile_rows - 1);
    (void)aspect;
    return ty1 >= ty0;
}

// The band-first kernels' dispatch order: whole-frame contexts only, a band that does not already start the frame, at most half of it.
void set_band_first(const rpt_ctx *ctx, rptd::KernelArgs &a, int tiles) {
    int ty0 = 0, ty1 = -1;
    if (mesh_band(ctx, a.aspect, tiles, ty0, ty1) && ty0 > 0 && (ty1 - ty0 + 1) * 2 < tiles) { a.first_ty = ty0; a.first_h = ty1 - ty0 + 1; }
}

#ifdef RPT_DIAGNOSTICS
// Persistent kernels (rpt_persistent.hip.h): claim geometry, counters, grid = what the chip holds at once.
int launch_persistent(rpt_ctx *ctx, rptd::KernelArgs &a, int tiles, int v) {
    a.tiles_x = (ctx->width + 7) / 8;
    a.runs_x = (a.tiles_x + RPT_SKY_RUN - 1) / RPT_SKY_RUN;
    a.first_ty = 0;
    a.first_h = 0;
    int ty0 = 0, ty1 = -1;
    static const bool no_band = std::getenv("RPT_NO_BAND") != nullptr;      // (experiment knob)
    if (!no_band && mesh_band(ctx, a.aspect, tiles, ty0, ty1)) { a.first_ty = ty0; a.first_h = ty1 - ty0 + 1; }
    const long long band = (long long)a.first_h * a.tiles_x, sky = (long long)(tiles - a.first_h) * a.runs_x;
    // index / tiles_x by multiplication with ceil(2^32 / tiles_x): exact while index * tiles_x < 2^32
    if (a.runs_x < 2 || (band + sky + 64) * a.tiles_x >= (1ll << 32)) return -1;     // (tiny or enormous frames: the caller takes the per-tile-launch kernel)
    a.tiles_x_magic = (unsigned int)((1ull << 32) / (unsigned long long)a.tiles_x + 1ull);
    a.runs_x_magic = (unsigned int)((1ull << 32) / (unsigned long long)a.runs_x + 1ull);
    a.band_tiles = (int)band;
    a.sky_runs = (int)sky;
    const size_t counter_bytes = (size_t)2 * RPT_CLAIM_QUEUES * RPT_CLAIM_STRIDE * sizeof(unsigned int);
    if (!ctx->claim_counters.ptr) {
        if (int rc = reserve(ctx, ctx->claim_counters, counter_bytes)) return rc;
        RPT_HIP(ctx, hipMemsetAsync(ctx->claim_counters.ptr, 0, counter_bytes, ctx->stream));
        ctx->claim_epoch = 0;
    }
    a.claim_set = (int)(ctx->claim_epoch++ & 1u);
    unsigned int *claims = (unsigned int *)ctx->claim_counters.ptr;
    const long long want = (band + sky + 3) / 4;
    static const int wgs_per_cu = std::getenv("RPT_WGS_PER_CU") ? std::atoi(std::getenv("RPT_WGS_PER_CU")) : 5;     // (experiment knob)
    const unsigned int wgs = (unsigned int)std::max(1ll, std::min((long long)ctx->cu_count * wgs_per_cu, want));
    switch (v) {
    case 60: hipLaunchKernelGGL(rptd::rpt_render_kernel_persistent_w5, dim3(wgs), dim3(256), 0, ctx->stream, a, a.out16, a.plane, a.debug_rgb, claims); break;
    case 62: hipLaunchKernelGGL(rptd::rpt_render_kernel_persistent_direct_w5, dim3(wgs), dim3(256), 0, ctx->stream, a, a.out16, a.plane, a.debug_rgb, claims); break;
    case 63: hipLaunchKernelGGL(rptd::rpt_render_kernel_persistent_classic_w5, dim3(wgs), dim3(256), 0, ctx->stream, a, a.out16, a.plane, a.debug_rgb, claims); break;
    default: return fail(ctx, RPT_ERR_ARG, "unknown persistent kernel variant");
    }
    return RPT_OK;
}
#endif

#ifdef RPT_DIAGNOSTICS
// librpt_hip_diag.so only: the measurement arms (rpt_diag_kernels.hip.h)
#define RPT_LAUNCH_X(N) case N: hipLaunchKernelGGL(rptd::rpt_render_kernel_x##N, grid, dim3(256), 0, ctx->stream, a); break;
void launch_sky_fill(rpt_ctx *ctx, const rptd::KernelArgs &a, int tiles, const int box[4]);      // (arm 786; defined with the sky split, below)
int launch_diagnostic(rpt_ctx *ctx, rptd::KernelArgs &a, dim3 grid, int tiles, int v) {
    if (v == 143 || v == 2573 || (v >= 256 && v < 1000 && (v & 8))) set_band_first(ctx, a, tiles);     // (DiagPolicy::band_first)
    switch (v) {
    case 26: {   // round 1's default: per-tile object masks from a prepass kernel
        const int tiles_x = ((ctx->width + 31) / 32) * 4;          // tiles per row as the 32-pixel-wide blocks see them
        const int n_tiles = tiles_x * tiles;
        if (int rc = reserve(ctx, ctx->tile_masks, (size_t)n_tiles * 8)) return rc;
        a.mask_tiles_x = tiles_x;
        a.n_tiles = n_tiles;
        a.tile_masks = (unsigned long long *)ctx->tile_masks.ptr;
        hipLaunchKernelGGL(rptd::rpt_tile_bin_kernel, dim3((n_tiles + 255) / 256), dim3(256), 0, ctx->stream, a);
        hipLaunchKernelGGL(rptd::rpt_render_kernel_v1_masked_w5, grid, dim3(256), 0, ctx->stream, a);
        break;
    }
    case 40: hipLaunchKernelGGL(rptd::rpt_render_kernel_ballot_w4, dim3(grid.x * 4, grid.y), dim3(64), 0, ctx->stream, a); break;      // (kernel 41's body: one wave per workgroup)
    case 42:      // (kernel 41 as the compiler fits it into six waves: no parking, scratch)
        if (ctx->geo->exact_rcp_ok) hipLaunchKernelGGL(rptd::rpt_render_kernel_ballot_w6, dim3(grid.x * 4, grid.y), dim3(64), 0, ctx->stream, a);
        else hipLaunchKernelGGL(rptd::rpt_render_kernel_ballot_ieee_w6, dim3(grid.x * 4, grid.y), dim3(64), 0, ctx->stream, a);
        break;
    case 141: hipLaunchKernelGGL(rptd::rpt_render_kernel_r02walk_w5, grid, dim3(256), 0, ctx->stream, a); break;
    case 143: hipLaunchKernelGGL(rptd::rpt_render_kernel_r02walk_first_w5, grid, dim3(256), 0, ctx->stream, a); break;
    case 60: case 62: case 63: {
        const int rc = launch_persistent(ctx, a, tiles, v);
        if (rc > 0) return rc;
        if (rc < 0) hipLaunchKernelGGL(rptd::rpt_render_kernel_ballot_w5, dim3(grid.x * 4, grid.y), dim3(64), 0, ctx->stream, a);     // (tiny or enormous frames: the product kernel)
        break;
    }
    case 61: hipLaunchKernelGGL(rptd::rpt_render_kernel_queue_w5, grid, dim3(256), 0, ctx->stream, a); break;
    RPT_LAUNCH_X(256) RPT_LAUNCH_X(257) RPT_LAUNCH_X(259) RPT_LAUNCH_X(261) RPT_LAUNCH_X(263) RPT_LAUNCH_X(265) RPT_LAUNCH_X(269)
    RPT_LAUNCH_X(273) RPT_LAUNCH_X(277) RPT_LAUNCH_X(285) RPT_LAUNCH_X(305) RPT_LAUNCH_X(317) RPT_LAUNCH_X(337) RPT_LAUNCH_X(349) RPT_LAUNCH_X(401) RPT_LAUNCH_X(785) RPT_LAUNCH_X(529) RPT_LAUNCH_X(541) RPT_LAUNCH_X(561) RPT_LAUNCH_X(573) RPT_LAUNCH_X(621) RPT_LAUNCH_X(641) RPT_LAUNCH_X(653)
    case 1257: hipLaunchKernelGGL(rptd::rpt_render_kernel_x257_w6, grid, dim3(256), 0, ctx->stream, a); break;
    case 2257: hipLaunchKernelGGL(rptd::rpt_render_kernel_x257_w4, grid, dim3(256), 0, ctx->stream, a); break;
    case 2259: hipLaunchKernelGGL(rptd::rpt_render_kernel_x259_w4, grid, dim3(256), 0, ctx->stream, a); break;
    case 2263: hipLaunchKernelGGL(rptd::rpt_render_kernel_x263_w4, grid, dim3(256), 0, ctx->stream, a); break;
    RPT_LAUNCH_X(689) RPT_LAUNCH_X(701)          // kernel 41's / 43's walk launched four waves per workgroup (what the product did before)
    case 2573: hipLaunchKernelGGL(rptd::rpt_render_kernel_x573_w4, grid, dim3(256), 0, ctx->stream, a); break;      // the latency kernel at 4 waves per SIMD (128 VGPRs, no scratch)
    case 7:
        if (int rc = reserve(ctx, ctx->counters, 16 * sizeof(unsigned long long))) return rc;
        RPT_HIP(ctx, hipMemsetAsync(ctx->counters.ptr, 0, 16 * sizeof(unsigned long long), ctx->stream));
        a.counters = (unsigned long long *)ctx->counters.ptr;
        hipLaunchKernelGGL(rptd::rpt_render_kernel_v1_diag, grid, dim3(256), 0, ctx->stream, a);
        break;
    case 8: hipLaunchKernelGGL(rptd::rpt_render_kernel_primary_only, grid, dim3(256), 0, ctx->stream, a); break;
    case 786: {  // MEASUREMENT (the image of an empty Object[] only): the sky fill of a split frame alone, over the whole frame
        if (!a.out16) return fail(ctx, RPT_ERR_ARG, "variant 786 writes the 16-byte framebuffer only");
        const int no_box[4] = {0, 0, 0, 0};
        launch_sky_fill(ctx, a, tiles, no_box);
        break;
    }
    case 11:
        if (int rc = reserve(ctx, ctx->wave_times, (size_t)grid.x * grid.y * 4 * 10 * sizeof(unsigned long long))) return rc;
        RPT_HIP(ctx, hipMemsetAsync(ctx->wave_times.ptr, 0, ctx->wave_times.bytes, ctx->stream));
        a.wave_times = (unsigned long long *)ctx->wave_times.ptr;
        hipLaunchKernelGGL(rptd::rpt_render_kernel_v1_timeline, grid, dim3(256), 0, ctx->stream, a);
        break;
    default: return fail(ctx, RPT_ERR_ARG, "unknown kernel variant");
    }
    return RPT_OK;
}
#endif

// ---- the equirectangular camera (rpt_set_projection, rpt_projection_tables) ---------------------------------------------------------
// {h_fov, v_fov, yaw}: NULL = the full sphere; h_fov in (0, 2 pi], v_fov in (0, pi] (the float nearest 2 pi and pi included), yaw finite
bool projection_params(const float *params, float out[3]) {
    const float p[3] = {params ? params[0] : (float)(2.0 * RPT_PI_D), params ? params[1] : (float)RPT_PI_D, params ? params[2] : 0.0f};
    if (!(p[0] > 0.0f && p[0] <= (float)(2.0 * RPT_PI_D)) || !(p[1] > 0.0f && p[1] <= (float)RPT_PI_D) || !std::isfinite(p[2])) return false;
    for (int k = 0; k < 3; k++) out[k] = p[k];
    return true;
}

// lambda_x = yaw + h_fov ((x + 0.5) / W - 0.5), phi_y = v_fov ((y + 0.5) / H - 0.5), in double from the float parameters; the tables hold
// the float-rounded sine and cosine of each (cols: 2 W floats, rows: 2 H floats)
void projection_fill(const float params[3], int width, int height, float *cols, float *rows) {
    const double h_fov = params[0], v_fov = params[1], yaw = params[2];
    for (int x = 0; x < width; x++) {
        const double lambda = yaw + h_fov * (((double)x + 0.5) / (double)width - 0.5);
        cols[2 * (size_t)x] = (float)std::sin(lambda);
        cols[2 * (size_t)x + 1] = (float)std::cos(lambda);
    }
    for (int y = 0; y < height; y++) {
        const double phi = v_fov * (((double)y + 0.5) / (double)height - 0.5);
        rows[2 * (size_t)y] = (float)std::sin(phi);
        rows[2 * (size_t)y + 1] = (float)std::cos(phi);
    }
}

// The device tables of the context's projection at n times this frame's size: n = 1 the frame's own (ctx->pano), n = aa_n the refine
// pass's (ctx->aa_pano: sample (sx, sy) of pixel (x, y) looks along pixel (n x + sx, n y + sy) of the n W x n H panorama).  Rebuilt only
// when n, the size or the parameters changed, and uploaded in stream order (StagedUpload).
int ensure_projection_tables(rpt_ctx *ctx, ProjectionTables &t, int n) {
    if (t.n == n && t.width == ctx->width && t.height == ctx->height && std::memcmp(t.params, ctx->projection_params, sizeof t.params) == 0) return RPT_OK;
    const size_t w = (size_t)n * ctx->width, h = (size_t)n * ctx->height;
    float *host = nullptr;
    if (int rc = staged_host(ctx, t.upload, 2 * (w + h) * sizeof(float), (void **)&host)) return rc;
    projection_fill(ctx->projection_params, (int)w, (int)h, host, host + 2 * w);
    if (int rc = staged_copy(ctx, t.upload)) return rc;
    t.n = n;
    t.width = ctx->width;
    t.height = ctx->height;
    std::memcpy(t.params, ctx->projection_params, sizeof t.params);
    return RPT_OK;
}

// ---- the kernels a frame can get: one table shape, one row per kernel, found by (camera, colour, form) ------------------------------
// variant   what rpt_last_variant (the colour kernels), rpt_last_aa_variant (the refine kernels) and rpt_last_events_variant report
// camera    the pinhole, the panorama (rpt_set_projection) or the pinhole under a lens (rpt_set_field_of_view)
// colour    plain, the Doppler twin (rpt_set_doppler) or the sky (rpt_set_environment: carries Doppler as a run-time flag, serves both)
// form      which walk, which culls, which arithmetic (Form below)
// kernel    launched with grid (4 ceil(W / 32), row tiles) x 64 threads; null: the relaxed-arithmetic build (rpt_relaxed.hip), launched
//           through rpt_launch_relaxed_kernel
// ieee      the kernel's IEEE-division form, launched instead for scenes outside rcp_exact's domain (rpt_scene_exact_rcp); where a row
//           has one, rpt_last_exact_rcp says whether the row's own kernel ran
// choose_kernels() below decides the three keys from the settings, in this order: the form from the variant, the call and the scene; the
// panorama; the proven window; MSAA; then the colour — the sky is looked up BEFORE Doppler, since a sky kernel serves Doppler off and on —
// and the lens LAST, as the lens form of whatever every other setting chose.  A key without a row is a refusal.
using rptd::Camera;
enum class Colour { plain, doppler, sky };
enum class Form {
    // what rpt_set_variant takes, by the number of its pinhole / plain row
    ref_layout,       // 1   the reference's octree layout (any valid octree), un-culled
    unculled,         // 3   every object tested everywhere
    walk,             // 41  the wave's object mask, the octree walk one record at a time
    walk_first,       // 43  ... the walk an iteration ahead, the band of tile rows that holds the meshes dispatched first
    analytic,         // 44  no walk compiled in (an Object[] without a mesh)
    ieee,             // 48  41 with the IEEE division whatever the scene (the A/B arm)
    ieee_first,       // 49  43 likewise
    relaxed5,         // 50  41's body with OpenCL's default arithmetic, 5 waves per SIMD
    relaxed6,         // 51  ... 6 waves per SIMD
    // reached through other settings only
    msaa,             // 46  MSAASAMPLES > 1 (rpt_set_msaa) of the default kernels
    msaa_unculled,    // 47  ... of the un-culled one
    record,           // 240 / 540  the Doppler debug kernel (rpt_set_debug_doppler), un-culled
    diagnostic,       // a measurement arm of librpt_hip_diag.so (launch_diagnostic): no row here
};
constexpr bool settable(Form f) { return f <= Form::relaxed6; }
// ... dispatches the band of tile rows that holds the meshes first (KernelArgs::first_h): what the kernels' policies say
constexpr bool band_first(Form f) { return f == Form::walk_first || f == Form::ieee_first; }
static_assert(rptd::BallotFirstExact::band_first && rptd::BallotFirst::band_first && !rptd::RefLayout::band_first && !rptd::Unculled::band_first &&
              !rptd::BallotExact::band_first && !rptd::Ballot::band_first && !rptd::Analytic::band_first && !rptd::DopplerRecorded::band_first,
              "band_first(Form) is the policies' band_first");
static_assert(rptd::Lens<rptd::Environment<rptd::BallotFirstExact>>::band_first && rptd::Lens<rptd::DopplerTwin<rptd::BallotFirst>>::band_first &&
              !rptd::Lens<rptd::Environment<rptd::BallotExact>>::band_first && !rptd::PanoramaWalk::band_first,
              "the camera and colour policies keep the band_first of the form they wrap (the panorama has no band-first form)");
static_assert(!rptd::Raymap<rptd::BallotExact>::band_first && !rptd::Raymap<rptd::BallotExact>::object_mask && !rptd::Raymap<rptd::Ballot>::tile_bits &&
              rptd::DopplerTwin<rptd::Raymap<rptd::Ballot>>::culled && !rptd::Environment<rptd::Raymap<rptd::Unculled>>::culled,
              "the ray-map policies: no band-first form, no object mask, no tile bitmaps; the shadow-segment culls of the form they wrap");
// ... culls with the per-object screen regions, which are PROVEN inside their window only (the relaxed builds cull with the same regions
// but keep culling outside the window: a known gap, ADVICE.md, third item, kept as it is here)
constexpr bool needs_proven_window(Form f) { return f == Form::walk || f == Form::walk_first || f == Form::analytic || f == Form::ieee || f == Form::ieee_first; }
constexpr int relaxed_waves(Form f) { return f == Form::relaxed5 ? 5 : (f == Form::relaxed6 ? 6 : 0); }

struct KernelRow {
    int variant;
    Camera camera;
    Colour colour;
    Form form;
    const void *kernel;
    const void *ieee;
};
#define RPT_KERNEL(name) reinterpret_cast<const void *>(&rptd::name)
const KernelRow colour_table[] = {
    {1,   Camera::pinhole,  Colour::plain,   Form::ref_layout,    RPT_KERNEL(rpt_render_kernel_v0),                         nullptr},
    {3,   Camera::pinhole,  Colour::plain,   Form::unculled,      RPT_KERNEL(rpt_render_kernel_unculled_w5),                nullptr},
    {41,  Camera::pinhole,  Colour::plain,   Form::walk,          RPT_KERNEL(rpt_render_kernel_ballot_w5),                  RPT_KERNEL(rpt_render_kernel_ballot_ieee_w5)},
    {43,  Camera::pinhole,  Colour::plain,   Form::walk_first,    RPT_KERNEL(rpt_render_kernel_ballot_first_w5),            RPT_KERNEL(rpt_render_kernel_ballot_first_ieee_w5)},
    {44,  Camera::pinhole,  Colour::plain,   Form::analytic,      RPT_KERNEL(rpt_render_kernel_analytic_w8),                nullptr},
    {48,  Camera::pinhole,  Colour::plain,   Form::ieee,          RPT_KERNEL(rpt_render_kernel_ballot_ieee_w5),             nullptr},
    {49,  Camera::pinhole,  Colour::plain,   Form::ieee_first,    RPT_KERNEL(rpt_render_kernel_ballot_first_ieee_w5),       nullptr},
    {50,  Camera::pinhole,  Colour::plain,   Form::relaxed5,      nullptr,                                                  nullptr},
    {51,  Camera::pinhole,  Colour::plain,   Form::relaxed6,      nullptr,                                                  nullptr},
    {46,  Camera::pinhole,  Colour::plain,   Form::msaa,          RPT_KERNEL(rpt_render_kernel_msaa_w5),                    nullptr},
    {47,  Camera::pinhole,  Colour::plain,   Form::msaa_unculled, RPT_KERNEL(rpt_render_kernel_msaa_unculled_w5),           nullptr},
    {203, Camera::pinhole,  Colour::doppler, Form::unculled,      RPT_KERNEL(rpt_render_kernel_unculled_doppler_w5),        nullptr},
    {240, Camera::pinhole,  Colour::doppler, Form::record,        RPT_KERNEL(rpt_render_kernel_doppler_record_w5),          nullptr},
    {241, Camera::pinhole,  Colour::doppler, Form::walk,          RPT_KERNEL(rpt_render_kernel_ballot_doppler_w5),          RPT_KERNEL(rpt_render_kernel_ballot_ieee_doppler_w5)},
    {243, Camera::pinhole,  Colour::doppler, Form::walk_first,    RPT_KERNEL(rpt_render_kernel_ballot_first_doppler_w5),    RPT_KERNEL(rpt_render_kernel_ballot_first_ieee_doppler_w5)},
    {244, Camera::pinhole,  Colour::doppler, Form::analytic,      RPT_KERNEL(rpt_render_kernel_analytic_doppler_w8),        nullptr},
    {248, Camera::pinhole,  Colour::doppler, Form::ieee,          RPT_KERNEL(rpt_render_kernel_ballot_ieee_doppler_w5),     nullptr},
    {249, Camera::pinhole,  Colour::doppler, Form::ieee_first,    RPT_KERNEL(rpt_render_kernel_ballot_first_ieee_doppler_w5), nullptr},
    {603, Camera::pinhole,  Colour::sky,     Form::unculled,      RPT_KERNEL(rpt_render_kernel_env_unculled_w5),            nullptr},
    {641, Camera::pinhole,  Colour::sky,     Form::walk,          RPT_KERNEL(rpt_render_kernel_env_ballot_w5),              RPT_KERNEL(rpt_render_kernel_env_ballot_ieee_w5)},
    {643, Camera::pinhole,  Colour::sky,     Form::walk_first,    RPT_KERNEL(rpt_render_kernel_env_ballot_first_w5),        RPT_KERNEL(rpt_render_kernel_env_ballot_first_ieee_w5)},
    {644, Camera::pinhole,  Colour::sky,     Form::analytic,      RPT_KERNEL(rpt_render_kernel_env_analytic_w8),            nullptr},
    // the panorama: no object mask, so no band-first form (a walk_first choice gets the walk) and no forced-IEEE arms
    {303, Camera::equirect, Colour::plain,   Form::unculled,      RPT_KERNEL(rpt_render_kernel_pano_unculled_w5),           nullptr},
    {341, Camera::equirect, Colour::plain,   Form::walk,          RPT_KERNEL(rpt_render_kernel_pano_w5),                    RPT_KERNEL(rpt_render_kernel_pano_ieee_w5)},
    {344, Camera::equirect, Colour::plain,   Form::analytic,      RPT_KERNEL(rpt_render_kernel_pano_analytic_w8),           nullptr},
    {503, Camera::equirect, Colour::doppler, Form::unculled,      RPT_KERNEL(rpt_render_kernel_pano_unculled_doppler_w5),   nullptr},
    {540, Camera::equirect, Colour::doppler, Form::record,        RPT_KERNEL(rpt_render_kernel_pano_doppler_record_w5),     nullptr},
    {541, Camera::equirect, Colour::doppler, Form::walk,          RPT_KERNEL(rpt_render_kernel_pano_doppler_w5),            RPT_KERNEL(rpt_render_kernel_pano_ieee_doppler_w5)},
    {544, Camera::equirect, Colour::doppler, Form::analytic,      RPT_KERNEL(rpt_render_kernel_pano_analytic_doppler_w8),   nullptr},
    {703, Camera::equirect, Colour::sky,     Form::unculled,      RPT_KERNEL(rpt_render_kernel_env_pano_unculled_w5),       nullptr},
    {741, Camera::equirect, Colour::sky,     Form::walk,          RPT_KERNEL(rpt_render_kernel_env_pano_w5),                RPT_KERNEL(rpt_render_kernel_env_pano_ieee_w5)},
    {744, Camera::equirect, Colour::sky,     Form::analytic,      RPT_KERNEL(rpt_render_kernel_env_pano_analytic_w8),       nullptr},
    {803, Camera::lens,     Colour::plain,   Form::unculled,      RPT_KERNEL(rpt_render_kernel_lens_unculled_w5),           nullptr},
    {841, Camera::lens,     Colour::plain,   Form::walk,          RPT_KERNEL(rpt_render_kernel_lens_ballot_w5),             RPT_KERNEL(rpt_render_kernel_lens_ballot_ieee_w5)},
    {843, Camera::lens,     Colour::plain,   Form::walk_first,    RPT_KERNEL(rpt_render_kernel_lens_ballot_first_w5),       RPT_KERNEL(rpt_render_kernel_lens_ballot_first_ieee_w5)},
    {844, Camera::lens,     Colour::plain,   Form::analytic,      RPT_KERNEL(rpt_render_kernel_lens_analytic_w8),           nullptr},
    {813, Camera::lens,     Colour::doppler, Form::unculled,      RPT_KERNEL(rpt_render_kernel_lens_doppler_unculled_w5),   nullptr},
    {851, Camera::lens,     Colour::doppler, Form::walk,          RPT_KERNEL(rpt_render_kernel_lens_doppler_ballot_w5),     RPT_KERNEL(rpt_render_kernel_lens_doppler_ballot_ieee_w5)},
    {853, Camera::lens,     Colour::doppler, Form::walk_first,    RPT_KERNEL(rpt_render_kernel_lens_doppler_ballot_first_w5), RPT_KERNEL(rpt_render_kernel_lens_doppler_ballot_first_ieee_w5)},
    {854, Camera::lens,     Colour::doppler, Form::analytic,      RPT_KERNEL(rpt_render_kernel_lens_doppler_analytic_w8),   nullptr},
    {823, Camera::lens,     Colour::sky,     Form::unculled,      RPT_KERNEL(rpt_render_kernel_lens_env_unculled_w5),       nullptr},
    {861, Camera::lens,     Colour::sky,     Form::walk,          RPT_KERNEL(rpt_render_kernel_lens_env_ballot_w5),         RPT_KERNEL(rpt_render_kernel_lens_env_ballot_ieee_w5)},
    {863, Camera::lens,     Colour::sky,     Form::walk_first,    RPT_KERNEL(rpt_render_kernel_lens_env_ballot_first_w5),   RPT_KERNEL(rpt_render_kernel_lens_env_ballot_first_ieee_w5)},
    {864, Camera::lens,     Colour::sky,     Form::analytic,      RPT_KERNEL(rpt_render_kernel_lens_env_analytic_w8),       nullptr},
    // the ray-map camera (rpt_set_raymap): as the panorama, no band-first form and no forced-IEEE arms; no record form
    {1203, Camera::raymap,  Colour::plain,   Form::unculled,      RPT_KERNEL(rpt_render_kernel_raymap_unculled_w5),         nullptr},
    {1241, Camera::raymap,  Colour::plain,   Form::walk,          RPT_KERNEL(rpt_render_kernel_raymap_walk_w5),             RPT_KERNEL(rpt_render_kernel_raymap_walk_ieee_w5)},
    {1244, Camera::raymap,  Colour::plain,   Form::analytic,      RPT_KERNEL(rpt_render_kernel_raymap_analytic_w8),         nullptr},
    {1213, Camera::raymap,  Colour::doppler, Form::unculled,      RPT_KERNEL(rpt_render_kernel_raymap_doppler_unculled_w5), nullptr},
    {1251, Camera::raymap,  Colour::doppler, Form::walk,          RPT_KERNEL(rpt_render_kernel_raymap_doppler_walk_w5),     RPT_KERNEL(rpt_render_kernel_raymap_doppler_walk_ieee_w5)},
    {1254, Camera::raymap,  Colour::doppler, Form::analytic,      RPT_KERNEL(rpt_render_kernel_raymap_doppler_analytic_w8), nullptr},
    {1223, Camera::raymap,  Colour::sky,     Form::unculled,      RPT_KERNEL(rpt_render_kernel_raymap_env_unculled_w5),     nullptr},
    {1261, Camera::raymap,  Colour::sky,     Form::walk,          RPT_KERNEL(rpt_render_kernel_raymap_env_walk_w5),         RPT_KERNEL(rpt_render_kernel_raymap_env_walk_ieee_w5)},
    {1264, Camera::raymap,  Colour::sky,     Form::analytic,      RPT_KERNEL(rpt_render_kernel_raymap_env_analytic_w8),     nullptr},
};

// The windowed kernels (rpt_set_object_windows): looked up AFTER everything else has chosen a row, by that row's camera (the pinhole's rows
// are served by the lens kernels at lens_scale 1.0f), its colour (plain and Doppler share the twin with the run-time flag) and its form
// (a band-first form gets the walk, a forced-IEEE arm the walk's IEEE kernel).  The variant here is an offset only: what is reported is
// 2000 + the variant of the row of the context's own camera and colour whose form ran.
#define RPT_WINDOWED_ROWS(camera, colour, name)                                                                                                                     \
    {2000, camera, colour, Form::unculled, RPT_KERNEL(rpt_render_kernel_win_##name##_unculled_w5),  nullptr},                                                        \
    {2000, camera, colour, Form::walk,     RPT_KERNEL(rpt_render_kernel_win_##name##_walk_w5),      RPT_KERNEL(rpt_render_kernel_win_##name##_walk_ieee_w5)},        \
    {2000, camera, colour, Form::analytic, RPT_KERNEL(rpt_render_kernel_win_##name##_analytic_w8),  nullptr}
const KernelRow windowed_table[] = {
    RPT_WINDOWED_ROWS(Camera::lens,     Colour::doppler, lens),
    RPT_WINDOWED_ROWS(Camera::lens,     Colour::sky,     lens_env),
    RPT_WINDOWED_ROWS(Camera::equirect, Colour::doppler, pano),
    RPT_WINDOWED_ROWS(Camera::equirect, Colour::sky,     pano_env),
    RPT_WINDOWED_ROWS(Camera::raymap,   Colour::doppler, raymap),
    RPT_WINDOWED_ROWS(Camera::raymap,   Colour::sky,     raymap_env),
    // the pinhole's forced-IEEE arms (48 / 49, 248 / 249; the other cameras and the sky refuse them): the walk's IEEE kernel whatever the scene
    {2000, Camera::lens, Colour::doppler, Form::ieee, RPT_KERNEL(rpt_render_kernel_win_lens_walk_ieee_w5), nullptr},
};
#undef RPT_WINDOWED_ROWS
const KernelRow windowed_events_table[] = {
    {2000, Camera::lens,     Colour::plain, Form::unculled, RPT_KERNEL(rpt_events_kernel_win_lens_unculled),   nullptr},
    {2000, Camera::lens,     Colour::plain, Form::walk,     RPT_KERNEL(rpt_events_kernel_win_lens_walk),       RPT_KERNEL(rpt_events_kernel_win_lens_walk_ieee)},
    {2000, Camera::lens,     Colour::plain, Form::analytic, RPT_KERNEL(rpt_events_kernel_win_lens_analytic),   nullptr},
    {2000, Camera::equirect, Colour::plain, Form::walk,     RPT_KERNEL(rpt_events_kernel_win_pano_walk),       RPT_KERNEL(rpt_events_kernel_win_pano_walk_ieee)},
    {2000, Camera::equirect, Colour::plain, Form::analytic, RPT_KERNEL(rpt_events_kernel_win_pano_analytic),   nullptr},
    {2000, Camera::raymap,   Colour::plain, Form::walk,     RPT_KERNEL(rpt_events_kernel_win_raymap_walk),     RPT_KERNEL(rpt_events_kernel_win_raymap_walk_ieee)},
    {2000, Camera::raymap,   Colour::plain, Form::analytic, RPT_KERNEL(rpt_events_kernel_win_raymap_analytic), nullptr},
};

// The refine kernels (rpt_set_adaptive_aa), variant 1000 + 10 (3 camera + colour) + {1 walk, 3 un-culled, 4 no walk}.  The form is pass
// A's: un-culled wherever the one-sample kernel ran un-culled, the walk with the wave's object mask, or no walk compiled in.
#define RPT_REFINE_ROWS(base, camera, colour, name)                                                                                                 \
    {base + 3, camera, colour, Form::unculled, RPT_KERNEL(rpt_refine_kernel_##name##_unculled), nullptr},                                          \
    {base + 1, camera, colour, Form::walk,     RPT_KERNEL(rpt_refine_kernel_##name##_walk),     RPT_KERNEL(rpt_refine_kernel_##name##_walk_ieee)}, \
    {base + 4, camera, colour, Form::analytic, RPT_KERNEL(rpt_refine_kernel_##name##_analytic), nullptr}
const KernelRow refine_table[] = {
    RPT_REFINE_ROWS(1000, Camera::pinhole,  Colour::plain,   plain),
    RPT_REFINE_ROWS(1010, Camera::pinhole,  Colour::doppler, doppler),
    RPT_REFINE_ROWS(1020, Camera::pinhole,  Colour::sky,     env),
    RPT_REFINE_ROWS(1030, Camera::lens,     Colour::plain,   lens),
    RPT_REFINE_ROWS(1040, Camera::lens,     Colour::doppler, lens_doppler),
    RPT_REFINE_ROWS(1050, Camera::lens,     Colour::sky,     lens_env),
    RPT_REFINE_ROWS(1060, Camera::equirect, Colour::plain,   pano),
    RPT_REFINE_ROWS(1070, Camera::equirect, Colour::doppler, pano_doppler),
    RPT_REFINE_ROWS(1080, Camera::equirect, Colour::sky,     pano_env),
};
#undef RPT_REFINE_ROWS

// The event kernels (rpt_render_events): colour does not exist there.  Un-culled is rpt_set_variant(3) and what a frame outside the proven
// window gets; the panorama has no un-culled row: it has no object mask and the pass has no shadow rays, so its two rows cull nothing.
const KernelRow events_table[] = {
    {903, Camera::pinhole,  Colour::plain, Form::unculled, RPT_KERNEL(rpt_events_kernel_unculled),      nullptr},
    {941, Camera::pinhole,  Colour::plain, Form::walk,     RPT_KERNEL(rpt_events_kernel_ballot),        RPT_KERNEL(rpt_events_kernel_ballot_ieee)},
    {944, Camera::pinhole,  Colour::plain, Form::analytic, RPT_KERNEL(rpt_events_kernel_analytic),      nullptr},
    {911, Camera::equirect, Colour::plain, Form::walk,     RPT_KERNEL(rpt_events_kernel_pano),          RPT_KERNEL(rpt_events_kernel_pano_ieee)},
    {914, Camera::equirect, Colour::plain, Form::analytic, RPT_KERNEL(rpt_events_kernel_pano_analytic), nullptr},
    {923, Camera::lens,     Colour::plain, Form::unculled, RPT_KERNEL(rpt_events_kernel_lens_unculled), nullptr},
    {921, Camera::lens,     Colour::plain, Form::walk,     RPT_KERNEL(rpt_events_kernel_lens_ballot),   RPT_KERNEL(rpt_events_kernel_lens_ballot_ieee)},
    {924, Camera::lens,     Colour::plain, Form::analytic, RPT_KERNEL(rpt_events_kernel_lens_analytic), nullptr},
    {1291, Camera::raymap,  Colour::plain, Form::walk,     RPT_KERNEL(rpt_events_kernel_raymap),        RPT_KERNEL(rpt_events_kernel_raymap_ieee)},
    {1294, Camera::raymap,  Colour::plain, Form::analytic, RPT_KERNEL(rpt_events_kernel_raymap_analytic), nullptr},
};
#undef RPT_KERNEL

template <size_t N>
const KernelRow *find_row(const KernelRow (&table)[N], Camera camera, Colour colour, Form form) {
    for (const KernelRow &r : table)
        if (r.camera == camera && r.colour == colour && r.form == form) return &r;
    return nullptr;
}

// the form rpt_set_variant(v) asks for; Form::diagnostic: not a number the product library takes
Form settable_form(int v) {
    for (const KernelRow &r : colour_table)
        if (r.variant == v && r.camera == Camera::pinhole && r.colour == Colour::plain && settable(r.form)) return r.form;
    return Form::diagnostic;
}

// ---- the rules over the settings that more than one choice follows -------------------------------------------------------------------
// The variants that exist for every camera and colour, as refine kernels and as event kernels: 0 and the forms it can resolve to
bool has_product_forms(int variant) { return variant == 0 || variant == 3 || variant == 41 || variant == 43 || variant == 44; }

// The per-object regions are PROVEN for the window |u| <= 2, |v| <= 1/2 (rpt_bounds_certify.hpp): a frame wider than 4 : 1 has pixels
// outside it, and beyond 2^20 pixels a side a tile's 1.5-pixel skirt is no longer large against float rounding — such frames are rendered
// un-culled (same pixels, every object tested everywhere).
// Under a lens pixel (x, y) looks through (fl(s fx2), fl(s fy2)): with s <= 1 no larger in magnitude than |fy2| <= 1/2 and than
// fl(s fl(aspect / 2)), which is what is compared here (rounding is monotone).  The 2^20 bound covers every s: the skirt and the rounding
// it is held against scale with s alike (rpt_kernels.hip.h: wave_object_mask_lens).  A wider lens: un-culled as well.
bool window_holds_frame(const rpt_ctx *ctx) {
    const float half_aspect = 0.5f * ((float)ctx->width / (float)ctx->height);
    const bool lens = ctx->v_fov != 0.0f;
    return (lens ? ctx->lens_scale <= 1.0f && ctx->lens_scale * half_aspect <= (float)rptb::cert::WINDOW_U : half_aspect <= (float)rptb::cert::WINDOW_U) &&
           ctx->width <= (1 << 20) && ctx->height <= (1 << 20);
}

// Frames in flight that are too small to fill the chip with walks wait for latency as the blocking call does
// (profiles/r03_latency_walk_ab.txt: 43 ahead of 41 up to 1920x1080 — bunny -6 %, shadows -19 % — level at 2560x1440, behind from
// 3200x1800).  A rank's share of a sharded frame counts, not the frame.
bool small_frame(const rpt_ctx *ctx) {
    return (size_t)local_tile_count(ctx) * RPT_TILE_ROWS * (size_t)ctx->width <= (size_t)RPT_LATENCY_KERNEL_MAX_PIXELS;
}

// The ray-map camera (rpt_set_projection with RPT_PROJECTION_RAYMAP): what a launch needs of the map; "" = nothing is missing
std::string raymap_missing(const rpt_ctx *ctx) {
    if (!ctx->raymap_on) return "rpt_set_raymap: RPT_PROJECTION_RAYMAP is set but the context has no ray map";
    if (ctx->raymap_width != ctx->width || ctx->raymap_height != ctx->height)
        return "rpt_set_raymap: the map is " + std::to_string(ctx->raymap_width) + " x " + std::to_string(ctx->raymap_height) + ", the frame " +
               std::to_string(ctx->width) + " x " + std::to_string(ctx->height);
    return "";
}

// the Doppler debug kernel stands in for every twin while the record hook is set (rpt_set_debug_doppler)
bool doppler_recording(const rpt_ctx *ctx) { return ctx->doppler && (ctx->external_doppler || ctx->want_owned_doppler); }

// ---- the choice: everything a launch decides, from the settings alone ----------------------------------------------------------------
// colour_frame: the launch renders a frame of rpt_render / rpt_render_async, which is what rpt_set_adaptive_aa acts on (pass A + pass B);
// rpt_verify_frame and rpt_timed_frames launch the one-sample pass alone, in flight.
enum class CallKind { blocking, in_flight, events };
struct Call {
    CallKind kind;
    bool colour_frame;
};
struct Choice {
    int code = RPT_OK;                  // != RPT_OK: the refusal, with its text
    std::string text;
    bool nothing = false;               // this context holds no row of the frame (rpt_set_rows): nothing to launch, nothing refused
    const KernelRow *colour = nullptr;  // the colour kernel (the event kernel of an event pass); null with `variant` set: a measurement arm
    const KernelRow *refine = nullptr;  // pass B of an adaptive frame, or null
    int variant = 0;                    // colour->variant, or the measurement arm's number (librpt_hip_diag.so)
    bool exact_rcp = false;             // the scene lies in rcp_exact's domain: a row that has an `ieee` sibling runs its own kernel
    bool band_first = false;            // the band of tile rows that holds the meshes goes first
    const KernelRow *windowed = nullptr;// rpt_set_object_windows: the row that is launched in `colour`'s place (`variant` is 2000 + the row's it stands for)
    const void *kernel(const KernelRow *row) const { return row->ieee && !exact_rcp ? row->ieee : row->kernel; }
    bool ran_exact(const KernelRow *row) const { return row && row->ieee && exact_rcp; }
    const KernelRow *launched() const { return windowed ? windowed : colour; }
};

Choice refuse(int code, std::string text) {
    Choice c;
    c.code = code;
    c.text = std::move(text);
    return c;
}

// rpt_set_object_windows: "" = the windows fit this launch's Object[]
std::string windows_mismatch(const rpt_ctx *ctx) {
    if (ctx->windows.size() == 2 * (size_t)ctx->object_count) return "";
    return "rpt_set_object_windows: " + std::to_string(ctx->windows.size() / 2) + " windows are set, the Object[] holds " + std::to_string(ctx->object_count);
}

Choice choose_event_kernel(const rpt_ctx *ctx) {
    if (!ctx->scene_uploaded) return refuse(RPT_ERR_STATE, "rpt_render_events before rpt_upload_scene");
    if (!ctx->params_set) return refuse(RPT_ERR_STATE, "rpt_render_events before rpt_set_params");
    if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_render_events: MSAA > 1 has no event kernel (one primary ray per pixel)");
    if (!has_product_forms(ctx->variant))
        return refuse(RPT_ERR_ARG, "rpt_render_events: variant " + std::to_string(ctx->variant) + " has no event kernel (variants 0, 3, 41, 43 and 44 have)");
    const bool panorama = ctx->projection == RPT_PROJECTION_EQUIRECT, raymap = ctx->projection == RPT_PROJECTION_RAYMAP, lens = ctx->v_fov != 0.0f;
    if (lens && panorama) return refuse(RPT_ERR_ARG, "rpt_render_events: the panorama has fields of view of its own (rpt_set_projection); a lens needs the pinhole");
    if (lens && raymap) return refuse(RPT_ERR_ARG, "rpt_render_events: the ray map has a field of view of its own (rpt_set_raymap); a lens needs the pinhole");
    if (raymap) {
        const std::string missing = raymap_missing(ctx);
        if (!missing.empty()) return refuse(RPT_ERR_ARG, missing);
    }
    const Camera camera = panorama ? Camera::equirect : (raymap ? Camera::raymap : (lens ? Camera::lens : Camera::pinhole));
    Form form = !ctx->has_mesh ? Form::analytic : Form::walk;
    if (camera != Camera::equirect && camera != Camera::raymap && (ctx->variant == 3 || !window_holds_frame(ctx))) form = Form::unculled;
    if (!ctx->geo->compact_ok && form != Form::analytic)
        return refuse(RPT_ERR_ARG, "rpt_render_events: the event kernels need the derived octree layout, which this scene's octree does not fit (children not consecutive)");
    Choice c;
    c.colour = find_row(events_table, camera, Colour::plain, form);
    if (!c.colour) return refuse(RPT_ERR_ARG, "rpt_render_events: no event kernel for this camera");
    c.variant = c.colour->variant;
    c.exact_rcp = ctx->geo->exact_rcp_ok;
    if (!ctx->windows.empty()) {       // the windowed form of the same row (the pinhole's: the lens kernel, lens_scale 1.0f)
        const std::string mismatch = windows_mismatch(ctx);
        if (!mismatch.empty()) return refuse(RPT_ERR_ARG, mismatch);
        c.windowed = find_row(windowed_events_table, camera == Camera::pinhole ? Camera::lens : camera, Colour::plain, form);
        if (!c.windowed) return refuse(RPT_ERR_ARG, "rpt_set_object_windows: no windowed event kernel for this camera");
        c.variant = 2000 + c.colour->variant;
    }
    return c;
}

// Calls nothing in HIP and changes nothing in the context.  Where several refusals apply, the first one here is what the caller sees.
Choice choose_kernels(const rpt_ctx *ctx, Call call) {
    if (call.kind == CallKind::events) return choose_event_kernel(ctx);
    if (!ctx->scene_uploaded) return refuse(RPT_ERR_STATE, "rpt_render before rpt_upload_scene");
    if (!ctx->params_set) return refuse(RPT_ERR_STATE, "rpt_render before rpt_set_params");
    const int sv = ctx->variant;
    const bool lens = ctx->v_fov != 0.0f, panorama = ctx->projection == RPT_PROJECTION_EQUIRECT, raymap = ctx->projection == RPT_PROJECTION_RAYMAP, recording = doppler_recording(ctx);
    // Adaptive anti-aliasing (rpt_set_adaptive_aa): what it cannot serve refuses first
    const bool adaptive = call.colour_frame && ctx->aa_n > 1;
    if (adaptive) {
        if (raymap) return refuse(RPT_ERR_ARG, "rpt_set_adaptive_aa: the ray-map camera (rpt_set_raymap) has no refine pass: a map holds one direction per pixel, none between them");
        if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_set_adaptive_aa: rpt_set_msaa > 1 is set as well (full supersampling is threshold -1 here)");
        if (ctx->first_tile != 0 || ctx->tile_step != 1 || ctx->run_log2 != 0 || ctx->colour_plane)
            return refuse(RPT_ERR_ARG, "rpt_set_adaptive_aa: this context renders a share of the frame's rows or a colour plane (rpt_set_rows / rpt_set_tile_pattern): the neighbour rows belong to another rank");
        if (!has_product_forms(sv))
            return refuse(RPT_ERR_ARG, "rpt_set_adaptive_aa: variant " + std::to_string(sv) + " has no refine kernel (variants 0, 3, 41, 43 and 44 have)");
        if (recording) return refuse(RPT_ERR_ARG, "rpt_set_adaptive_aa: the Doppler debug kernels (rpt_set_debug_doppler) have no refine pass");
        if (!ctx->geo->compact_ok && ctx->has_mesh)
            return refuse(RPT_ERR_ARG, "rpt_set_adaptive_aa: the refine kernels need the derived octree layout, which this scene's octree does not fit (children not consecutive)");
    }
    Choice c;
    c.exact_rcp = ctx->geo->exact_rcp_ok;
    if (local_tile_count(ctx) == 0) {
        c.nothing = true;
        return c;
    }
    // The form.  Variant 0 = default: rpt_render_async() is a throughput call (frames in flight fill each other's gaps): the in-wave cull
    // kernel in natural order (41).  The blocking rpt_render() is a latency call — its caller waits for this frame, and the frame is as
    // long as its longest wave — so the band of tile rows that holds the meshes is dispatched first and the walk asks for its triangle
    // records an iteration ahead (43); small frames in flight likewise.  A frame whose Object[] holds no mesh gets the kernel without the
    // octree walk (44): 8 waves per SIMD instead of 5.  An octree the derived layout cannot hold gets the general kernel (1).
    // Kernels 41 and 43 take the triangle test's 1 / det through rcp_exact when the scene's triangles allow it and the IEEE division
    // otherwise (KernelRow::ieee); rpt_last_variant reports 41 / 43 either way, rpt_last_exact_rcp which ran.
    c.variant = sv;
    Form form = sv == 0 ? (!ctx->has_mesh ? Form::analytic : (call.kind == CallKind::blocking || small_frame(ctx) ? Form::walk_first : Form::walk)) : settable_form(sv);
    if (form == Form::analytic && ctx->has_mesh) form = Form::walk;          // (asked for explicitly on a scene with meshes: the full kernel)
    if (!ctx->geo->compact_ok && form != Form::analytic) form = Form::ref_layout;
    // A lens (rpt_set_field_of_view), the panorama (rpt_set_projection), MSAA, Doppler and the sky: what has no kernel refuses here, at
    // the launch, so that the settings may be made in any order
    if (lens) {
        if (panorama) return refuse(RPT_ERR_ARG, "rpt_set_field_of_view: the panorama has fields of view of its own (rpt_set_projection); a lens needs the pinhole");
        if (raymap) return refuse(RPT_ERR_ARG, "rpt_set_field_of_view: the ray map has a field of view of its own (rpt_set_raymap); a lens needs the pinhole");
        if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_set_field_of_view: MSAA > 1 has no lens kernel");
        if (!has_product_forms(sv))
            return refuse(RPT_ERR_ARG, "rpt_set_field_of_view: variant " + std::to_string(sv) + " has no lens kernel (variants 0, 3, 41, 43 and 44 have)");
        if (form == Form::ref_layout)
            return refuse(RPT_ERR_ARG, "rpt_set_field_of_view: the lens kernels need the derived octree layout, which this scene's octree does not fit (children not consecutive)");
        if (recording) return refuse(RPT_ERR_ARG, "rpt_set_field_of_view: the Doppler debug kernel (rpt_set_debug_doppler) has no lens form");
    }
    Camera camera = Camera::pinhole;
    if (panorama) {      // variant 0's choice and variant 3 only; its rays leave the pinhole's proven window anyway
        if (sv != 0 && sv != 3) return refuse(RPT_ERR_ARG, "rpt_set_projection: variant " + std::to_string(sv) + " has no panorama kernel (variants 0 and 3 have)");
        if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_set_projection: MSAA > 1 has no panorama kernel");
        if (form == Form::walk_first) form = Form::walk;
        camera = Camera::equirect;
        if (!find_row(colour_table, camera, Colour::plain, form))
            return refuse(RPT_ERR_ARG, "rpt_set_projection: the panorama kernels need the derived octree layout, which this scene's octree does not fit (children not consecutive)");
    } else if (raymap) {  // variant 0's choice, the forms it can resolve to, and variant 3; nothing of the pinhole's window applies
        const std::string missing = raymap_missing(ctx);
        if (!missing.empty()) return refuse(RPT_ERR_ARG, missing);
        if (!has_product_forms(sv))
            return refuse(RPT_ERR_ARG, "rpt_set_raymap: variant " + std::to_string(sv) + " has no ray-map kernel (variants 0, 3, 41, 43 and 44 have)");
        if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_set_raymap: MSAA > 1 has no ray-map kernel");
        if (recording) return refuse(RPT_ERR_ARG, "rpt_set_raymap: the Doppler debug kernel (rpt_set_debug_doppler) has no ray-map form");
        if (form == Form::walk_first) form = Form::walk;
        camera = Camera::raymap;
        if (!find_row(colour_table, camera, Colour::plain, form))
            return refuse(RPT_ERR_ARG, "rpt_set_raymap: the ray-map kernels need the derived octree layout, which this scene's octree does not fit (children not consecutive)");
    } else if (needs_proven_window(form) && !window_holds_frame(ctx)) {
        form = Form::unculled;
    }
    // (pass B's form is pass A's at this point: un-culled, without the walk, else the walk)
    const Form refine_form = form == Form::unculled || form == Form::analytic ? form : Form::walk;
    c.band_first = band_first(form);
    if (ctx->msaa > 1) {       // MSAASAMPLES > 1: the multi-sample form of the default kernel (46), or of the un-culled one (47)
        form = form == Form::unculled ? Form::msaa_unculled : (form == Form::walk || form == Form::walk_first || form == Form::analytic ? Form::msaa : Form::diagnostic);
        if (!find_row(colour_table, camera, Colour::plain, form))
            return refuse(RPT_ERR_ARG, "rpt_set_msaa > 1 is implemented for the default kernels and variant 3 (derived octree layouts)");
    }
    Colour colour = Colour::plain;
    if (ctx->env_on) {         // looked up before Doppler: a sky kernel carries Doppler as a run-time flag and serves both
        if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_set_environment: MSAA > 1 has no environment kernel");
        if (recording) return refuse(RPT_ERR_ARG, "rpt_set_environment: the Doppler debug kernels (rpt_set_debug_doppler) have no environment form");
        colour = Colour::sky;
        if (!find_row(colour_table, camera, colour, form))
            return refuse(RPT_ERR_ARG, form == Form::ref_layout && sv != 1
                                           ? "rpt_set_environment: the environment kernels need the derived octree layout, which this scene's octree does not fit (children not consecutive)"
                                           : "rpt_set_environment: variant " + std::to_string(sv) + " has no environment kernel (variants 0, 3, 41, 43 and 44 have)");
    } else if (ctx->doppler) {
        if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_set_doppler: MSAA > 1 has no Doppler kernel");
        colour = Colour::doppler;
        if (!find_row(colour_table, camera, colour, form))
            return refuse(RPT_ERR_ARG, form == Form::ref_layout ? "rpt_set_doppler: kernel 1 (the reference's octree layout) has no Doppler twin"
                                                                : "rpt_set_doppler: this kernel variant has no Doppler twin");
        if (recording) form = Form::record;
    }
    if (lens) camera = Camera::lens;         // last: the lens form of what every other setting chose
    c.colour = find_row(colour_table, camera, colour, form);
    if (c.colour) c.variant = c.colour->variant;
#ifndef RPT_DIAGNOSTICS
    if (!c.colour) return refuse(RPT_ERR_ARG, "unknown kernel variant");
#endif
    if (!ctx->windows.empty()) {
        // Time windows (rpt_set_object_windows): the windowed form of the row everything above chose.  What has none refuses here.
        if (adaptive) return refuse(RPT_ERR_ARG, "rpt_set_object_windows: adaptive anti-aliasing (rpt_set_adaptive_aa) has no windowed refine pass");
        if (ctx->msaa > 1) return refuse(RPT_ERR_ARG, "rpt_set_object_windows: MSAA > 1 has no windowed kernel");
        if (recording) return refuse(RPT_ERR_ARG, "rpt_set_object_windows: the Doppler debug kernels (rpt_set_debug_doppler) have no windowed form");
#ifdef RPT_DIAGNOSTICS
        if (!c.colour) return refuse(RPT_ERR_ARG, "rpt_set_object_windows: the measurement arms have no windowed form");
#endif
        if (form == Form::ref_layout || form == Form::relaxed5 || form == Form::relaxed6)
            return refuse(RPT_ERR_ARG, sv == 1 || sv == 50 || sv == 51 ? "rpt_set_object_windows: variant " + std::to_string(sv) + " has no windowed kernel"
                                                                      : "rpt_set_object_windows: the windowed kernels need the derived octree layout, which this scene's octree does not fit (children not consecutive)");
        const std::string mismatch = windows_mismatch(ctx);
        if (!mismatch.empty()) return refuse(RPT_ERR_ARG, mismatch);
        const Form wform = form == Form::walk_first ? Form::walk : (form == Form::ieee_first ? Form::ieee : form);      // (no band-first form: the walk)
        const Camera own = camera;
        c.windowed = find_row(windowed_table, own == Camera::pinhole ? Camera::lens : own, colour == Colour::sky ? Colour::sky : Colour::doppler, wform);
        const KernelRow *stands_for = find_row(colour_table, own, colour, wform);
        if (!c.windowed || !stands_for) return refuse(RPT_ERR_ARG, "rpt_set_object_windows: this kernel variant has no windowed form");
        c.variant = 2000 + stands_for->variant;
        c.band_first = false;
    }
    if (adaptive) {
        // under a lens the skirt's proof for the SAMPLE positions reaches 0.98 million pixels a side, not 2^20 (rpt_kernels.hip.h: refine_pixel_body)
        const bool beyond_samples = lens && (ctx->width > (1 << 19) || ctx->height > (1 << 19));
        c.refine = find_row(refine_table, camera, colour, beyond_samples ? Form::unculled : refine_form);
        if (!c.refine) return refuse(RPT_ERR_ARG, "rpt_set_adaptive_aa: no refine kernel for this camera");
    }
    return c;
}

// The diagonal slabs hold inside their window only (rpt_screen_bounds.hpp): frames up to 4 : 1, |v| <= 1/2 always.  Under a lens
// (rpt_set_field_of_view) the tiles' plane coordinates are those of the reference's lens times s <= 1 — a wider lens gets the un-culled
// kernel — so the same rule holds with both sides of the tile scaled.
bool frame_inside_diagonal_window(const rpt_ctx *ctx) {
    const bool lens = ctx->v_fov != 0.0f;
    const float aspect = (float)ctx->width / (float)ctx->height, s = lens ? ctx->lens_scale : 1.0f;
    const float diag_reach = 0.5f * aspect + 2.0f * (1.0f / (float)ctx->height) * aspect;
    return lens ? s <= 1.0f && s * diag_reach <= (float)rptb::DIAG_WINDOW_U : diag_reach <= (float)rptb::DIAG_WINDOW_U;
}

// do the bitmaps on the device belong to this frame?  (its size, its lens, its objects)
bool tile_bits_current(const rpt_ctx *ctx) {
    const int slots = ctx->object_count < 64 ? ctx->object_count : 64;
    return ctx->bits_width == ctx->width && ctx->bits_height == ctx->height && ctx->bits_slots == slots &&
           ctx->bits_lens == (ctx->v_fov != 0.0f ? ctx->lens_scale : 1.0f) && ctx->bits_diagonals == frame_inside_diagonal_window(ctx);
}

// The tile bitmap of one mesh object for this frame, into `bits`; false: this object gets none (not a mesh with sub-tree boxes, or
// outside the rule 16.2 K + 3.2u <= 0.25 that DObj::mslope >= 0 stands for, or a box's region could not be proven)
// stage: 0 the sub-tree stage alone, 1 the triangle stage alone, -1 the product a context puts on the device — the sub-tree stage ANDed
// with the triangle stage where that one yields a bitmap (and the context has not switched it off).  stats: those of the stage asked
// for; of the sub-tree stage for the product.
bool build_tile_bitmap(const rpt_ctx *ctx, const rpt_object &o, uint32_t *bits, rptb::tiles::Stats *stats, int stage = -1) {
    if (o.type != RPT_MESH) return false;
    const auto it = ctx->geo->mesh_boxes.find(o.meshIndex);
    if (it == ctx->geo->mesh_boxes.end() || it->second.empty() || (size_t)o.meshIndex >= ctx->geo->node_tri_K.size()) return false;
    rptd::DObj d;
    build_dobjs(ctx, &o, 1, &d);
    if (!(d.mslope >= 0.0f)) return false;
    const double slope = 16.2 * (double)ctx->geo->node_tri_K[(size_t)o.meshIndex] + 3.2 * rptb::cert::U24, L = (double)ctx->geo->node_tri_L[(size_t)o.meshIndex];
    const rptb::tiles::Frame f{ctx->width, ctx->height, ctx->v_fov != 0.0f ? ctx->lens_scale : 1.0f, frame_inside_diagonal_window(ctx)};
    const auto tri = ctx->geo->mesh_tri_boxes.find(o.meshIndex);
    const bool has_tri = tri != ctx->geo->mesh_tri_boxes.end() && !tri->second.empty();
    if (stage == 1) return has_tri && rptb::tiles::build_pooled(o, ctx->interval, tri->second.data(), (int)(tri->second.size() / 6), slope, L, f, bits, stats);
    if (!rptb::tiles::build(o, ctx->interval, it->second.data(), (int)(it->second.size() / 6), slope, L, f, bits, stats)) return false;
    if (stage == 0 || !ctx->tile_triangles || !has_tri) return true;
    const size_t words = rptb::tiles::bitmap_words(ctx->width, ctx->height);
    std::vector<uint32_t> fine(words);
    if (rptb::tiles::build_pooled(o, ctx->interval, tri->second.data(), (int)(tri->second.size() / 6), slope, L, f, fine.data(), nullptr))
        for (size_t k = 0; k < words; k++) bits[k] &= fine[k];
    return true;
}

// RPT_TILE_TRIANGLES=0 (read when a context is created): the sub-tree stage alone, for the A/B and as an escape hatch
bool tile_triangles_wanted() {
    const char *e = std::getenv("RPT_TILE_TRIANGLES");
    return !(e && e[0] == '0' && e[1] == 0);
}

// build_tile_bitmap's product through the geometry's cache: the contexts of one scene build a bitmap once
bool shared_tile_bitmap(const rpt_ctx *ctx, const rpt_object &o, uint32_t *bits) {
    if (o.type != RPT_MESH) return false;        // (ensure_tile_bits asks for every still object when no bitmap is live: only meshes take a place in the cache)
    Geometry &g = *ctx->geo;
    const size_t words = rptb::tiles::bitmap_words(ctx->width, ctx->height);
    const float lens = ctx->v_fov != 0.0f ? ctx->lens_scale : 1.0f;
    const bool diagonals = frame_inside_diagonal_window(ctx);
    std::lock_guard<std::mutex> lock(g.bitmap_cache_lock);
    for (const Geometry::BitmapEntry &e : g.bitmap_cache) {
        if (e.interval != ctx->interval || e.width != ctx->width || e.height != ctx->height || e.lens != lens || e.diagonals != diagonals ||
            e.triangles != ctx->tile_triangles || std::memcmp(e.object, &o, sizeof(rpt_object)) != 0)
            continue;
        if (e.built) std::memcpy(bits, e.bits.data(), words * 4);
        g.bitmap_copies++;
        return e.built;
    }
    g.bitmap_builds++;
    const bool room = g.bitmap_cache.size() < Geometry::BITMAP_CACHE_ENTRIES;
    if (room) g.bitmap_cache.emplace_back();
    Geometry::BitmapEntry &e = room ? g.bitmap_cache.back() : g.bitmap_cache[g.bitmap_cache_next++ % Geometry::BITMAP_CACHE_ENTRIES];
    std::memcpy(e.object, &o, sizeof(rpt_object));
    e.interval = ctx->interval; e.width = ctx->width; e.height = ctx->height; e.lens = lens; e.diagonals = diagonals; e.triangles = ctx->tile_triangles;
    e.built = build_tile_bitmap(ctx, o, bits, nullptr);
    if (e.built) e.bits.assign(bits, bits + words);
    else e.bits.clear();
    return e.built;
}

// Before a colour frame's launch: every still mesh that has no bitmap for this frame yet gets one (or is marked as tried), behind
// everything enqueued so far — a frame in flight reads what it was launched with.  Here and not in rpt_set_objects because the bitmap
// also depends on the frame's size and lens, which may be set after the objects.  Frames the culled kernels refuse (beyond 4 : 1,
// beyond 2^20 pixels a side, a wide lens), the panorama, variant 3 and MSAA get none.
int ensure_tile_bits(rpt_ctx *ctx) {
    if (ctx->projection != RPT_PROJECTION_PINHOLE || ctx->variant == 3 || ctx->msaa > 1 || !ctx->geo->compact_ok || !ctx->has_mesh || !window_holds_frame(ctx) ||
        ctx->host_objects.size() != (size_t)ctx->object_count * sizeof(rpt_object))
        return RPT_OK;
    const int slots = ctx->object_count < 64 ? ctx->object_count : 64;
    if (!tile_bits_current(ctx)) {
        ctx->bits_has = ctx->bits_tried = 0;
        ctx->bits_width = ctx->width; ctx->bits_height = ctx->height; ctx->bits_slots = slots;
        ctx->bits_lens = ctx->v_fov != 0.0f ? ctx->lens_scale : 1.0f;
        ctx->bits_diagonals = frame_inside_diagonal_window(ctx);
    }
    const rpt_object *objs = (const rpt_object *)ctx->host_objects.data();
    unsigned long long todo = 0;
    for (int i = 0; i < slots; i++)
        if (((ctx->bits_still & ~ctx->bits_tried) >> i & 1ull) && objs[i].type == RPT_MESH) todo |= 1ull << i;
    ctx->bits_tried |= ctx->bits_still;
    if (!todo) return RPT_OK;
    const size_t words = rptb::tiles::bitmap_words(ctx->width, ctx->height), bytes = (size_t)slots * words * 4;
    if (bytes > ctx->tile_bits.host_capacity) ctx->bits_has = 0;      // (the pinned copy is replaced: the others' bitmaps go with it)
    if (ctx->bits_has == 0) todo = ctx->bits_still;
    void *host = nullptr;
    if (int rc = staged_host(ctx, ctx->tile_bits, bytes, &host)) return rc;
    bool any = false;
    for (int i = 0; i < slots; i++) {
        if (!(todo >> i & 1ull)) continue;
        const auto t0 = std::chrono::steady_clock::now();
        if (!shared_tile_bitmap(ctx, objs[i], (uint32_t *)host + (size_t)i * words)) continue;
        ctx->bits_last_build_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
        ctx->bits_has |= 1ull << i;
        ctx->bits_builds++;
        any = true;
    }
    if (any) return staged_copy(ctx, ctx->tile_bits);
    return RPT_OK;
}

// What every frame's arguments hold whatever kernel renders it: the scene, the outputs, the per-frame constants, the rows and the camera
// (launch() adds the colour, launch_events() the records).  One LensArgs serves every kernel: each reads its own prefix of it.
void fill_frame_args(const rpt_ctx *ctx, rptd::LensArgs &a) {
    std::memset((void *)&a, 0, sizeof a);
    a.dnodes = (const rptd::DNode *)ctx->geo->dnodes.ptr;
    a.dtris = (const rptd::DTri *)ctx->geo->dtris.ptr;
    a.links = (const int *)ctx->geo->dlinks.ptr;
    a.first_tris = (const rptd::DTri *)ctx->geo->dfirst.ptr;
    a.exits = (const rptd::DExit *)ctx->geo->dexits.ptr;
    a.hits = (const rptd::DHit *)ctx->geo->dhits.ptr;
    a.top_count = ctx->geo->top_count;
    a.dobjs = (const rptd::DObj *)((const char *)ctx->objects.ptr + (size_t)ctx->object_count * sizeof(rpt_object));
    a.objects = (const rpt_object *)ctx->objects.ptr;
    a.rects = (const float4 *)((const char *)ctx->objects.ptr + (size_t)ctx->object_count * (sizeof(rpt_object) + sizeof(rptd::DObj)));
    a.vertices = (const rpt_float3 *)ctx->geo->vertices.ptr;
    a.normals = (const rpt_float3 *)ctx->geo->normals.ptr;
    a.uvs = (const rpt_float2 *)ctx->geo->uvs.ptr;
    a.triangles = (const uint32_t *)ctx->geo->triangles.ptr;
    a.octrees = (const rpt_octree *)ctx->geo->octrees.ptr;
    a.octreeTris = (const int32_t *)ctx->geo->octreeTris.ptr;
    a.textures = (const uint8_t *)ctx->geo->textures.ptr;
    a.texture_bytes = (long long)ctx->geo->textures.bytes;
    a.out16 = ctx->colour_plane ? nullptr : (rpt_pixel *)(ctx->external_out ? ctx->external_out : ctx->owned_out.ptr);
    a.plane = ctx->colour_plane ? (uint32_t *)(ctx->external_plane ? ctx->external_plane : ctx->owned_plane.ptr) : nullptr;
    a.debug_rgb = (float *)(ctx->external_rgb ? ctx->external_rgb : (ctx->want_owned_rgb ? ctx->owned_rgb.ptr : nullptr));
    for (int c = 0; c < 3; c++) a.hable_wp[c] = hable_host(ctx->white_point[c]);
    {   // background colour of opencl_kernel.cl:565 through the tonemap and pack of :649-657, once per frame
        const float bg[3] = {0.15f, 0.15f, 0.25f};
        uint32_t packed = 1u << 24;
        for (int c = 0; c < 3; c++) {
            const float m = hable_host(bg[c]) / a.hable_wp[c];
            a.bg_mapped[c] = 1.0f < m ? 1.0f : m;
            packed |= to_u8_host(a.bg_mapped[c]) << (8 * c);
        }
        a.bg_packed = packed;
    }
    a.ambient = ctx->ambient;
    a.aspect = (float)ctx->width / (float)ctx->height;
    a.inv_width = 1.0f / (float)ctx->width;
    a.inv_height = 1.0f / (float)ctx->height;
    a.diagonals = 0;
    const bool lens = ctx->v_fov != 0.0f;
    a.lens_scale = lens ? ctx->lens_scale : 1.0f;
    if (frame_inside_diagonal_window(ctx) && ctx->rects.size() == (size_t)ctx->object_count)
        for (const rptb::Rect &r : ctx->rects) a.diagonals |= rptb::has_diagonals(r) ? 1 : 0;
    // the tile bitmaps of the still meshes (ensure_tile_bits; the kernels of render_pixel_body that take the wave's object mask read them)
    if (ctx->bits_has && ctx->tile_bits.device.ptr && tile_bits_current(ctx)) {
        a.tile_bits = (const uint32_t *)ctx->tile_bits.device.ptr;
        a.tile_bits_objects = ctx->bits_has;
    }
    a.object_count = ctx->object_count;
    a.width = ctx->width;
    a.height = ctx->height;
    a.interval = ctx->interval;
    a.first_tile = ctx->first_tile;
    a.tile_step = ctx->tile_step;
    a.run_log2 = ctx->run_log2;
    if (ctx->projection == RPT_PROJECTION_EQUIRECT) {     // (the caller has made them this frame's: ensure_projection_tables)
        a.pano_cols = (const float2 *)ctx->pano.upload.device.ptr;
        a.pano_rows = a.pano_cols + ctx->width;
    }
}

// ---- the sky split (rpt_sky_split.hpp; rpt_kernels.hip.h: rpt_sky_fill_kernel) --------------------------------------
// A plain pinhole colour frame whose objects' regions lie in a box of tiles that is a small share of the frame is launched as two
// kernels: rpt_sky_fill_kernel writes every pixel outside the box, the frame's own kernel runs over the box alone.  The sky's waves then
// hold a dozen registers for their microsecond, not the 96 of a walk kernel, and fit next to the walkers of the frames in flight.
// The rule — everything else gets the single launch:
//   * a frame in flight (rpt_render_async, rpt_timed_frames) of more than RPT_SKY_SPLIT_MIN_PIXELS pixels: the throughput case, where
//     the fill runs beside the walkers of the other frames.  On one stream the frame's own kernel starts when the fill has ended, so
//     a frame its caller waits for gets longer by the fill, and so does a frame too small to keep the chip full of walks: the blocking
//     rpt_render lost 5 % at 4K; in flight, bunny.txt lost 5 % at 1080p and 3 % at 2560x1440, was level at 3200x1800 (5.8 Mpx) and
//     gained 7 % at 3840x2160 (8.3 Mpx) (§6.2d).  RPT_SKY_SPLIT_MIN_PIXELS=<n> in the environment, read when a context is created, sets
//     another floor (frames of MORE than n pixels split): the tests' way to the small frames on which a box's placement can go wrong,
//     and the A/B's;
//   * kernels 41 / 44 / 48 as the frame's only pass: no lens, panorama or ray map, no sky image, no Doppler, no MSAA, no time windows,
//     no refine pass, no debug_rgb (a miss pixel's triple would have to be written as well).  Not the band-first kernels 43 / 49: they
//     serve the blocking call and the small frames, which the first point excludes, so their code is left as it was
//     (rpt_kernels.hip.h: tile_origin_policy);
//   * a context that renders whole frames into the 16-byte framebuffer (no colour plane, no rpt_set_rows / rpt_set_tile_pattern);
//   * 1 .. 64 objects, the rectangles of this frame at hand (those rpt_set_objects put on the device);
//   * a box of at most RPT_SKY_SPLIT_SHARE percent of the frame's tiles: split whatever the box covers, cubes.txt at 4K lost 1 % and
//     arch.txt at 1080p 6 % (§6.2d).  RPT_SKY_SPLIT_SHARE=<0..100> in the environment, read when a context is created, sets another
//     share: 0 is the escape hatch (never split), the others are for the A/B.
#define RPT_SKY_SPLIT_SHARE 50
#define RPT_SKY_SPLIT_MIN_PIXELS 6000000
long long env_integer(const char *name, long long lo, long long hi, long long otherwise) {
    const char *e = std::getenv(name);
    if (!e || !*e) return otherwise;
    char *end = nullptr;
    const long long v = std::strtoll(e, &end, 10);
    return *end == 0 && v >= lo && v <= hi ? v : otherwise;
}
int sky_split_share_wanted() { return (int)env_integer("RPT_SKY_SPLIT_SHARE", 0, 100, RPT_SKY_SPLIT_SHARE); }
long long sky_split_min_pixels_wanted() { return env_integer("RPT_SKY_SPLIT_MIN_PIXELS", 0, 1ll << 40, RPT_SKY_SPLIT_MIN_PIXELS); }
static_assert(rptd::tile_origin_policy<rptd::BallotExact> && rptd::tile_origin_policy<rptd::Ballot> && rptd::tile_origin_policy<rptd::Analytic> &&
              !rptd::tile_origin_policy<rptd::BallotFirstExact> && !rptd::tile_origin_policy<rptd::BallotFirst> && !rptd::tile_origin_policy<rptd::Unculled> &&
              !rptd::tile_origin_policy<rptd::DopplerTwin<rptd::BallotExact>> && !rptd::tile_origin_policy<rptd::Lens<rptd::BallotExact>>,
              "the forms sky_split_box lets through (walk, analytic, ieee) are the kernels that add tile_x0");
bool sky_split_box(const rpt_ctx *ctx, const Choice &c, Call call, const rptd::KernelArgs &a, int tiles, int box[4]) {
    const KernelRow *row = c.colour;
    if (!row || !row->kernel || c.windowed || c.refine || row->camera != Camera::pinhole || row->colour != Colour::plain) return false;
    if (!(row->form == Form::walk || row->form == Form::analytic || row->form == Form::ieee)) return false;
    if (call.kind != CallKind::in_flight || (long long)ctx->width * ctx->height <= ctx->sky_split_min_pixels) return false;
    if (!a.out16 || a.plane || a.debug_rgb || ctx->colour_plane || ctx->first_tile != 0 || ctx->tile_step != 1 || ctx->run_log2 != 0) return false;
    if (ctx->msaa > 1 || ctx->doppler || ctx->env_on || ctx->v_fov != 0.0f || ctx->projection != RPT_PROJECTION_PINHOLE) return false;
    if (ctx->object_count < 1 || ctx->object_count > 64 || ctx->rects.size() != (size_t)ctx->object_count) return false;
    if (!rpts::object_box(ctx->rects.data(), ctx->object_count, ctx->width, ctx->height, box)) return false;      // (nothing in view: one launch of sky tiles)
    const long long tiles_x = (ctx->width + 7) / 8, covered = (long long)(box[2] - box[0]) * (box[3] - box[1]);
    return covered * 100 <= tiles_x * tiles * ctx->sky_split_share;
}

// box: the tiles left to the render kernel; box[0] >= box[2]: none, the whole frame is filled
void launch_sky_fill(rpt_ctx *ctx, const rptd::KernelArgs &a, int tiles, const int box[4]) {
    rptd::SkyFillArgs s;
    s.out16 = a.out16;
    s.width = ctx->width;
    s.height = ctx->height;
    s.bg_packed = a.bg_packed;
    s.tx0 = box[0]; s.ty0 = box[1]; s.tx1 = box[2]; s.ty1 = box[3];
    const int tiles_x = (ctx->width + 7) / 8;
    hipLaunchKernelGGL(rptd::rpt_sky_fill_kernel, dim3((tiles_x + RPT_SKY_FILL_TILES - 1) / RPT_SKY_FILL_TILES, tiles), dim3(64), 0, ctx->stream, s);
}

// One colour frame on the context's stream: the choice, then buffers, arguments and the launch (pass A + pass B of an adaptive frame).
int launch(rpt_ctx *ctx, Call call) {
    const Choice c = choose_kernels(ctx, call);
    if (call.colour_frame && ctx->scene_uploaded && ctx->params_set) ctx->last_aa_variant = 0;
    if (c.code != RPT_OK) return fail(ctx, c.code, c.text);
    ctx->last_sky_split = false;
    if (int rc = ensure_outputs(ctx)) return rc;
    const int tiles = local_tile_count(ctx);
    if (call.colour_frame && ctx->aa_n > 1) {
        // pass A writes its packed colours here as well (the kernels honour `plane` next to `out16`; whole-frame contexts: local rows are the frame's)
        if (int rc = reserve(ctx, ctx->aa_plane, (size_t)tiles * RPT_TILE_ROWS * ctx->width * 4)) return rc;
        if (int rc = tally_ready(ctx, ctx->tally[TALLY_AA], 1)) return rc;
    }
    if (c.nothing) return RPT_OK;
    const bool panorama = ctx->projection == RPT_PROJECTION_EQUIRECT;
    if (panorama) {
        if (int rc = ensure_projection_tables(ctx, ctx->pano, 1)) return rc;
        if (c.refine)
            if (int rc = ensure_projection_tables(ctx, ctx->aa_pano, ctx->aa_n)) return rc;
    }

    if (int rc = ensure_tile_bits(ctx)) return rc;
    rptd::RaymapArgs a;         // (one block serves every render kernel: each reads its own prefix of it)
    fill_frame_args(ctx, a);
    a.raymap = c.colour && c.colour->camera == Camera::raymap ? (const float4 *)ctx->raymap.device.ptr : nullptr;     // (choose_kernels has checked it against the frame)
    a.raymap_pitch = ctx->raymap_pitch;
    if (c.refine) a.plane = (uint32_t *)ctx->aa_plane.ptr;
    if (c.band_first) set_band_first(ctx, a, tiles);
    a.msaa = ctx->msaa;
    a.doppler = ctx->doppler;
    a.debug_doppler = doppler_recording(ctx) ? (float *)(ctx->external_doppler ? ctx->external_doppler : ctx->owned_doppler.ptr) : nullptr;
    ctx->doppler_recorded = a.debug_doppler != nullptr;
    a.env_texels = ctx->env_on ? (const uint32_t *)ctx->env.device.ptr : nullptr;
    a.env_width = ctx->env_width;
    a.env_height = ctx->env_height;
    std::memcpy(a.env_frame, ctx->env_frame, sizeof a.env_frame);
    if (ctx->oriented) {          // (rpt_set_orientation: E' = E diag(1, R) — a sky at rest in the scene stays at rest when the head turns)
        rpt_float4 e[4];
        std::memcpy(e, ctx->env_frame, sizeof e);
        rebase_columns(e, ctx->R, a.env_frame);
    }

    const dim3 grid1(((ctx->width + 31) / 32) * 4, tiles);  // the product kernels: one wave (an 8 x 8 tile) per workgroup
    if (!c.colour) {
#ifdef RPT_DIAGNOSTICS
        const dim3 grid((ctx->width + 31) / 32, tiles);     // the measurement arms: four waves (a 32 x 8 strip) per workgroup
        if (int rc = launch_diagnostic(ctx, a, grid, tiles, c.variant)) return rc;
#endif
    } else if (!c.colour->kernel) {
        if (rpt_launch_relaxed_kernel(relaxed_waves(c.colour->form), &a, sizeof(rptd::KernelArgs), grid1.x, grid1.y, (void *)ctx->stream)) return fail(ctx, RPT_ERR_DEVICE, "relaxed-arithmetic kernel launch failed");
    } else {
        dim3 grid = grid1;
        int box[4];
        if (sky_split_box(ctx, c, call, a, tiles, box)) {
            // The sky split: the fill first, then the frame's own kernel over the box alone, both on the context's stream (the events of
            // render_frame bracket the two).  The box's origin: the column through tile_x0, the row through first_tile (0 here: the
            // rule refuses a context that renders a share of the rows).
            launch_sky_fill(ctx, a, tiles, box);
            a.tile_x0 = box[0];
            a.first_tile = box[1];
            grid = dim3(box[2] - box[0], box[3] - box[1]);
            ctx->last_sky_split = true;
            std::memcpy(ctx->last_sky_box, box, sizeof box);
        }
        void *args[] = {(void *)&a};
        (void)hipLaunchKernel(c.kernel(c.launched()), grid, dim3(64), args, 0, ctx->stream);     // (errors: below)
    }
    RPT_HIP(ctx, hipGetLastError());
    ctx->last_variant = c.variant;
    ctx->last_exact_rcp = c.ran_exact(c.launched());
    Tally &refined = ctx->tally[TALLY_AA];
    if (c.refine) {               // pass B, behind pass A on the same stream; then the counter's way home (last_event: the frame's end, render_frame)
        rptd::RefineArgs ra;
        std::memset(&ra, 0, sizeof ra);
        static_cast<rptd::LensArgs &>(ra) = static_cast<const rptd::LensArgs &>(a);
        ra.plane = nullptr;           // (pass B writes the framebuffer and debug_rgb only: the plane is what its neighbours still read)
        ra.aa_plane = (const uint32_t *)ctx->aa_plane.ptr;
        ra.aa_refined = (unsigned long long *)refined.device.ptr;
        ra.aa_cols = panorama ? (const float2 *)ctx->aa_pano.upload.device.ptr : nullptr;
        ra.aa_rows = panorama ? ra.aa_cols + (size_t)ctx->aa_n * ctx->width : nullptr;
        ra.aa_n = ctx->aa_n;
        ra.aa_threshold = ctx->aa_threshold;
        if (int rc = tally_zero(ctx, refined)) return rc;
        void *args[] = {(void *)&ra};
        (void)hipLaunchKernel(c.kernel(c.refine), grid1, dim3(64), args, 0, ctx->stream);
        RPT_HIP(ctx, hipGetLastError());
        if (int rc = tally_home(ctx, refined)) return rc;
        ctx->last_aa_variant = c.refine->variant;
    } else if (call.colour_frame) {    // a frame with the setting off refines nothing
        tally_off(refined);
    }
    return RPT_OK;
}

// One event pass on the context's stream: the record of every pixel of this context's rows, written at y * width + x of the full-frame
// record buffer.  The settings of Doppler, the sky and debug_rgb are not looked at (they act on colour only); neither the colour
// framebuffer nor anything rpt_last_variant / rpt_last_frame_ms report is touched.
int launch_events(rpt_ctx *ctx) {
    const Choice c = choose_kernels(ctx, Call{CallKind::events, false});
    if (c.code != RPT_OK) return fail(ctx, c.code, c.text);
    const size_t px = (size_t)ctx->width * ctx->height;
    if (!ctx->external_events && (px * sizeof(rpt_event) > ctx->owned_events.capacity || ctx->owned_events.bytes != px * sizeof(rpt_event))) {
        if (int rc = reserve(ctx, ctx->owned_events, px * sizeof(rpt_event))) return rc;
        RPT_HIP(ctx, hipMemsetAsync(ctx->owned_events.ptr, 0, px * sizeof(rpt_event), ctx->stream));
    }
    if (ctx->projection == RPT_PROJECTION_EQUIRECT)
        if (int rc = ensure_projection_tables(ctx, ctx->pano, 1)) return rc;
    rptd::RaymapEventArgs ea;   // (every event kernel reads its own prefix: EventArgs, or all of it)
    std::memset((void *)&ea, 0, sizeof ea);
    fill_frame_args(ctx, ea);
    ea.raymap = c.colour->camera == Camera::raymap ? (const float4 *)ctx->raymap.device.ptr : nullptr;
    ea.raymap_pitch = ctx->raymap_pitch;
    ea.out16 = nullptr;         // (the pass writes records only)
    ea.plane = nullptr;
    ea.debug_rgb = nullptr;
    ea.events = (rpt_event *)(ctx->external_events ? ctx->external_events : ctx->owned_events.ptr);
    ctx->event_frame.buffer = ea.events;
    ctx->event_frame.width = ctx->width;
    ctx->event_frame.height = ctx->height;
    ctx->events_first_tile = ctx->first_tile;
    ctx->events_tile_step = ctx->tile_step;
    ctx->events_run_log2 = ctx->run_log2;
    ctx->last_events_variant = c.variant;
    ctx->last_events_exact_rcp = c.ran_exact(c.launched());
    const int tiles = local_tile_count(ctx);
    if (tiles == 0) return RPT_OK;
    const dim3 grid1(((ctx->width + 31) / 32) * 4, tiles);      // one wave (an 8 x 8 tile) per workgroup, as the product kernels
    void *args[] = {(void *)&ea};
    (void)hipLaunchKernel(c.kernel(c.launched()), grid1, dim3(64), args, 0, ctx->stream);     // (errors: below)
    RPT_HIP(ctx, hipGetLastError());
    return RPT_OK;
}

uint32_t packed_rgba(const uint8_t c[4]) { return (uint32_t)c[0] | ((uint32_t)c[1] << 8) | ((uint32_t)c[2] << 16) | ((uint32_t)c[3] << 24); }

// What a pass over a rendered frame and its records (the overlay, the readouts, the splat passes) asks for before it launches, `call` naming it in the
// messages: a context that renders whole frames, and a colour frame and an event frame of the current size and view in the buffers
// now set.  *out16 and *events: those buffers.
int frames_of_this_view(rpt_ctx *ctx, const char *call, rpt_pixel **out16_out, const rpt_event **events_out) {
    const std::string name(call);
    if (!ctx->scene_uploaded) return fail(ctx, RPT_ERR_STATE, name + " before rpt_upload_scene");
    if (!ctx->params_set) return fail(ctx, RPT_ERR_STATE, name + " before rpt_set_params");
    if (ctx->first_tile != 0 || ctx->tile_step != 1 || ctx->colour_plane)
        return fail(ctx, RPT_ERR_ARG, name + ": the pass reads a pixel's upper neighbour, which on a context restricted by rpt_set_rows / rpt_set_tile_pattern (or rendering a colour plane) belongs to another rank");
    const FrameMark &colour = ctx->colour_frame, &event = ctx->event_frame;
    const auto of_this_size = [ctx](const FrameMark &f) { return f.width == ctx->width && f.height == ctx->height; };
    if (!colour.rendered()) return fail(ctx, RPT_ERR_STATE, name + ": no colour frame rendered yet");
    if (!event.rendered()) return fail(ctx, RPT_ERR_STATE, name + ": no event frame rendered yet (rpt_render_events)");
    if (!of_this_size(colour) || !of_this_size(event))
        return fail(ctx, RPT_ERR_STATE, name + ": the last colour frame and event frame are not both of the current width x height");
    if (colour.generation != ctx->view_generation || event.generation != ctx->view_generation)
        return fail(ctx, RPT_ERR_STATE, name + ": the view has changed (objects, time windows, params, projection, orientation or lens) since the last colour frame or event frame; render both again");
    rpt_pixel *out16 = (rpt_pixel *)(ctx->external_out ? ctx->external_out : ctx->owned_out.ptr);
    const rpt_event *events = (const rpt_event *)(ctx->external_events ? ctx->external_events : ctx->owned_events.ptr);
    // the buffers the two frames were rendered into are the ones the pass reads and writes: a buffer set since then holds no frame (and
    // a library-owned one may be smaller than this frame)
    if (!out16 || !events || (void *)out16 != colour.buffer || (const void *)events != event.buffer)
        return fail(ctx, RPT_ERR_STATE, name + ": rpt_set_output or rpt_set_events_output has named another buffer since the colour frame and the event frame were rendered");
    *out16_out = out16;
    *events_out = events;
    return RPT_OK;
}

// The shape of a pass over a rendered frame (the overlay, the readouts and the three splat passes: the stars, the particles, the
// segments), `call` naming it in the messages and `which` its tally.  Off: nothing is checked, launched or changed, and it reports zero.
// On: frames_of_this_view, then `enqueue`, the pass's own part (its refusals, tally_ready, its arguments, tally_zero, its launches; a
// splat pass has enqueue_splat do all but the first and the arguments), then the tally's way home, whose event is last_event.
using PassEnqueue = int (*)(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events);
int frame_pass(rpt_ctx *ctx, const char *call, bool on, int which, PassEnqueue enqueue) {
    Tally &tally = ctx->tally[which];
    if (!on) {
        tally_off(tally);
        return RPT_OK;
    }
    rpt_pixel *out16 = nullptr;
    const rpt_event *events = nullptr;
    if (int rc = frames_of_this_view(ctx, call, &out16, &events)) return rc;
    if (int rc = enqueue(ctx, tally, out16, events)) return rc;
    if (int rc = tally_home(ctx, tally)) return rc;
    ctx->last_event = tally.copied;
    return RPT_OK;
}

// One overlay pass on the context's stream (kernel 1100, behind 1101 where the tint's range is the frame's own).  The tally's 8 spare
// bytes: the bit pattern of the frame's largest delay.
int enqueue_overlay(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    const rpt_overlay_desc &d = ctx->overlay;
    if (int rc = tally_ready(ctx, tally, 1, 8)) return rc;

    rptd::OverlayArgs a;
    std::memset(&a, 0, sizeof a);
    a.events = events;
    a.out16 = out16;
    a.changed = (unsigned long long *)tally.device.ptr;
    a.width = ctx->width;
    a.height = ctx->height;
    a.layers = d.layers;
    a.interval = (float)ctx->interval;
    if (d.layers & RPT_OVERLAY_ISO_DELAY) a.delay_inv = 1.0f / d.delay_step;
    if (d.layers & RPT_OVERLAY_ISO_CLOCK) a.clock_inv = 1.0f / d.clock_step;
    if (d.layers & RPT_OVERLAY_LATTICE)
        for (int k = 0; k < 3; k++)
            if (d.lattice_step[k] != 0.0f) {
                a.lattice_inv[k] = 1.0f / d.lattice_step[k];
                a.layers |= (1u << k) << RPT_OVERLAY_AXIS_SHIFT;
            }
    a.tint_t_max = d.tint_t_max;
    a.outline_rgba = packed_rgba(d.outline_rgba);
    a.delay_rgba = packed_rgba(d.delay_rgba);
    a.clock_rgba = packed_rgba(d.clock_rgba);
    a.lattice_rgba = packed_rgba(d.lattice_rgba);
    a.tint_alpha = d.tint_alpha;

    const size_t pixels = (size_t)ctx->width * ctx->height;
    if (int rc = tally_zero(ctx, tally)) return rc;
    if ((d.layers & RPT_OVERLAY_DELAY_TINT) && d.tint_t_max == 0.0f) {
        uint32_t *tmax = (uint32_t *)tally.device.ptr + 2;
        a.tmax_bits = tmax;
        const size_t blocks = (pixels + 255) / 256;
        const float interval = a.interval;
        void *args[] = {(void *)&events, (void *)&pixels, (void *)&interval, (void *)&tmax};
        (void)hipLaunchKernel((const void *)rptd::rpt_overlay_tmax_kernel, dim3((unsigned)(blocks < 4096 ? blocks : 4096)), dim3(256), args, 0, ctx->stream);
        RPT_HIP(ctx, hipGetLastError());
    }
    const dim3 grid((ctx->width + RPT_OVERLAY_TILE_W - 1) / RPT_OVERLAY_TILE_W, (ctx->height + RPT_OVERLAY_TILE_H - 1) / RPT_OVERLAY_TILE_H);
    void *args[] = {(void *)&a};
    (void)hipLaunchKernel((const void *)rptd::rpt_overlay_kernel, grid, dim3(RPT_OVERLAY_TILE_W * RPT_OVERLAY_TILE_H), args, 0, ctx->stream);
    RPT_HIP(ctx, hipGetLastError());
    return RPT_OK;
}

int launch_overlay(rpt_ctx *ctx) { return frame_pass(ctx, "rpt_render_overlay", ctx->overlay.layers != 0, TALLY_OVERLAY, enqueue_overlay); }

// One readout pass on the context's stream (kernel 1110)
int enqueue_readouts(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    if (ctx->readouts.size() != (size_t)ctx->object_count)
        return fail(ctx, RPT_ERR_ARG, "rpt_render_readouts: " + std::to_string(ctx->readouts.size()) + " readouts are set, the Object[] holds " + std::to_string(ctx->object_count));
    if (int rc = tally_ready(ctx, tally, 1)) return rc;

    rptd::ReadoutArgs a;
    std::memset(&a, 0, sizeof a);
    a.events = events;
    a.out16 = out16;
    a.changed = (unsigned long long *)tally.device.ptr;
    a.displays = (const rptd::ReadoutDisplay *)ctx->readout_table.device.ptr;
    a.low_mask = ctx->readout_low_mask;
    a.width = ctx->width;
    a.height = ctx->height;
    a.count = ctx->object_count;
    if (int rc = tally_zero(ctx, tally)) return rc;
    const dim3 grid((ctx->width + RPT_OVERLAY_TILE_W - 1) / RPT_OVERLAY_TILE_W, (ctx->height + RPT_OVERLAY_TILE_H - 1) / RPT_OVERLAY_TILE_H);
    void *args[] = {(void *)&a};
    (void)hipLaunchKernel((const void *)rptd::rpt_readout_kernel, grid, dim3(RPT_OVERLAY_TILE_W * RPT_OVERLAY_TILE_H), args, 0, ctx->stream);
    RPT_HIP(ctx, hipGetLastError());
    return RPT_OK;
}

int launch_readouts(rpt_ctx *ctx) { return frame_pass(ctx, "rpt_render_readouts", !ctx->readouts.empty(), TALLY_READOUTS, enqueue_readouts); }

// The fixed-point accumulator of the splat passes, 24 B per pixel of the largest frame so far
int accumulator_ready(rpt_ctx *ctx, size_t pixels) {
    const size_t acc_bytes = pixels * 3 * sizeof(unsigned long long);
    if (acc_bytes > ctx->splat_acc.capacity || !ctx->splat_acc.ptr) {    // a new accumulator starts all zero; passes leave it so
        RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // (a pass in flight may still use the old one)
        if (int rc = reserve(ctx, ctx->splat_acc, acc_bytes)) return rc;
        RPT_HIP(ctx, hipMemsetAsync(ctx->splat_acc.ptr, 0, ctx->splat_acc.capacity, ctx->stream));
    }
    return RPT_OK;
}

// The planes of a glared pass, `layers` of 24 B per pixel.  They need no zeroing: kernel 1170 writes every word of the frame's planes
// before kernel 1171 reads any
int glare_planes_ready(rpt_ctx *ctx, size_t pixels) {
    const size_t bytes = pixels * 3 * sizeof(unsigned long long) * (size_t)ctx->glare_layers;
    if (bytes > ctx->glare_planes.capacity || !ctx->glare_planes.ptr) {
        RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));                 // (a pass in flight may still use the old ones)
        if (int rc = reserve(ctx, ctx->glare_planes, bytes)) return rc;
    }
    return RPT_OK;
}

// The refusals the splat passes share, `call` naming the pass and `noun` what it projects: a caller's ray map (all three); and for a
// pass whose records ride objects an interval the light cone has no closed form for, and a set that names an object beyond Object[] —
// what keeps every index the splat follows inside it.  Like all of a pass's refusals they come before anything touches the device.
int splat_refusals(rpt_ctx *ctx, const SplatPass &p, const char *call, const char *noun, bool rides_objects) {
    const std::string name(call);
    if (ctx->projection == RPT_PROJECTION_RAYMAP)
        return fail(ctx, RPT_ERR_ARG, name + ": RPT_PROJECTION_RAYMAP is set, and a caller's ray map has no inverse to project a " + noun + " with");
    if (!rides_objects) return RPT_OK;
    if (ctx->interval != -1 && ctx->interval != 0)
        return fail(ctx, RPT_ERR_ARG, name + ": interval is " + std::to_string(ctx->interval) + "; the light cone has a closed form for -1 and 0 only");
    if (p.largest_object >= ctx->object_count)
        return fail(ctx, RPT_ERR_ARG, name + ": the set names object " + std::to_string(p.largest_object) + ", the Object[] holds " + std::to_string(ctx->object_count));
    return RPT_OK;
}

// ... and the one of the passes with temperatures, `setter` having set them and `records` naming what they run parallel to: a count that
// is not the records' (what keeps xg[i] of kernels 1122 and 1132 inside its array)
int thermal_refusal(rpt_ctx *ctx, const SplatPass &p, const char *call, const char *setter, const char *records) {
    if (p.thermal_count == 0 || p.thermal_count == p.count) return RPT_OK;
    return fail(ctx, RPT_ERR_ARG, std::string(call) + ": " + std::to_string(p.thermal_count) + " temperatures are set (" + setter + "), the " + records + " holds " + std::to_string(p.count));
}

// The view as §19 rule 4 projects it, for StarArgs and ParticleArgs alike
template <typename Args>
void splat_view(const rpt_ctx *ctx, Args &a) {
    a.width = ctx->width;
    a.height = ctx->height;
    a.interval = ctx->interval;
    a.doppler = ctx->interval != 0 ? ctx->doppler : 0;
    if (ctx->projection == RPT_PROJECTION_EQUIRECT) {
        a.camera = RPT_STARS_EQUIRECT;
        a.h_fov = ctx->projection_params[0];
        a.v_fov = ctx->projection_params[1];
        a.yaw = ctx->projection_params[2];
        a.wrap = a.h_fov == (float)(2.0 * RPT_PI_D) ? 1 : 0;
    } else {
        const float s = ctx->v_fov != 0.0f ? ctx->lens_scale : 1.0f;
        a.plane_x = s * ((float)ctx->width / (float)ctx->height);
        a.plane_y = s;
    }
}

// What follows a splat pass's refusals, once for the three: the accumulator, the tally's `words`, the marks of a timed pass, the tally
// zeroed, `splat` — the pass's own launch, handed the accumulator and the tally's words for its arguments — and the resolve, kernel
// `resolve` with `b`: the caller has set what is its kernel's alone (1121's records), the rest is filled here.  With rpt_set_glare the
// planes are made ready behind the accumulator, and kernels 1170 and 1171 (rpt_glare.hip.h) stand in the resolve's place, between the
// same two marks: `wrap` is the splat's, and the star pass's records are the mask of rule G2.
template <typename ResolveArgs, typename Splat>
int enqueue_splat(rpt_ctx *ctx, int which, Tally &tally, size_t words, rpt_pixel *out16, const void *resolve, ResolveArgs &b, Splat splat) {
    SplatPass &p = ctx->splat[which];
    const size_t pixels = (size_t)ctx->width * (size_t)ctx->height;
    if (int rc = accumulator_ready(ctx, pixels)) return rc;
    if (ctx->glare_layers != 0)
        if (int rc = glare_planes_ready(ctx, pixels)) return rc;
    if (int rc = tally_ready(ctx, tally, words)) return rc;
    if (p.timed)
        for (hipEvent_t &m : p.marks)
            if (!m) RPT_HIP(ctx, hipEventCreate(&m));

    b.acc = (unsigned long long *)ctx->splat_acc.ptr;
    b.out16 = out16;
    b.counts = (unsigned long long *)tally.device.ptr;
    b.pixels = pixels;
    for (int c = 0; c < 3; c++) b.hable_wp[c] = hable_host(ctx->white_point[c]);

    if (int rc = tally_zero(ctx, tally)) return rc;
    if (p.timed) RPT_HIP(ctx, hipEventRecord(p.marks[0], ctx->stream));
    splat(b.acc, b.counts);
    RPT_HIP(ctx, hipGetLastError());
    if (p.timed) RPT_HIP(ctx, hipEventRecord(p.marks[1], ctx->stream));
    if (ctx->glare_layers != 0) {
        rptd::GlareArgs g;
        std::memset((void *)&g, 0, sizeof g);
        g.acc = b.acc;
        g.planes = (unsigned long long *)ctx->glare_planes.ptr;
        if constexpr (std::is_same<ResolveArgs, rptd::StarResolveArgs>::value) g.events = b.events;
        g.out16 = out16;
        g.counts = b.counts;
        g.pixels = pixels;
        g.width = ctx->width;
        g.height = ctx->height;
        g.wrap = ctx->projection == RPT_PROJECTION_EQUIRECT && ctx->projection_params[0] == (float)(2.0 * RPT_PI_D) ? 1 : 0;     // (splat_view's)
        g.layers = ctx->glare_layers;
        std::memcpy(g.hable_wp, b.hable_wp, sizeof g.hable_wp);
        std::memcpy(g.weight, ctx->glare_weight, sizeof g.weight);
        std::memcpy(g.radius, ctx->glare_radius, sizeof g.radius);
        std::memcpy(g.taps, ctx->glare_taps, sizeof g.taps);
        void *glare_args[] = {(void *)&g};
        const dim3 segments((unsigned)((ctx->width + RPT_GLARE_SEGMENT - 1) / RPT_GLARE_SEGMENT), (unsigned)ctx->height);
        (void)hipLaunchKernel((const void *)rptd::rpt_glare_rows_kernel, segments, dim3(RPT_GLARE_SEGMENT), glare_args, 0, ctx->stream);
        RPT_HIP(ctx, hipGetLastError());
        const dim3 tiles((unsigned)((ctx->width + RPT_GLARE_TILE - 1) / RPT_GLARE_TILE), (unsigned)((ctx->height + RPT_GLARE_TILE - 1) / RPT_GLARE_TILE));
        (void)hipLaunchKernel((const void *)rptd::rpt_glare_columns_kernel, tiles, dim3(RPT_GLARE_TILE * RPT_GLARE_TILE), glare_args, 0, ctx->stream);
    } else {
        void *resolve_args[] = {(void *)&b};
        (void)hipLaunchKernel(resolve, dim3((unsigned)((pixels + 255) / 256)), dim3(256), resolve_args, 0, ctx->stream);
    }
    RPT_HIP(ctx, hipGetLastError());
    if (p.timed) RPT_HIP(ctx, hipEventRecord(p.marks[2], ctx->stream));
    p.marked = p.timed;
    return RPT_OK;
}

// rpt_render_stars, _particles, _segments, _ballistics, _rockets: a pass that is off has no marks of one either; then frame_pass
int launch_splat(rpt_ctx *ctx, int which, const char *call, int tally, PassEnqueue enqueue) {
    SplatPass &p = ctx->splat[which];
    if (p.count == 0) p.marked = false;
    return frame_pass(ctx, call, p.count != 0, tally, enqueue);
}

// One star-field pass on the context's stream (kernels 1120 or 1122, and 1121): its refusals, G, the launch
int enqueue_stars(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    const SplatPass &p = ctx->splat[SPLAT_STARS];
    if (int rc = splat_refusals(ctx, p, "rpt_render_stars", "star", false)) return rc;
    if (int rc = thermal_refusal(ctx, p, "rpt_render_stars", "rpt_set_star_temperatures", "catalogue")) return rc;
    rptd::StarArgs a;
    std::memset((void *)&a, 0, sizeof a);
    {   // E' as a colour frame's launch forms it, then G
        rpt_float4 e[4];
        std::memcpy(e, ctx->env_frame, sizeof e);
        if (ctx->oriented) rebase_columns(e, ctx->R, e);
        float g[16];
        if (!rpts::sky_to_camera(&e[0].x, ctx->interval, g))
            return fail(ctx, RPT_ERR_ARG, "rpt_render_stars: the sky matrix (rpt_set_environment_frame) cannot be inverted");
        std::memcpy(a.G, g, sizeof a.G);
    }
    a.stars = (const rpt_star *)p.table.device.ptr;
    a.count = p.count;
    splat_view(ctx, a);
    rptd::StarResolveArgs b;
    std::memset((void *)&b, 0, sizeof b);
    b.events = events;
    return enqueue_splat(ctx, SPLAT_STARS, tally, 2, out16, (const void *)rptd::rpt_stars_resolve_kernel, b, [&](unsigned long long *acc, unsigned long long *counts) {
        a.acc = acc;
        a.counts = counts;
        const float *xg = (const float *)p.thermal_table.device.ptr;
        void *splat_args[] = {(void *)&a, (void *)&xg};     // (1120 takes the first only)
        (void)hipLaunchKernel(p.thermal_count != 0 ? (const void *)rptd::rpt_stars_thermal_splat_kernel : (const void *)rptd::rpt_stars_splat_kernel,
                              dim3((unsigned)((p.count + 255) / 256)), dim3(256), splat_args, 0, ctx->stream);
    });
}

int launch_stars(rpt_ctx *ctx) { return launch_splat(ctx, SPLAT_STARS, "rpt_render_stars", TALLY_STARS, enqueue_stars); }

// the arguments the ray-level probes and the lit particles' shadow ray need: the resident scene and the current Object[] / DObj[] (no
// frame, no outputs)
void probe_kernel_args(rpt_ctx *ctx, rptd::KernelArgs &a) {
    std::memset(&a, 0, sizeof a);
    a.dnodes = (const rptd::DNode *)ctx->geo->dnodes.ptr;
    a.dtris = (const rptd::DTri *)ctx->geo->dtris.ptr;
    a.links = (const int *)ctx->geo->dlinks.ptr;
    a.first_tris = (const rptd::DTri *)ctx->geo->dfirst.ptr;
    a.exits = (const rptd::DExit *)ctx->geo->dexits.ptr;
    a.hits = (const rptd::DHit *)ctx->geo->dhits.ptr;
    a.top_count = ctx->geo->top_count;
    a.dobjs = (const rptd::DObj *)((const char *)ctx->objects.ptr + (size_t)ctx->object_count * sizeof(rpt_object));
    a.objects = (const rpt_object *)ctx->objects.ptr;
    a.vertices = (const rpt_float3 *)ctx->geo->vertices.ptr;
    a.normals = (const rpt_float3 *)ctx->geo->normals.ptr;
    a.uvs = (const rpt_float2 *)ctx->geo->uvs.ptr;
    a.triangles = (const uint32_t *)ctx->geo->triangles.ptr;
    a.octrees = (const rpt_octree *)ctx->geo->octrees.ptr;
    a.octreeTris = (const int32_t *)ctx->geo->octreeTris.ptr;
    a.textures = (const uint8_t *)ctx->geo->textures.ptr;
    a.texture_bytes = (long long)ctx->geo->textures.bytes;
    a.object_count = ctx->object_count;
    a.interval = ctx->interval;
}

// What the passes whose records name objects hand their splat kernels alike: the objects, the records of the view, the view, and the
// pass's count and options.  The objects' windows (`with_windows`: the particles and the segments ride their objects; a ballistic
// record and a rocket bring their own) and the set's pointer are the caller's; the accumulator and the tally's words come with the launch.
void object_pass_args(rpt_ctx *ctx, const SplatPass &p, const rpt_event *events, bool with_windows, rptd::ParticleArgs &a) {
    std::memset((void *)&a, 0, sizeof a);
    a.objects = (const rpt_object *)ctx->objects.ptr;
    if (with_windows && !ctx->windows.empty())      // (their count is the Object[]'s: the frames of this view were launched with them)
        a.dobjs = (const rptd::DObj *)((const char *)ctx->objects.ptr + (size_t)ctx->object_count * sizeof(rpt_object));
    a.events = events;
    a.object_count = ctx->object_count;
    a.count = p.count;
    a.inverse_square = p.flags & RPT_PARTICLES_INVERSE_SQUARE;       // (RPT_SEGMENTS_INVERSE_SQUARE is the same bit)
    a.depth_bias = p.depth_bias;
    splat_view(ctx, a);
}

// A point-source splat, one lane per record: `plain`, or `thermal` with the pass's x_G where temperatures are set
void launch_point_splat(rpt_ctx *ctx, const SplatPass &p, rptd::ParticleArgs &a, const void *plain, const void *thermal) {
    const float *xg = (const float *)p.thermal_table.device.ptr;
    void *splat_args[] = {(void *)&a, (void *)&xg};         // (`plain` takes the first only)
    (void)hipLaunchKernel(p.thermal_count != 0 ? thermal : plain, dim3((unsigned)((p.count + 255) / 256)), dim3(256), splat_args, 0, ctx->stream);
}

// One particle pass on the context's stream (kernels 1130 or 1132, and 1131): its refusals, the launch.  With rpt_set_particle_lighting
// the splat is one of the lit kernels (1134, 1135, 1136; rptl::splat_kernel chooses) after two more refusals (rptl::launch_fault), and
// two more words of the tally come home: the (particle, light) pairs that lit and the pairs shadowed
int enqueue_particles(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    const SplatPass &p = ctx->splat[SPLAT_PARTICLES];
    if (int rc = splat_refusals(ctx, p, "rpt_render_particles", "particle", true)) return rc;
    if (int rc = thermal_refusal(ctx, p, "rpt_render_particles", "rpt_set_particle_temperatures", "set")) return rc;
    const rptl::LaunchFault dust_fault = rptl::launch_fault(ctx->particle_lighting, p.thermal_count, ctx->geo->compact_ok);
    if (dust_fault.code != RPT_OK) return fail(ctx, dust_fault.code, "rpt_render_particles: " + dust_fault.message);

    rptd::ParticleArgs a;
    object_pass_args(ctx, p, events, true, a);
    a.particles = (const rpt_particle *)p.table.device.ptr;
    rptd::ParticleResolveArgs b;
    std::memset((void *)&b, 0, sizeof b);
    // the tally's four words: seen, changed pixels; (particle, light) pairs lit, pairs shadowed (zero for a plain pass)
    return enqueue_splat(ctx, SPLAT_PARTICLES, tally, 4, out16, (const void *)rptd::rpt_particles_resolve_kernel, b, [&](unsigned long long *acc, unsigned long long *counts) {
        a.acc = acc;
        a.counts = counts;
        const int splat = rptl::splat_kernel(ctx->particle_lighting, ctx->interval, p.thermal_count, !ctx->windows.empty());
        if (splat == 1130 || splat == 1132) {                   // (1132: temperatures are set)
            launch_point_splat(ctx, p, a, (const void *)rptd::rpt_particles_splat_kernel, (const void *)rptd::rpt_particles_thermal_splat_kernel);
        } else {                                                // lit particles: 1134, or 1135 / 1136 with the scene for the shadow ray
            rptd::DustArgs d;
            std::memset((void *)&d, 0, sizeof d);
            d.p = a;
            d.ambient = ctx->ambient;
            d.add_ambient = ctx->particle_lighting & RPT_PARTICLES_AMBIENT;
            rptd::KernelArgs k;
            probe_kernel_args(ctx, k);
            void *splat_args[] = {(void *)&d, (void *)&k};      // (1134 takes the first only)
            (void)hipLaunchKernel(splat == 1134 ? (const void *)rptd::rpt_dust_splat_kernel
                                  : splat == 1135 ? (const void *)rptd::rpt_dust_shadowed_splat_kernel : (const void *)rptd::rpt_dust_shadowed_windowed_splat_kernel,
                                  dim3((unsigned)((p.count + 255) / 256)), dim3(256), splat_args, 0, ctx->stream);
        }
    });
}

int launch_particles(rpt_ctx *ctx) { return launch_splat(ctx, SPLAT_PARTICLES, "rpt_render_particles", TALLY_PARTICLES, enqueue_particles); }

// One segment pass on the context's stream (kernels 1140 and 1131): the refusals of a pass that rides objects, the launch.  One lane
// per piece.
int enqueue_segments(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    const SplatPass &p = ctx->splat[SPLAT_SEGMENTS];
    if (int rc = splat_refusals(ctx, p, "rpt_render_segments", "node", true)) return rc;

    rptd::SegmentArgs a;
    std::memset((void *)&a, 0, sizeof a);
    object_pass_args(ctx, p, events, true, a.p);
    a.segments = (const rpt_segment *)p.table.device.ptr;
    a.pieces = ctx->segment_pieces;
    while ((1 << a.shift) < a.pieces) a.shift++;
    if (a.p.camera == RPT_STARS_EQUIRECT) a.period = (float)ctx->width * ((float)(2.0 * RPT_PI_D) / a.p.h_fov);
    rptd::ParticleResolveArgs b;
    std::memset((void *)&b, 0, sizeof b);
    return enqueue_splat(ctx, SPLAT_SEGMENTS, tally, 2, out16, (const void *)rptd::rpt_particles_resolve_kernel, b, [&](unsigned long long *acc, unsigned long long *counts) {
        a.p.acc = acc;
        a.p.counts = counts;
        const void *splat = (const void *)rptd::rpt_segments_splat_kernel;
#ifdef RPT_DIAGNOSTICS
        if (ctx->variant == 1141) splat = (const void *)rptd::rpt_segments_splat_loop_kernel;      // the measurement arm: a loop per lane
#endif
        const unsigned lanes = (unsigned)p.count * (unsigned)ctx->segment_pieces;      // <= 2^21 (rptg::kMaxPieces)
        void *splat_args[] = {(void *)&a};
        (void)hipLaunchKernel(splat, dim3((lanes + 255u) / 256u), dim3(256), splat_args, 0, ctx->stream);
    });
}

int launch_segments(rpt_ctx *ctx) { return launch_splat(ctx, SPLAT_SEGMENTS, "rpt_render_segments", TALLY_SEGMENTS, enqueue_segments); }

// The passes of records with a worldline of their own, written in an object's frame: what differs between them on the host
struct WorldlinePass {
    int which;                          // SPLAT_*
    const char *call, *noun;            // as the refusals name the pass and what it projects
    const char *temperatures;           // the setter of its temperatures
    const void *plain, *thermal;        // the splat kernel without and with them
};

// One ballistic or rocket pass on the context's stream (kernels 1150 or 1152, 1160 or 1162, and 1131): the refusals
// of a pass whose records name objects, the launch.  The objects' time windows are not handed over: a record has its own window.  The
// kernels read a.particles as their own records, 48 B and 64 B each.
int enqueue_worldlines(rpt_ctx *ctx, const WorldlinePass &w, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    const SplatPass &p = ctx->splat[w.which];
    if (int rc = splat_refusals(ctx, p, w.call, w.noun, true)) return rc;
    if (int rc = thermal_refusal(ctx, p, w.call, w.temperatures, "set")) return rc;

    rptd::ParticleArgs a;
    object_pass_args(ctx, p, events, false, a);
    a.particles = (const rpt_particle *)p.table.device.ptr;
    rptd::ParticleResolveArgs b;
    std::memset((void *)&b, 0, sizeof b);
    return enqueue_splat(ctx, w.which, tally, 2, out16, (const void *)rptd::rpt_particles_resolve_kernel, b, [&](unsigned long long *acc, unsigned long long *counts) {
        a.acc = acc;
        a.counts = counts;
        launch_point_splat(ctx, p, a, w.plain, w.thermal);
    });
}

int enqueue_ballistics(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    return enqueue_worldlines(ctx, {SPLAT_BALLISTICS, "rpt_render_ballistics", "particle", "rpt_set_ballistic_temperatures", (const void *)rptd::rpt_ballistics_splat_kernel,
                                    (const void *)rptd::rpt_ballistics_thermal_splat_kernel}, tally, out16, events);
}

int enqueue_rockets(rpt_ctx *ctx, Tally &tally, rpt_pixel *out16, const rpt_event *events) {
    return enqueue_worldlines(ctx, {SPLAT_ROCKETS, "rpt_render_rockets", "rocket", "rpt_set_rocket_temperatures", (const void *)rptd::rpt_rockets_splat_kernel,
                                    (const void *)rptd::rpt_rockets_thermal_splat_kernel}, tally, out16, events);
}

int launch_ballistics(rpt_ctx *ctx) { return launch_splat(ctx, SPLAT_BALLISTICS, "rpt_render_ballistics", TALLY_BALLISTICS, enqueue_ballistics); }
int launch_rockets(rpt_ctx *ctx) { return launch_splat(ctx, SPLAT_ROCKETS, "rpt_render_rockets", TALLY_ROCKETS, enqueue_rockets); }

// The event pass and what it leaves for rpt_pick, rpt_read_events and the passes over the frame
int launch_event_frame(rpt_ctx *ctx) {
    if (!ctx->ev_events) RPT_HIP(ctx, hipEventCreateWithFlags(&ctx->ev_events, hipEventDisableTiming));
    if (int rc = launch_events(ctx)) return rc;
    RPT_HIP(ctx, hipEventRecord(ctx->ev_events, ctx->stream));
    ctx->last_event = ctx->ev_events;
    ctx->event_frame.generation = ctx->view_generation;
    return RPT_OK;
}

// rpt_render_events, _overlay, _readouts, _stars, _particles, _segments and their _async forms: one pass on the context's stream, waited for or not
int render_pass(rpt_ctx *ctx, int (*launch_pass)(rpt_ctx *), bool wait) {
    if (!ctx) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = launch_pass(ctx)) return rc;
    return wait ? rpt_sync(ctx) : RPT_OK;
}

// a colour frame has been enqueued for the present view and size, into the present framebuffer
void mark_colour_frame(rpt_ctx *ctx) {
    ctx->colour_frame = FrameMark{ctx->view_generation, ctx->width, ctx->height, ctx->colour_plane ? nullptr : rpt_output_ptr(ctx)};
}

// rpt_set_stars, rpt_set_particles, rpt_set_segments, rpt_set_ballistics, rpt_set_rockets and the four rpt_set_*_temperatures, `call` naming the one: `count` records go to
// the device here, once, as `prepare` writes them, in stream order (a pass in flight keeps what it was launched with).  Null or zero
// switches off; a call refused for its arguments (`fault`: "" or what is wrong with them) has changed nothing, one that fails on the
// device (RPT_ERR_DEVICE) leaves nothing set — the table may be gone or half written.  `largest`, for records that name objects: what
// every launch holds against object_count.
template <typename Record, typename Fault>
int set_records(rpt_ctx *ctx, const char *call, StagedUpload &table, int &table_count, int &largest_object, const Record *records_or_null, int count,
                int max_count, Fault fault, void (*prepare)(const Record *, int, Record *), int (*largest)(const Record *, int) = nullptr) {
    const std::string name(call);
    if (count < 0 || count > max_count) return fail(ctx, RPT_ERR_ARG, name + ": " + fault((const Record *)nullptr, count));
    const bool off = !records_or_null || count == 0;
    if (!off) {
        const std::string what = fault(records_or_null, count);
        if (!what.empty()) return fail(ctx, RPT_ERR_ARG, name + ": " + what);
    }
    if (!off) RPT_HIP(ctx, hipSetDevice(ctx->device));
    table_count = 0;                    // (off, or until the copy below is on its way)
    largest_object = -1;
    if (off) return RPT_OK;
    void *host = nullptr;
    if (int rc = staged_host(ctx, table, (size_t)count * sizeof(Record), &host)) return rc;
    prepare(records_or_null, count, (Record *)host);
    if (int rc = staged_copy(ctx, table)) return rc;
    table_count = count;
    if (largest) largest_object = largest(records_or_null, count);
    return RPT_OK;
}

// rpt_set_stars_measurement, _particles_, _segments_, _ballistics_, _rockets_
int set_splat_measurement(rpt_ctx *ctx, int which, int timed) {
    if (!ctx) return RPT_ERR_ARG;
    ctx->splat[which].timed = timed != 0;
    return RPT_OK;
}

// rpt_last_stars_ms, _particles_, _segments_, _ballistics_, _rockets_: `name` as those calls spell the pass, `pass` as their message does
int last_splat_ms(rpt_ctx *ctx, int which, float ms[2], const char *name, const char *pass) {
    if (!ctx || !ms) return RPT_ERR_ARG;
    const SplatPass &p = ctx->splat[which];
    if (!p.marked)
        return fail(ctx, RPT_ERR_STATE, std::string("rpt_last_") + name + "_ms: the last " + pass + " pass was not timed (rpt_set_" + name + "_measurement)");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    RPT_HIP(ctx, hipEventSynchronize(p.marks[2]));
    RPT_HIP(ctx, hipEventElapsedTime(&ms[0], p.marks[0], p.marks[1]));
    RPT_HIP(ctx, hipEventElapsedTime(&ms[1], p.marks[1], p.marks[2]));
    return RPT_OK;
}

}  // namespace

extern "C" {

#ifdef RPT_DIAGNOSTICS
const char *rpt_version(void) { return "rpt-hip 0.2 (gfx950, diagnostics build)"; }
#else
const char *rpt_version(void) { return "rpt-hip 0.2 (gfx950)"; }
#endif

int rpt_create(rpt_ctx **out, int device_ordinal) {
    if (!out) return RPT_ERR_ARG;
    *out = nullptr;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return RPT_ERR_DEVICE;
    if (device_ordinal < 0 || device_ordinal >= n) return RPT_ERR_ARG;
    rpt_ctx *ctx = new (std::nothrow) rpt_ctx();
    if (!ctx) return RPT_ERR_NOMEM;
    ctx->device = device_ordinal;
    ctx->tile_triangles = tile_triangles_wanted();
    ctx->sky_split_share = sky_split_share_wanted();
    ctx->sky_split_min_pixels = sky_split_min_pixels_wanted();
    (void)rpth::Workers::instance();       // the helper pool exists from the first context on, not from the first animated frame (rpt_workers.hpp: fork())
    {
        static std::atomic<int> created{0};
        ctx->serial = created.fetch_add(1);
    }
    ctx->geo = std::make_shared<Geometry>();
    ctx->geo->device = device_ordinal;
    if (hipSetDevice(device_ordinal) != hipSuccess || hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking) != hipSuccess ||

        hipEventCreate(&ctx->ev_begin) != hipSuccess || hipEventCreate(&ctx->ev_end) != hipSuccess) {
        rpt_destroy(ctx);
        return RPT_ERR_DEVICE;
    }
    ctx->stream = ctx->own_stream;
    if (hipDeviceGetAttribute(&ctx->cu_count, hipDeviceAttributeMultiprocessorCount, device_ordinal) != hipSuccess || ctx->cu_count <= 0) ctx->cu_count = 256;
    *out = ctx;
    return RPT_OK;
}

int rpt_create_multi(rpt_ctx **out, const int *device_ordinals, int n) {
    if (!out || !device_ordinals || n <= 0) return RPT_ERR_ARG;
    for (int i = 0; i < n; i++) out[i] = nullptr;
    for (int i = 0; i < n; i++) {
        const int rc = rpt_create(&out[i], device_ordinals[i]);
        if (rc != RPT_OK) {
            for (int k = 0; k < i; k++) { rpt_destroy(out[k]); out[k] = nullptr; }
            return rc;
        }
    }
    return RPT_OK;
}

void rpt_destroy(rpt_ctx *ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    // work of this context may still be running on an external stream (rpt_set_stream) whose handle the caller may already
    // have destroyed: wait for the device rather than for a handle that may be dead, then free
    (void)hipDeviceSynchronize();
#ifdef RPT_DIAGNOSTICS
    if (ctx->host_calls > 0 && getenv("RPT_HOST_PROFILE"))
        fprintf(stderr, "[rpt] context %d: rpt_set_objects x %ld, us per call: wait for the staging slot %.1f, copy + DObj %.1f, screen bounds %.1f, hipMemcpyAsync %.1f, hipEventRecord %.1f\n",
                ctx->serial, ctx->host_calls, ctx->host_us[1] / ctx->host_calls, ctx->host_us[2] / ctx->host_calls, ctx->host_us[3] / ctx->host_calls,
                ctx->host_us[4] / ctx->host_calls, ctx->host_us[5] / ctx->host_calls);
#endif
    ctx->geo.reset();
    for (DeviceBuffer *b : {&ctx->objects, &ctx->dobjs, &ctx->counters, &ctx->wave_times, &ctx->tile_masks, &ctx->claim_counters, &ctx->verify_planes, &ctx->owned_out, &ctx->owned_plane, &ctx->owned_rgb, &ctx->owned_doppler, &ctx->owned_events, &ctx->aa_plane, &ctx->splat_acc, &ctx->glare_planes})
        release(*b);
    if (ctx->pinned_objects) (void)hipHostFree(ctx->pinned_objects);
    for (StagedUpload *u : {&ctx->pano.upload, &ctx->aa_pano.upload, &ctx->env, &ctx->tile_bits, &ctx->raymap, &ctx->readout_table}) release(*u);
    for (Tally &t : ctx->tally) release(t);
    for (SplatPass &p : ctx->splat) {
        release(p.table);
        release(p.thermal_table);
        for (hipEvent_t m : p.marks) if (m) (void)hipEventDestroy(m);
    }
    for (hipEvent_t e : ctx->staging_done) if (e) (void)hipEventDestroy(e);
    if (ctx->ev_begin) (void)hipEventDestroy(ctx->ev_begin);
    if (ctx->ev_end) (void)hipEventDestroy(ctx->ev_end);
    if (ctx->ev_events) (void)hipEventDestroy(ctx->ev_events);
    for (hipEvent_t e : ctx->timing_events) (void)hipEventDestroy(e);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

const char *rpt_last_error(const rpt_ctx *ctx) { return ctx ? ctx->error.c_str() : "null context"; }

int rpt_upload_scene(rpt_ctx *ctx, const rpt_scene_desc *s) {
    if (!ctx || !s) return RPT_ERR_ARG;
    if ((s->object_count && !s->objects) || (s->vertex_count && !s->vertices) || (s->normal_count && !s->normals) ||
        (s->uv_count && !s->uvs) || (s->triangle_words && !s->triangles) || (s->octree_count && !s->octrees) ||
        (s->octree_tri_count && !s->octreeTris) || (s->texture_bytes && !s->textures))
        return fail(ctx, RPT_ERR_ARG, "rpt_upload_scene: null pointer with nonzero count");
    if (s->object_count > (1u << 20)) return fail(ctx, RPT_ERR_ARG, "rpt_upload_scene: too many objects");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = validate_geometry(ctx, *s)) return rc;
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->scene_uploaded = false;
    // a fresh Geometry: contexts sharing the previous one (rpt_share_scene) keep it until they let go
    ctx->geo = std::make_shared<Geometry>();
    ctx->geo->device = ctx->device;
    {   // (an address can be reused by a later Geometry; a generation cannot)
        static std::atomic<unsigned long long> next_generation{1};
        ctx->geo->generation = next_generation.fetch_add(1);
    }
    ctx->rects.clear();
    if (int rc = upload(ctx, ctx->geo->vertices, s->vertices, s->vertex_count * sizeof(rpt_float3))) return rc;
    if (int rc = upload(ctx, ctx->geo->normals, s->normals, s->normal_count * sizeof(rpt_float3))) return rc;
    if (int rc = upload(ctx, ctx->geo->uvs, s->uvs, s->uv_count * sizeof(rpt_float2))) return rc;
    if (int rc = upload(ctx, ctx->geo->triangles, s->triangles, s->triangle_words * sizeof(uint32_t))) return rc;
    if (int rc = upload(ctx, ctx->geo->octrees, s->octrees, s->octree_count * sizeof(rpt_octree))) return rc;
    if (int rc = upload(ctx, ctx->geo->octreeTris, s->octreeTris, s->octree_tri_count * sizeof(int32_t))) return rc;
    if (int rc = upload(ctx, ctx->geo->textures, s->textures, s->texture_bytes)) return rc;
    ctx->geo->vertex_count = s->vertex_count;
    ctx->geo->normal_count = s->normal_count;
    ctx->geo->uv_count = s->uv_count;
    ctx->geo->triangle_words = s->triangle_words;
    ctx->geo->octree_count = s->octree_count;
    ctx->geo->octree_tri_count = s->octree_tri_count;
    if (int rc = build_derived_geometry(ctx, *s)) return rc;
    ctx->geo->exact_rcp_ok = rpt_scene_exact_rcp(s) == 1;
    host_mesh_facts(*ctx->geo, s, rptb::tiles::MAX_BOXES, rptb::tiles::MAX_TRIANGLES);
    ctx->bits_still = ctx->bits_tried = ctx->bits_has = 0;
    ctx->scene_uploaded = true;
    const int rc = rpt_set_objects(ctx, s->objects, (int)s->object_count);
    if (rc) ctx->scene_uploaded = false;
    return rc;
}

int rpt_share_scene(rpt_ctx *ctx, rpt_ctx *owner) {
    if (!ctx || !owner || ctx == owner) return RPT_ERR_ARG;
    if (!owner->scene_uploaded) return fail(ctx, RPT_ERR_STATE, "rpt_share_scene: the owner has no scene");
    if (ctx->device != owner->device) return fail(ctx, RPT_ERR_ARG, "rpt_share_scene: contexts are on different devices");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->geo = owner->geo;
    ctx->scene_uploaded = true;
    // (the owner's objects as ITS caller gave them: the orientation is per context, this one applies its own)
    const std::vector<uint8_t> &given = owner->oriented ? owner->caller_objects : owner->host_objects;
    const int count = (int)(given.size() / sizeof(rpt_object));
    const int rc = rpt_set_objects(ctx, count ? given.data() : nullptr, count);
    if (rc) ctx->scene_uploaded = false;
    return rc;
}

// rpt_set_objects with an orientation set (rpt_set_orientation): the caller's bytes are kept as they came, and what the context
// derives everything from, uploads and hands its test hooks is the re-based copy
static int set_objects_as_given(rpt_ctx *ctx, const void *objects, int count);
int rpt_set_objects(rpt_ctx *ctx, const void *objects, int count) {
    if (!ctx || count < 0 || (count && !objects)) return RPT_ERR_ARG;
    if (!ctx->oriented) {
        const int rc = set_objects_as_given(ctx, objects, count);
        if (rc == RPT_OK) ctx->caller_objects.clear();
        return rc;
    }
    const size_t bytes = (size_t)count * sizeof(rpt_object);
    std::vector<uint8_t> &given = ctx->given_scratch, &turned = ctx->turned_scratch;
    given.assign((const uint8_t *)objects, (const uint8_t *)objects + bytes);
    turned.resize(bytes);
    orient_objects((const rpt_object *)given.data(), count, ctx->R, (rpt_object *)turned.data());
    const int rc = set_objects_as_given(ctx, turned.data(), count);
    if (rc == RPT_OK) ctx->caller_objects.swap(given);      // (the old copy becomes next frame's scratch)
    return rc;
}

static int set_objects_as_given(rpt_ctx *ctx, const void *objects, int count) {
    if (!ctx->scene_uploaded) return fail(ctx, RPT_ERR_STATE, "rpt_set_objects before rpt_upload_scene");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = validate_objects(ctx, (const rpt_object *)objects, count)) return rc;
    const size_t bytes = (size_t)count * sizeof(rpt_object);
    const size_t dbytes = (size_t)count * (sizeof(rptd::DObj) + sizeof(rptb::Rect));     // DObj[count] then Rect[count]
    // staging ring of pinned slots: the copy of frame k may still be in flight when frame k+1 is staged, so
    // each slot has an event and is reused only once its own transfer has completed (no per-frame stream sync)
    const size_t slot_bytes = ((bytes + dbytes + 255) / 256) * 256;
    if (slot_bytes * RPT_STAGING_SLOTS > ctx->pinned_capacity) {
        RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->pinned_objects) RPT_HIP(ctx, hipHostFree(ctx->pinned_objects));
        ctx->pinned_objects = nullptr;
        ctx->pinned_capacity = 0;
        const size_t cap = (slot_bytes < 4096 ? 4096 : slot_bytes * 2) * RPT_STAGING_SLOTS;
        RPT_HIP(ctx, hipHostMalloc(&ctx->pinned_objects, cap, hipHostMallocDefault));
        ctx->pinned_capacity = cap;
        for (int k = 0; k < RPT_STAGING_SLOTS; k++)
            if (!ctx->staging_done[k]) RPT_HIP(ctx, hipEventCreateWithFlags(&ctx->staging_done[k], hipEventDisableTiming));
        ctx->staging_used = 0;
    }
    // Object[] and DObj[] live back to back in one device buffer: one transfer per frame
    if (bytes + dbytes > ctx->objects.capacity) RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (int rc = reserve(ctx, ctx->objects, bytes + dbytes)) return rc;
    if (bytes) {
        const int k = (int)(ctx->staging_next % RPT_STAGING_SLOTS);
        RPT_HOST_MARK(0);
        if (ctx->staging_used & (1u << k)) RPT_HIP(ctx, hipEventSynchronize(ctx->staging_done[k]));
        RPT_HOST_MARK(1);
        char *slot = (char *)ctx->pinned_objects + (ctx->pinned_capacity / RPT_STAGING_SLOTS) * k;
        std::memcpy(slot, objects, bytes);
        build_dobjs(ctx, (const rpt_object *)objects, count, (rptd::DObj *)(slot + bytes));
        if (ctx->windows.size() == 2 * (size_t)count)       // (another count: refused at the launch, choose_kernels)
            for (int i = 0; i < count; i++) {
                rptd::DObj &d = ((rptd::DObj *)(slot + bytes))[i];
                d.win_t0 = ctx->windows[2 * (size_t)i];
                d.win_t1 = ctx->windows[2 * (size_t)i + 1];
            }
        RPT_HOST_MARK(2);
        note_still_objects(ctx, (const rpt_object *)objects, count);
        build_rects(ctx, (const rpt_object *)objects, count, (rptb::Rect *)(slot + bytes + (size_t)count * sizeof(rptd::DObj)));
        RPT_HOST_MARK(3);
        RPT_HIP(ctx, hipMemcpyAsync(ctx->objects.ptr, slot, bytes + dbytes, hipMemcpyHostToDevice, ctx->stream));
        RPT_HOST_MARK(4);
        RPT_HIP(ctx, hipEventRecord(ctx->staging_done[k], ctx->stream));
        RPT_HOST_MARK(5);
        ctx->last_event = ctx->staging_done[k];
        ctx->staging_used |= 1u << k;
        ctx->staging_next++;
    }
    if (!bytes) ctx->bits_still = ctx->bits_tried = ctx->bits_has = 0;
    ctx->object_count = count;
    ctx->has_mesh = false;
    for (int i = 0; i < count; i++) ctx->has_mesh = ctx->has_mesh || ((const rpt_object *)objects)[i].type == RPT_MESH;
    ctx->host_objects.assign((const uint8_t *)objects, (const uint8_t *)objects + bytes);
    ctx->view_generation++;
    return RPT_OK;
}

int rpt_set_params(rpt_ctx *ctx, const float white_point[3], float ambient, int width, int height, int interval) {
    if (!ctx || !white_point) return RPT_ERR_ARG;
    if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 31) - 1) return fail(ctx, RPT_ERR_ARG, "rpt_set_params: bad resolution");
    for (int c = 0; c < 3; c++) ctx->white_point[c] = white_point[c];
    ctx->ambient = ambient;
    ctx->width = width;
    ctx->height = height;
    const bool interval_changed = ctx->interval != interval;
    ctx->interval = interval;
    ctx->params_set = true;
    ctx->view_generation++;
    if (interval_changed && ctx->scene_uploaded && ctx->object_count > 0) {
        const std::vector<uint8_t> copy = ctx->oriented ? ctx->caller_objects : ctx->host_objects;      // the culling record of DObj uses `interval`
        if (copy.size() != (size_t)ctx->object_count * sizeof(rpt_object)) return fail(ctx, RPT_ERR_STATE, "rpt_set_params: the context holds no copy of the caller's objects");
        return rpt_set_objects(ctx, copy.data(), ctx->object_count);
    }
    return RPT_OK;
}

// The windows ride in DObj::win_t0 / win_t1, which the context uploads with its Object[]: the caller's last objects are taken over again
// so that frames launched from here on see the new windows (frames in flight keep theirs: the upload is in stream order).  If that
// upload fails the setting is as it was before the call.
int rpt_set_object_windows(rpt_ctx *ctx, const float *t0t1_or_null, int count) {
    if (!ctx || count < 0) return RPT_ERR_ARG;
    if (count == 0) t0t1_or_null = nullptr;
    if (t0t1_or_null)
        for (int i = 0; i < 2 * count; i++)
            if (t0t1_or_null[i] != t0t1_or_null[i]) return fail(ctx, RPT_ERR_ARG, "rpt_set_object_windows: a bound is NaN");
    if (!t0t1_or_null && ctx->windows.empty()) return RPT_OK;
    std::vector<float> before(t0t1_or_null, t0t1_or_null ? t0t1_or_null + 2 * (size_t)count : t0t1_or_null);
    before.swap(ctx->windows);          // (`before` now holds the old setting)
    if (ctx->scene_uploaded && ctx->object_count > 0) {
        const std::vector<uint8_t> copy = ctx->oriented ? ctx->caller_objects : ctx->host_objects;
        int rc = copy.size() == (size_t)ctx->object_count * sizeof(rpt_object) ? rpt_set_objects(ctx, copy.data(), ctx->object_count)
                                                                                : fail(ctx, RPT_ERR_STATE, "rpt_set_object_windows: the context holds no copy of the caller's objects");
        if (rc != RPT_OK) {
            ctx->windows.swap(before);
            return rc;
        }
    }
    ctx->view_generation++;
    return RPT_OK;
}

int rpt_set_output(rpt_ctx *ctx, void *device_ptr_or_null) {
    if (!ctx) return RPT_ERR_ARG;
    ctx->external_out = device_ptr_or_null;
    return RPT_OK;
}

int rpt_set_rows(rpt_ctx *ctx, int first_tile, int tile_step, int colour_plane) {
    return rpt_set_tile_pattern(ctx, first_tile, tile_step, 1, colour_plane);
}

int rpt_set_tile_pattern(rpt_ctx *ctx, int first_tile, int tile_step, int run, int colour_plane) {
    if (!ctx || first_tile < 0 || tile_step < 1 || run < 1 || run > tile_step || (run & (run - 1))) return RPT_ERR_ARG;
    int lg = 0;
    while ((1 << lg) < run) lg++;
    ctx->first_tile = first_tile;
    ctx->tile_step = tile_step;
    ctx->run_log2 = lg;
    ctx->colour_plane = colour_plane != 0;
    return RPT_OK;
}

int rpt_set_stream(rpt_ctx *ctx, void *hip_stream) {
    if (!ctx) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    // drain what this context has enqueued on the stream it is leaving.  If that is an external stream the caller has
    // destroyed in the meantime, the handle is dead: the context's last launch is then waited for through its event.
    if (ctx->stream == ctx->own_stream) RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    else if (ctx->last_event) RPT_HIP(ctx, hipEventSynchronize(ctx->last_event));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return RPT_OK;
}

int rpt_set_debug_rgb(rpt_ctx *ctx, void *p) {
    if (!ctx) return RPT_ERR_ARG;
    ctx->want_owned_rgb = (p == (void *)1);
    ctx->external_rgb = ctx->want_owned_rgb ? nullptr : p;
    return RPT_OK;
}

int rpt_set_doppler(rpt_ctx *ctx, int flags) {
    if (!ctx) return RPT_ERR_ARG;
    if (flags & ~(RPT_DOPPLER_SHIFT | RPT_DOPPLER_BEAMING)) return fail(ctx, RPT_ERR_ARG, "rpt_set_doppler: flags are 0 or RPT_DOPPLER_SHIFT | RPT_DOPPLER_BEAMING");
    ctx->doppler = flags;
    return RPT_OK;
}

int rpt_set_debug_doppler(rpt_ctx *ctx, void *p) {
    if (!ctx) return RPT_ERR_ARG;
    ctx->want_owned_doppler = (p == (void *)1);
    ctx->external_doppler = ctx->want_owned_doppler ? nullptr : p;
    return RPT_OK;
}

int rpt_set_projection(rpt_ctx *ctx, int mode, const float *params) {
    if (!ctx) return RPT_ERR_ARG;
    float p[3] = {0, 0, 0};
    if (mode == RPT_PROJECTION_PINHOLE) {
        if (params) return fail(ctx, RPT_ERR_ARG, "rpt_set_projection: RPT_PROJECTION_PINHOLE takes no parameters (NULL)");
    } else if (mode == RPT_PROJECTION_EQUIRECT) {
        if (!projection_params(params, p))
            return fail(ctx, RPT_ERR_ARG, "rpt_set_projection: equirect parameters are {h_fov in (0, 2 pi], v_fov in (0, pi], finite yaw} in radians, or NULL");
    } else if (mode == RPT_PROJECTION_RAYMAP) {
        if (params) return fail(ctx, RPT_ERR_ARG, "rpt_set_projection: RPT_PROJECTION_RAYMAP takes no parameters (NULL): the directions are the context's map (rpt_set_raymap)");
        // (the number was no mode before the ray map existed, and a context that has no map still has no such camera; a map that is
        // dropped LATER, or one of another size, is what the launch refuses)
        if (!ctx->raymap_on) return fail(ctx, RPT_ERR_ARG, "rpt_set_projection: RPT_PROJECTION_RAYMAP needs the context's ray map: call rpt_set_raymap first");
    } else {
        return fail(ctx, RPT_ERR_ARG, "rpt_set_projection: mode is RPT_PROJECTION_PINHOLE, RPT_PROJECTION_EQUIRECT or RPT_PROJECTION_RAYMAP");
    }
    ctx->projection = mode;
    std::memcpy(ctx->projection_params, p, sizeof p);
    ctx->view_generation++;
    return RPT_OK;
}

int rpt_projection_tables(int mode, const float *params, int width, int height, float *cols_out, float *rows_out) {
    float p[3];
    if (mode != RPT_PROJECTION_EQUIRECT || !projection_params(params, p)) return RPT_ERR_ARG;
    if (width <= 0 || height <= 0 || (long long)width * height > (1ll << 31) - 1 || !cols_out || !rows_out) return RPT_ERR_ARG;
    projection_fill(p, width, height, cols_out, rows_out);
    return RPT_OK;
}

// ---- the ray-map camera (rpt_set_raymap, rpt_raymap_fill) ----------------------------------------------------------------------------
// The map goes to the device as one float4 per pixel in rows of the width rounded up to 8 pixels (rpt_kernels.hip.h: RaymapArgs), in
// stream order from a pinned buffer that is not rewritten before its previous copy has run (the sky image's discipline): a frame still
// in flight reads the map it was launched with, a later one the new map.  Dropping the map frees nothing (rpt_destroy does).
int rpt_set_raymap(rpt_ctx *ctx, const float *dirs3, int width, int height) {
    if (!ctx) return RPT_ERR_ARG;
    if (!dirs3) {
        ctx->raymap_on = false;
        ctx->view_generation++;
        return RPT_OK;
    }
    if (width < 1 || height < 1 || 3ll * width * height >= (1ll << 31))
        return fail(ctx, RPT_ERR_ARG, "rpt_set_raymap: width and height are >= 1 and 3 width height < 2^31");
    const size_t n = 3 * (size_t)width * (size_t)height;
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(dirs3[i])) return fail(ctx, RPT_ERR_ARG, "rpt_set_raymap: component " + std::to_string(i) + " of the map is not finite");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t pitch = ((size_t)width + 7) & ~(size_t)7, bytes = pitch * (size_t)height * 4 * sizeof(float);
    ctx->raymap_on = false;      // (until the new map is in place)
    float *host = nullptr;
    if (int rc = staged_host(ctx, ctx->raymap, bytes, (void **)&host)) return rc;
    for (int y = 0; y < height; y++) {
        float *row = host + (size_t)y * pitch * 4;
        const float *src = dirs3 + 3 * (size_t)y * (size_t)width;
        for (int x = 0; x < width; x++) {
            row[4 * (size_t)x] = src[3 * (size_t)x];
            row[4 * (size_t)x + 1] = src[3 * (size_t)x + 1];
            row[4 * (size_t)x + 2] = src[3 * (size_t)x + 2];
            row[4 * (size_t)x + 3] = 0.0f;
        }
        for (size_t k = 4 * (size_t)width; k < 4 * pitch; k++) row[k] = 0.0f;
    }
    if (int rc = staged_copy(ctx, ctx->raymap)) return rc;
    ctx->raymap_width = width;
    ctx->raymap_height = height;
    ctx->raymap_pitch = (int)pitch;
    ctx->raymap_on = true;
    ctx->view_generation++;
    return RPT_OK;
}

// Host code, no device.  Everything in double from the float parameters, one rounding to float per component.
int rpt_raymap_fill(int kind, const float *params, int width, int height, float *dirs3_out) {
    if (width < 1 || height < 1 || 3ll * width * height >= (1ll << 31) || !dirs3_out) return RPT_ERR_ARG;
    const double W = width, H = height;
    if (kind == RPT_RAYMAP_CUBE_STRIP) {
        if (params || (long long)width != 6ll * height) return RPT_ERR_ARG;
        // face f: p = forward + a right + b up, a and b the face's pinhole coordinates in (-1, 1) — a 90-degree lens
        static const double forward[6][3] = {{1, 0, 0}, {-1, 0, 0}, {0, 1, 0}, {0, -1, 0}, {0, 0, 1}, {0, 0, -1}};
        static const double right[6][3] = {{0, 0, -1}, {0, 0, 1}, {1, 0, 0}, {1, 0, 0}, {1, 0, 0}, {-1, 0, 0}};
        static const double up[6][3] = {{0, 1, 0}, {0, 1, 0}, {0, 0, -1}, {0, 0, 1}, {0, 1, 0}, {0, 1, 0}};
        for (int y = 0; y < height; y++) {
            const double b = (2.0 * ((double)y + 0.5) - H) / H;
            for (int x = 0; x < width; x++) {
                const int f = x / height;
                const double a = (2.0 * ((double)(x - f * height) + 0.5) - H) / H;
                float *o = dirs3_out + 3 * ((size_t)y * (size_t)width + (size_t)x);
                for (int k = 0; k < 3; k++) o[k] = (float)(forward[f][k] + a * right[f][k] + b * up[f][k]);
            }
        }
        return RPT_OK;
    }
    if (kind != RPT_RAYMAP_FISHEYE && kind != RPT_RAYMAP_FISHEYE_EQUISOLID && kind != RPT_RAYMAP_STEREOGRAPHIC) return RPT_ERR_ARG;
    if (!params) return RPT_ERR_ARG;
    const float fov_f = params[0], fit_f = params[1];
    const float two_pi = (float)(2.0 * RPT_PI_D);
    if (!(fov_f > 0.0f && fov_f <= two_pi) || (kind == RPT_RAYMAP_STEREOGRAPHIC && !(fov_f < two_pi))) return RPT_ERR_ARG;
    if (fit_f != 0.0f && fit_f != 1.0f) return RPT_ERR_ARG;
    const double fov = fov_f, S = fit_f == 0.0f ? (W < H ? W : H) : std::sqrt(W * W + H * H);
    for (int y = 0; y < height; y++) {
        const double Y = (2.0 * ((double)y + 0.5) - H) / S;
        for (int x = 0; x < width; x++) {
            const double X = (2.0 * ((double)x + 0.5) - W) / S;
            const double rho = std::sqrt(X * X + Y * Y);
            float *o = dirs3_out + 3 * ((size_t)y * (size_t)width + (size_t)x);
            if (rho > 1.0) {
                o[0] = o[1] = o[2] = 0.0f;
                continue;
            }
            if (rho == 0.0) {
                o[0] = o[1] = 0.0f;
                o[2] = 1.0f;
                continue;
            }
            double theta;
            if (kind == RPT_RAYMAP_FISHEYE) theta = rho * fov / 2.0;
            else if (kind == RPT_RAYMAP_FISHEYE_EQUISOLID) theta = 2.0 * std::asin(rho * std::sin(fov / 4.0));
            else theta = 2.0 * std::atan(rho * std::tan(fov / 4.0));
            const double st = std::sin(theta);
            o[0] = (float)(st * X / rho);
            o[1] = (float)(st * Y / rho);
            o[2] = (float)std::cos(theta);
        }
    }
    return RPT_OK;
}

// The image goes to the device as one dword per texel, in stream order from a pinned buffer that is not rewritten before its previous
// copy has run (the panorama tables' discipline): a frame still in flight reads the image it was launched with, a later one the new
// one.  Switching off frees nothing (rpt_destroy does), so it cannot pull the image from under a frame either.
int rpt_set_environment(rpt_ctx *ctx, const unsigned char *rgb8, int width, int height) {
    if (!ctx) return RPT_ERR_ARG;
    if (!rgb8) {
        ctx->env_on = false;
        return RPT_OK;
    }
    if (width < 1 || height < 1 || 3ll * width * height >= (1ll << 31))
        return fail(ctx, RPT_ERR_ARG, "rpt_set_environment: width and height are >= 1 and 3 width height < 2^31");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t texels = (size_t)width * (size_t)height, bytes = texels * sizeof(uint32_t);
    ctx->env_on = false;         // (until the new image is in place)
    uint32_t *host = nullptr;
    if (int rc = staged_host(ctx, ctx->env, bytes, (void **)&host)) return rc;
    for (size_t i = 0; i < texels; i++)
        host[i] = (uint32_t)rgb8[3 * i] | ((uint32_t)rgb8[3 * i + 1] << 8) | ((uint32_t)rgb8[3 * i + 2] << 16);
    if (int rc = staged_copy(ctx, ctx->env)) return rc;
    ctx->env_width = width;
    ctx->env_height = height;
    ctx->env_on = true;
    return RPT_OK;
}

int rpt_set_environment_frame(rpt_ctx *ctx, const float lorentz[16]) {
    if (!ctx) return RPT_ERR_ARG;
    static const float identity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    const float *m = lorentz ? lorentz : identity;
    for (int k = 0; k < 16; k++)
        if (!std::isfinite(m[k])) return fail(ctx, RPT_ERR_ARG, "rpt_set_environment_frame: every entry must be finite");
    std::memcpy(ctx->env_frame, m, sizeof ctx->env_frame);
    return RPT_OK;
}

int rpt_set_orientation(rpt_ctx *ctx, const float ypr[3]) {
    if (!ctx) return RPT_ERR_ARG;
    double R[3][3];
    if (!orientation_matrix(ypr, R)) return fail(ctx, RPT_ERR_ARG, "rpt_set_orientation: yaw, pitch and roll must be finite (radians), or NULL");
    // the caller's last Object[], as given, BEFORE the setting changes (host_objects holds it while no orientation is set)
    const std::vector<uint8_t> given = ctx->oriented ? ctx->caller_objects : ctx->host_objects;
    const bool was_oriented = ctx->oriented;
    double was_R[3][3];
    std::memcpy(was_R, ctx->R, sizeof was_R);
    ctx->oriented = !is_identity(R);
    std::memcpy(ctx->R, R, sizeof R);
    ctx->view_generation++;
    if (!ctx->scene_uploaded || ctx->object_count <= 0) return RPT_OK;
    if (given.size() != (size_t)ctx->object_count * sizeof(rpt_object)) {      // (cannot happen: every successful rpt_set_objects leaves the copy that matches `oriented`)
        ctx->oriented = was_oriented;
        std::memcpy(ctx->R, was_R, sizeof was_R);
        return fail(ctx, RPT_ERR_STATE, "rpt_set_orientation: the context holds no copy of the caller's objects to re-derive from");
    }
    const int rc = rpt_set_objects(ctx, given.data(), ctx->object_count);      // re-derive regions, proofs, records and the upload at once
    if (rc != RPT_OK) {          // nothing was taken over: the setting goes back with it, so `oriented`, host_objects and caller_objects still match
        ctx->oriented = was_oriented;
        std::memcpy(ctx->R, was_R, sizeof was_R);
    }
    return rc;
}

int rpt_set_field_of_view(rpt_ctx *ctx, float v_fov) {
    if (!ctx) return RPT_ERR_ARG;
    if (v_fov != 0.0f && !(v_fov >= 0.01f && v_fov <= 3.0f))
        return fail(ctx, RPT_ERR_ARG, "rpt_set_field_of_view: the vertical field of view is 0 (the reference's lens) or 0.01 <= v_fov <= 3.0 radians");
    ctx->v_fov = v_fov;
    ctx->lens_scale = v_fov != 0.0f ? (float)std::tan(0.5 * (double)v_fov) : 1.0f;
    ctx->view_generation++;
    return RPT_OK;
}

int rpt_orient_objects(const void *objects_in, int count, const float ypr[3], void *objects_out) {
    double R[3][3];
    if (count < 0 || (count && (!objects_in || !objects_out)) || !orientation_matrix(ypr, R)) return RPT_ERR_ARG;
    orient_objects((const rpt_object *)objects_in, count, R, (rpt_object *)objects_out);
    return RPT_OK;
}

int rpt_orient_matrix(const float lorentz_in[16], const float ypr[3], float lorentz_out[16]) {
    double R[3][3];
    if (!lorentz_in || !lorentz_out || !orientation_matrix(ypr, R)) return RPT_ERR_ARG;
    rpt_float4 m[4];
    std::memcpy(m, lorentz_in, sizeof m);
    if (!is_identity(R)) rebase_columns(m, R, m);
    std::memcpy(lorentz_out, m, sizeof m);
    return RPT_OK;
}

int rpt_read_debug_doppler(rpt_ctx *ctx, void *host_dst, size_t bytes) {
    if (!ctx || !host_dst) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const void *src = ctx->external_doppler ? ctx->external_doppler : (ctx->want_owned_doppler ? ctx->owned_doppler.ptr : nullptr);
    if (!src || !ctx->colour_frame.rendered() || !ctx->doppler_recorded)
        return fail(ctx, RPT_ERR_STATE, "rpt_read_debug_doppler: the last frame was not rendered with Doppler on and the record hook set");
    if (bytes > (size_t)ctx->width * ctx->height * RPT_DOPPLER_RECORD * sizeof(float)) return fail(ctx, RPT_ERR_ARG, "rpt_read_debug_doppler: too many bytes");
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RPT_HIP(ctx, hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_object_screen_rect(const void *object, int interval, const float *root_bounds_or_null, float rect_out[4]) {
    if (!object || !rect_out) return RPT_ERR_ARG;
    const rptb::Rect r = rptb::certified_object_rect(*(const rpt_object *)object, interval, root_bounds_or_null);
    rect_out[0] = r.u0; rect_out[1] = r.v0; rect_out[2] = r.u1; rect_out[3] = r.v1;
    return RPT_OK;
}

int rpt_object_screen_bounds(const void *object, int interval, const float *root_bounds_or_null, float bounds_out[8]) {
    if (!object || !bounds_out) return RPT_ERR_ARG;
    const rptb::Rect r = rptb::certified_object_rect(*(const rpt_object *)object, interval, root_bounds_or_null);
    const float v[8] = {r.u0, r.v0, r.u1, r.v1, r.p_lo, r.p_hi, r.m_lo, r.m_hi};
    for (int k = 0; k < 8; k++) bounds_out[k] = v[k];
    return RPT_OK;
}

int rpt_mesh_segment_cull_record(rpt_ctx *ctx, int object_index, float out[10]) {
    if (!ctx || !out || object_index < 0 || (size_t)(object_index + 1) * sizeof(rpt_object) > ctx->host_objects.size()) return RPT_ERR_ARG;
    const rpt_object *objs = (const rpt_object *)ctx->host_objects.data();
    std::vector<rptd::DObj> d((size_t)object_index + 1);
    build_dobjs(ctx, objs, object_index + 1, d.data());
    const rptd::DObj &r = d[(size_t)object_index];
    const int mi = objs[object_index].meshIndex;
    const bool known = objs[object_index].type == RPT_MESH && mi >= 0 && (size_t)mi < ctx->geo->node_tri_K.size();
    for (int k = 0; k < 3; k++) out[k] = r.mh[k];
    out[3] = r.mconst; out[4] = r.mslope; out[5] = r.mcw; out[6] = r.ms0;
    out[7] = known ? ctx->geo->node_tri_K[(size_t)mi] : 0.0f;
    out[8] = known ? ctx->geo->node_tri_L[(size_t)mi] : 0.0f;
    out[9] = r.mesh_in_box;
    return RPT_OK;
}

int rpt_object_screen_bounds_proposed(const void *object, int interval, const float *root_bounds_or_null, float bounds_out[8]) {
    if (!object || !bounds_out) return RPT_ERR_ARG;
    const rptb::Rect r = rptb::proposed_object_rect(*(const rpt_object *)object, interval, root_bounds_or_null);
    const float v[8] = {r.u0, r.v0, r.u1, r.v1, r.p_lo, r.p_hi, r.m_lo, r.m_hi};
    for (int k = 0; k < 8; k++) bounds_out[k] = v[k];
    return RPT_OK;
}

int rpt_certify_screen_bounds(const void *object, int interval, const float *root_bounds_or_null, const float bounds[8], int stats_out[4]) {
    if (!object || !bounds) return RPT_ERR_ARG;
    const rptb::Rect r{bounds[0], bounds[1], bounds[2], bounds[3], bounds[4], bounds[5], bounds[6], bounds[7]};
    rptb::cert::Stats st{0, 0, 0, 0};
    const bool ok = rptb::cert::certify(*(const rpt_object *)object, interval, root_bounds_or_null, r, &st);
    if (stats_out) { stats_out[0] = st.reason; stats_out[1] = st.tests; stats_out[2] = st.max_depth; stats_out[3] = st.segments; }
    return ok ? 1 : 0;
}

// The tile bitmap of mesh object `object_index` of `scene` (its Object[] as it stands) for a frame, on the host alone: what a context
// would put on the device for the same object, frame and lens.  boxes_or_null: n_boxes sub-tree boxes to use INSTEAD of the mesh's own
// (tests: a broken box must never clear a tile).  1: built; 0: this object gets no bitmap; < 0: an error.
// stats_out: boxes, boxes proven, tiles set, tiles, the depth of the cut — of the SUB-TREE stage; bits_out is the product with the triangle
// stage (RPT_TILE_TRIANGLES as a context created now would read it: read on EVERY call here, there is no context to have read it), except
// with the caller's boxes: those are the whole input then.
int rpt_tile_bitmap_host(const rpt_scene_desc *s, int object_index, int interval, int width, int height, float lens_scale, int max_boxes,
                         const float *boxes_or_null, int n_boxes, uint32_t *bits_out, size_t words, int stats_out[5]) {
    if (!s || !bits_out || object_index < 0 || (size_t)object_index >= s->object_count || width < 1 || height < 1 || max_boxes < 1) return -RPT_ERR_ARG;
    if (words < rptb::tiles::bitmap_words(width, height)) return -RPT_ERR_ARG;
    rpt_ctx tmp;
    if (validate_geometry(&tmp, *s) != RPT_OK) return -RPT_ERR_SCENE;
    const rpt_object &o = s->objects[object_index];
    if (o.type == RPT_MESH && (o.meshIndex < 0 || (size_t)o.meshIndex >= s->octree_count)) return -RPT_ERR_SCENE;
    tmp.geo = std::make_shared<Geometry>();
    tmp.geo->compact_ok = true;
    tmp.geo->octree_count = s->octree_count;
    const bool callers = boxes_or_null && n_boxes > 0;
    tmp.tile_triangles = tile_triangles_wanted() && !callers;
    host_mesh_facts(*tmp.geo, s, max_boxes, tmp.tile_triangles ? rptb::tiles::MAX_TRIANGLES : 0);
    int depth = -1;
    if (o.type == RPT_MESH) {
        std::vector<float> own;
        if (tmp.geo->mesh_boxes.count(o.meshIndex)) rptb::tiles::subtree_boxes(*s, o.meshIndex, max_boxes, own, &depth);
        if (callers && tmp.geo->mesh_boxes.count(o.meshIndex)) tmp.geo->mesh_boxes[o.meshIndex].assign(boxes_or_null, boxes_or_null + 6 * (size_t)n_boxes);
    }
    tmp.interval = interval;
    tmp.width = width;
    tmp.height = height;
    tmp.v_fov = lens_scale == 1.0f ? 0.0f : 1.0f;       // (only "a lens is set" is read from it)
    tmp.lens_scale = lens_scale;
    rptb::tiles::Stats st{0, 0, 0, 0};
    if (!window_holds_frame(&tmp)) return 0;
    const bool ok = build_tile_bitmap(&tmp, o, bits_out, &st);
    if (stats_out) { stats_out[0] = st.boxes; stats_out[1] = st.proven; stats_out[2] = st.tiles_set; stats_out[3] = st.tiles; stats_out[4] = depth; }
    return ok ? 1 : 0;
}

// One stage of the tile bitmap alone, on the host: stage 0 the sub-tree stage (the mesh's own cut, at most 64 boxes), stage 1 the triangle
// stage with at most `max_triangles` distinct triangles; stage 2 their product under that cap (a mesh over it: the sub-tree stage), with
// the sub-tree stage's statistics.  rpt_tile_bitmap_host's returns; stats_out: boxes, boxes proven, tiles set, tiles.
int rpt_tile_bitmap_stage_host(const rpt_scene_desc *s, int object_index, int interval, int width, int height, float lens_scale, int stage, int max_triangles,
                               uint32_t *bits_out, size_t words, int stats_out[4]) {
    if (!s || !bits_out || object_index < 0 || (size_t)object_index >= s->object_count || width < 1 || height < 1 || stage < 0 || stage > 2 || max_triangles < 1) return -RPT_ERR_ARG;
    if (words < rptb::tiles::bitmap_words(width, height)) return -RPT_ERR_ARG;
    rpt_ctx tmp;
    if (validate_geometry(&tmp, *s) != RPT_OK) return -RPT_ERR_SCENE;
    const rpt_object &o = s->objects[object_index];
    if (o.type == RPT_MESH && (o.meshIndex < 0 || (size_t)o.meshIndex >= s->octree_count)) return -RPT_ERR_SCENE;
    tmp.geo = std::make_shared<Geometry>();
    tmp.geo->compact_ok = true;
    tmp.geo->octree_count = s->octree_count;
    host_mesh_facts(*tmp.geo, s, rptb::tiles::MAX_BOXES, stage >= 1 ? max_triangles : 0);
    tmp.interval = interval;
    tmp.width = width;
    tmp.height = height;
    tmp.v_fov = lens_scale == 1.0f ? 0.0f : 1.0f;       // (only "a lens is set" is read from it)
    tmp.lens_scale = lens_scale;
    rptb::tiles::Stats st{0, 0, 0, 0};
    if (!window_holds_frame(&tmp)) return 0;
    const bool ok = build_tile_bitmap(&tmp, o, bits_out, &st, stage == 2 ? -1 : stage);
    if (stats_out) { stats_out[0] = st.boxes; stats_out[1] = st.proven; stats_out[2] = st.tiles_set; stats_out[3] = st.tiles; }
    return ok ? 1 : 0;
}

// The bitmap's rasterisation alone (tests): the tiles of a width x height frame whose grown square touches the region bounds[8] =
// {u0, v0, u1, v1, p_lo, p_hi, m_lo, m_hi}, octagon sides only with `diagonals`.  1: done; 0: an empty or NaN region (nothing set).
int rpt_tile_rasterise_host(int width, int height, float lens_scale, int diagonals, const float bounds[8], uint32_t *bits_out, size_t words) {
    if (!bounds || !bits_out || width < 1 || height < 1 || !(lens_scale > 0.0f) || words < rptb::tiles::bitmap_words(width, height)) return -RPT_ERR_ARG;
    for (size_t k = 0; k < words; k++) bits_out[k] = 0u;
    const rptb::Rect r{bounds[0], bounds[1], bounds[2], bounds[3], bounds[4], bounds[5], bounds[6], bounds[7]};
    if (!(r.u0 <= r.u1) || !(r.v0 <= r.v1)) return 0;
    const rptb::tiles::Frame f{width, height, lens_scale, diagonals != 0};
    rptb::tiles::rasterise(r, diagonals != 0, rptb::tiles::Grid(f), bits_out);
    return 1;
}

// The derived layouts of `scene` on the host alone: what build_derived_geometry uploads, array by array (include/rpt.h).
int rpt_derived_layout_host(const rpt_scene_desc *s, int which, void *out, size_t bytes, size_t *bytes_needed) {
    if (!s || which < RPT_LAYOUT_NODES || which > RPT_LAYOUT_NODE_INDEX) return -RPT_ERR_ARG;
    rpt_ctx tmp;
    if (validate_geometry(&tmp, *s) != RPT_OK) return -RPT_ERR_SCENE;
    if (s->octree_count == 0) return 0;
    Geometry g;
    DerivedLayouts L;
    if (!derive_layouts(g, *s, L)) return 0;
    const void *src = which == RPT_LAYOUT_NODES ? (const void *)L.nodes.data() : which == RPT_LAYOUT_EXITS ? (const void *)L.exits.data()
                    : which == RPT_LAYOUT_HITS ? (const void *)L.hits.data() : (const void *)g.node_new_index.data();
    const size_t need = which == RPT_LAYOUT_NODES ? L.nodes.size() * sizeof(rptd::DNode) : which == RPT_LAYOUT_EXITS ? L.exits.size() * sizeof(rptd::DExit)
                      : which == RPT_LAYOUT_HITS ? L.hits.size() * sizeof(rptd::DHit) : g.node_new_index.size() * sizeof(int);
    if (bytes_needed) *bytes_needed = need;
    if (out) {
        if (bytes < need) return -RPT_ERR_ARG;
        if (need) std::memcpy(out, src, need);
    }
    return 1;
}

// The context's tile bitmaps: out = {objects that have one on the device for the current frame, bitmaps built so far, host
// microseconds of the last build, dwords per bitmap}; bits_or_null: the bitmap of `object_index` (the pinned copy the device's was made from)
int rpt_tile_bitmap_state(rpt_ctx *ctx, unsigned long long out[4], int object_index, uint32_t *bits_or_null, size_t words) {
    if (!ctx || !out) return RPT_ERR_ARG;
    const bool current = ctx->params_set && tile_bits_current(ctx);
    const size_t w = ctx->params_set ? rptb::tiles::bitmap_words(ctx->width, ctx->height) : 0;
    out[0] = current ? ctx->bits_has : 0ull;
    out[1] = ctx->bits_builds;
    out[2] = (unsigned long long)(ctx->bits_last_build_us + 0.5);
    out[3] = w;
    if (bits_or_null) {
        if (!current || object_index < 0 || object_index >= 64 || !(ctx->bits_has >> object_index & 1ull) || words < w || !ctx->tile_bits.host) return fail(ctx, RPT_ERR_ARG, "rpt_tile_bitmap_state: no bitmap for this object");
        RPT_HIP(ctx, hipEventSynchronize(ctx->tile_bits.copied));
        std::memcpy(bits_or_null, (const uint32_t *)ctx->tile_bits.host + (size_t)object_index * w, w * 4);
    }
    return RPT_OK;
}

// The bitmap cache of the context's scene (tests, diagnostics): out = {keys built, requests answered with a copy} since its upload
int rpt_tile_bitmap_shared_state(rpt_ctx *ctx, unsigned long long out[2]) {
    if (!ctx || !out) return RPT_ERR_ARG;
    std::lock_guard<std::mutex> lock(ctx->geo->bitmap_cache_lock);
    out[0] = ctx->geo->bitmap_builds;
    out[1] = ctx->geo->bitmap_copies;
    return RPT_OK;
}

// The object mask of every 8x8 tile of the current frame as the device forms it: out[2 t] before and out[2 t + 1] after the tile
// bitmaps, t = ty * ceil(width / 8) + tx.  Prepares the frame as a launch does (a still mesh gets its bitmap here as there).
int rpt_probe_tile_masks(rpt_ctx *ctx, unsigned long long *out, size_t tiles) {
    if (!ctx || !out) return RPT_ERR_ARG;
    if (!ctx->scene_uploaded || !ctx->params_set) return fail(ctx, RPT_ERR_STATE, "rpt_probe_tile_masks before rpt_upload_scene / rpt_set_params");
    if (ctx->projection != RPT_PROJECTION_PINHOLE || !window_holds_frame(ctx)) return fail(ctx, RPT_ERR_ARG, "rpt_probe_tile_masks: this frame is not rendered with the object mask");
    const int tx = (ctx->width + 7) / 8, ty = (ctx->height + 7) / 8;
    if (tiles != (size_t)tx * ty) return fail(ctx, RPT_ERR_ARG, "rpt_probe_tile_masks: tiles != ceil(width / 8) * ceil(height / 8)");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    if (int rc = ensure_tile_bits(ctx)) return rc;
    rptd::LensArgs a;
    fill_frame_args(ctx, a);
    unsigned long long *d_out = nullptr;
    RPT_HIP(ctx, hipMalloc((void **)&d_out, tiles * 16));
    hipLaunchKernelGGL(rptd::rpt_probe_tile_masks_kernel, dim3(tx, ty), dim3(64), 0, ctx->stream, a, ctx->v_fov != 0.0f ? 1 : 0, d_out);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, tiles * 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(ctx, RPT_ERR_DEVICE, std::string("rpt_probe_tile_masks: ") + hipGetErrorString(e));
    return RPT_OK;
}

int rpt_set_variant(rpt_ctx *ctx, int variant) {
    if (!ctx) return RPT_ERR_ARG;
#ifndef RPT_DIAGNOSTICS     /* the diagnostics library knows many more (rpt_diag_kernels.hip.h); an unknown number fails at the launch */
    if (variant != 0 && settable_form(variant) == Form::diagnostic)
        return fail(ctx, RPT_ERR_ARG, "rpt_set_variant: unknown variant (measurement arms and instrumented kernels exist in librpt_hip_diag.so only)");
#endif
    ctx->variant = variant;
    return RPT_OK;
}

int rpt_last_variant(const rpt_ctx *ctx) { return ctx ? ctx->last_variant : 0; }
int rpt_last_exact_rcp(const rpt_ctx *ctx) { return ctx && ctx->last_exact_rcp ? 1 : 0; }
int rpt_last_sky_split(const rpt_ctx *ctx, int rect[4]) {
    const bool split = ctx && ctx->last_sky_split;
    if (rect)
        for (int k = 0; k < 4; k++) rect[k] = split ? ctx->last_sky_box[k] : 0;
    return split ? 1 : 0;
}

// The domain of the triangle test's exact reciprocal (rcp_exact, intersect_triangle_edges<true>): |det| <= |e1| |e2| (1 + 2^-20) for
// a normalised direction, and rcp_exact equals 1 / det for 1e-7 <= |det| <= 2^125.  Asked here: |e1| |e2| <= 2^60 for every triangle a
// walk tests (those the octrees' lists name), e1 = fl(B - A) and e2 = fl(C - A) as the derived records hold them; a non-finite
// vertex fails.  The margin (2^60 against 2^125) makes the double-precision product's rounding irrelevant.
int rpt_scene_exact_rcp(const rpt_scene_desc *s) {
    if (!s || (s->vertex_count && !s->vertices) || (s->triangle_words && !s->triangles) || (s->octree_tri_count && !s->octreeTris)) return -RPT_ERR_ARG;
    const size_t n_tris = s->triangle_words / RPT_TRI_STRIDE;
    const double limit = 0x1p60;
    for (size_t i = 0; i < s->octree_tri_count; i++) {
        const int t = s->octreeTris[i];
        if (t < 0 || (size_t)t >= n_tris) return -RPT_ERR_SCENE;
        const rpt_float3 *vv[3];
        for (int c = 0; c < 3; c++) {
            const uint32_t w = s->triangles[9 * (size_t)t + 3 * c];
            if (w >= s->vertex_count) return -RPT_ERR_SCENE;
            vv[c] = &s->vertices[w];
        }
        const float e1[3] = {vv[1]->x - vv[0]->x, vv[1]->y - vv[0]->y, vv[1]->z - vv[0]->z}, e2[3] = {vv[2]->x - vv[0]->x, vv[2]->y - vv[0]->y, vv[2]->z - vv[0]->z};
        const double l1 = std::sqrt((double)e1[0] * e1[0] + (double)e1[1] * e1[1] + (double)e1[2] * e1[2]);
        const double l2 = std::sqrt((double)e2[0] * e2[0] + (double)e2[1] * e2[1] + (double)e2[2] * e2[2]);
        if (!(l1 * l2 <= limit)) return 0;      // (NaN and inf fail too)
    }
    return 1;
}

int rpt_set_msaa(rpt_ctx *ctx, int samples_per_axis) {
    if (!ctx) return RPT_ERR_ARG;
    if (samples_per_axis < 1 || samples_per_axis > 8) return fail(ctx, RPT_ERR_ARG, "rpt_set_msaa: 1..8 samples per axis");
    ctx->msaa = samples_per_axis;
    return RPT_OK;
}

int rpt_verify_frame(rpt_ctx *ctx, unsigned long long *differing_pixels) {
    if (!ctx || !differing_pixels) return RPT_ERR_ARG;
    if (!ctx->scene_uploaded) return fail(ctx, RPT_ERR_STATE, "rpt_verify_frame before rpt_upload_scene");
    if (!ctx->params_set) return fail(ctx, RPT_ERR_STATE, "rpt_verify_frame before rpt_set_params");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t words = (size_t)local_tile_count(ctx) * RPT_TILE_ROWS * ctx->width;
    if (int rc = reserve(ctx, ctx->verify_planes, 2 * words * 4 + 8)) return rc;
    uint32_t *plane_a = (uint32_t *)ctx->verify_planes.ptr, *plane_b = plane_a + words;
    unsigned long long *count = (unsigned long long *)(plane_b + words);
    RPT_HIP(ctx, hipMemsetAsync(plane_a, 0, 2 * words * 4 + 8, ctx->stream));     // (rows of the last tile beyond the frame's height are never written)
    // render twice into the scratch planes: the kernel a frame would get, then the un-culled one; the context's own outputs,
    // its variant and its debug hook are put back whatever happens
    struct Saved { void *plane, *rgb, *dop; bool colour_plane, want_rgb, want_dop, dop_recorded; int variant; } saved = {ctx->external_plane, ctx->external_rgb, ctx->external_doppler, ctx->colour_plane, ctx->want_owned_rgb, ctx->want_owned_doppler, ctx->doppler_recorded, ctx->variant};
    ctx->colour_plane = true;
    ctx->external_rgb = nullptr;
    ctx->want_owned_rgb = false;
    ctx->external_doppler = nullptr;         // (with Doppler on: the twin a frame would get against the un-culled twin, 203)
    ctx->want_owned_doppler = false;
    int rc = RPT_OK;
    ctx->external_plane = plane_a;
    rc = launch(ctx, Call{CallKind::in_flight, false});
    const int verified_variant = ctx->last_variant;      // what rpt_last_variant reports afterwards: the kernel that was CHECKED, not the un-culled one
    // (both launches write colour planes, which are never split: rpt_last_sky_split reports "one launch" afterwards, of that same checked launch)
    if (rc == RPT_OK) {
        ctx->external_plane = plane_b;
        ctx->variant = 3;
        rc = launch(ctx, Call{CallKind::in_flight, false});
    }
    ctx->last_variant = verified_variant;
    ctx->external_plane = saved.plane; ctx->external_rgb = saved.rgb; ctx->colour_plane = saved.colour_plane; ctx->want_owned_rgb = saved.want_rgb; ctx->variant = saved.variant;
    ctx->external_doppler = saved.dop; ctx->want_owned_doppler = saved.want_dop; ctx->doppler_recorded = saved.dop_recorded;
    if (rc != RPT_OK) return rc;
    if (words) {
        const unsigned int blocks = (unsigned int)std::min<size_t>((words + 255) / 256, 4096);
        hipLaunchKernelGGL(rptd::rpt_count_differences_kernel, dim3(blocks), dim3(256), 0, ctx->stream, plane_a, plane_b, words, count);
        RPT_HIP(ctx, hipGetLastError());
    }
    RPT_HIP(ctx, hipMemcpyAsync(differing_pixels, count, 8, hipMemcpyDeviceToHost, ctx->stream));
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return RPT_OK;
}

// One colour frame between its two events: rpt_render_async, and rpt_render before it waits
static int render_frame(rpt_ctx *ctx, CallKind kind) {
    if (!ctx) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    hipEvent_t eb = ctx->ev_begin, ee = ctx->ev_end;
    const bool timed = ctx->timing_frames >= 0 && (size_t)(2 * ctx->timing_frames + 1) < ctx->timing_events.size();
    if (timed) {
        eb = ctx->timing_events[2 * ctx->timing_frames];
        ee = ctx->timing_events[2 * ctx->timing_frames + 1];
    }
    RPT_HIP(ctx, hipEventRecord(eb, ctx->stream));
    if (int rc = launch(ctx, Call{kind, true})) return rc;
    RPT_HIP(ctx, hipEventRecord(ee, ctx->stream));
    ctx->last_event = ee;
    if (timed) ctx->timing_frames++;
    else if (ctx->timing_frames >= 0) return fail(ctx, RPT_ERR_STATE, "timing region is full");
    mark_colour_frame(ctx);
    return RPT_OK;
}

int rpt_render_async(rpt_ctx *ctx) { return render_frame(ctx, CallKind::in_flight); }

int rpt_timing_begin(rpt_ctx *ctx, int max_frames) {
    if (!ctx || max_frames <= 0 || max_frames > (1 << 20)) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    while (ctx->timing_events.size() < (size_t)(2 * max_frames)) {
        hipEvent_t e = nullptr;
        RPT_HIP(ctx, hipEventCreate(&e));
        ctx->timing_events.push_back(e);
    }
    ctx->timing_frames = 0;
    return RPT_OK;
}

int rpt_timing_end(rpt_ctx *ctx, float *total_ms, int *frames) {
    if (!ctx || !total_ms || !frames) return RPT_ERR_ARG;
    if (ctx->timing_frames < 0) return fail(ctx, RPT_ERR_STATE, "rpt_timing_end without rpt_timing_begin");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    float sum = 0.0f;
    for (int i = 0; i < ctx->timing_frames; i++) {
        float ms = 0.0f;
        RPT_HIP(ctx, hipEventSynchronize(ctx->timing_events[2 * i + 1]));
        RPT_HIP(ctx, hipEventElapsedTime(&ms, ctx->timing_events[2 * i], ctx->timing_events[2 * i + 1]));
        sum += ms;
    }
    *total_ms = sum;
    *frames = ctx->timing_frames;
    ctx->timing_frames = -1;
    return RPT_OK;
}

int rpt_timing_end_frames(rpt_ctx *ctx, float *per_frame_ms, int capacity, int *frames) {
    if (!ctx || !per_frame_ms || capacity < 0 || !frames) return RPT_ERR_ARG;
    if (ctx->timing_frames < 0) return fail(ctx, RPT_ERR_STATE, "rpt_timing_end_frames without rpt_timing_begin");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const int n = ctx->timing_frames < capacity ? ctx->timing_frames : capacity;
    for (int i = 0; i < n; i++) {
        RPT_HIP(ctx, hipEventSynchronize(ctx->timing_events[2 * i + 1]));
        RPT_HIP(ctx, hipEventElapsedTime(&per_frame_ms[i], ctx->timing_events[2 * i], ctx->timing_events[2 * i + 1]));
    }
    *frames = n;
    ctx->timing_frames = -1;
    return RPT_OK;
}

int rpt_timing_end_spans(rpt_ctx *ctx, const rpt_ctx *base, float *begin_ms, float *end_ms, int capacity, int *frames) {
    if (!ctx || !base || !begin_ms || !end_ms || capacity < 0 || !frames) return RPT_ERR_ARG;
    if (ctx->timing_frames < 0) return fail(ctx, RPT_ERR_STATE, "rpt_timing_end_spans without rpt_timing_begin");
    if (base->timing_events.empty() || base->device != ctx->device) return fail(ctx, RPT_ERR_ARG, "rpt_timing_end_spans: the base context has no timing events on this device");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const int n = ctx->timing_frames < capacity ? ctx->timing_frames : capacity;
    RPT_HIP(ctx, hipEventSynchronize(base->timing_events[0]));
    for (int i = 0; i < n; i++) {
        RPT_HIP(ctx, hipEventSynchronize(ctx->timing_events[2 * i + 1]));
        RPT_HIP(ctx, hipEventElapsedTime(&begin_ms[i], base->timing_events[0], ctx->timing_events[2 * i]));
        RPT_HIP(ctx, hipEventElapsedTime(&end_ms[i], base->timing_events[0], ctx->timing_events[2 * i + 1]));
    }
    *frames = n;
    ctx->timing_frames = -1;
    return RPT_OK;
}

int rpt_set_plane_output(rpt_ctx *ctx, void *device_ptr_or_null) {
    if (!ctx) return RPT_ERR_ARG;
    ctx->external_plane = device_ptr_or_null;
    return RPT_OK;
}

int rpt_sync(rpt_ctx *ctx) {
    if (!ctx) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    for (Tally &t : ctx->tally) tally_collect(t);
    return RPT_OK;
}

int rpt_set_adaptive_aa(rpt_ctx *ctx, int samples_per_axis, int threshold) {
    if (!ctx) return RPT_ERR_ARG;
    if (samples_per_axis < 1 || samples_per_axis > 8) return fail(ctx, RPT_ERR_ARG, "rpt_set_adaptive_aa: 1..8 samples per axis (1 = off)");
    if (threshold < -1 || threshold > 255) return fail(ctx, RPT_ERR_ARG, "rpt_set_adaptive_aa: the threshold is -1 (refine every pixel) .. 255 (refine none)");
    ctx->aa_n = samples_per_axis;
    ctx->aa_threshold = threshold;
    return RPT_OK;
}

int rpt_last_aa_refined(rpt_ctx *ctx, unsigned long long *pixels) { return tally_read(ctx, TALLY_AA, pixels, 1); }

int rpt_last_aa_variant(const rpt_ctx *ctx) { return ctx ? ctx->last_aa_variant : RPT_ERR_ARG; }

int rpt_render(rpt_ctx *ctx) {
    if (int rc = render_frame(ctx, CallKind::blocking)) return rc;
    return rpt_sync(ctx);
}

int rpt_set_events_output(rpt_ctx *ctx, void *device_ptr_or_null) {
    if (!ctx) return RPT_ERR_ARG;
    ctx->external_events = device_ptr_or_null;
    return RPT_OK;
}

int rpt_render_events_async(rpt_ctx *ctx) { return render_pass(ctx, launch_event_frame, false); }
int rpt_render_events(rpt_ctx *ctx) { return render_pass(ctx, launch_event_frame, true); }

int rpt_read_events(rpt_ctx *ctx, void *host_dst, size_t bytes) {
    if (!ctx || !host_dst) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->event_frame.rendered() || !ctx->event_frame.buffer) return fail(ctx, RPT_ERR_STATE, "rpt_read_events: no event frame rendered yet");
    if (bytes > (size_t)ctx->event_frame.width * ctx->event_frame.height * sizeof(rpt_event)) return fail(ctx, RPT_ERR_ARG, "rpt_read_events: more bytes requested than the event frame holds");
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RPT_HIP(ctx, hipMemcpy(host_dst, ctx->event_frame.buffer, bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_pick(rpt_ctx *ctx, int x, int y, rpt_event *out) {
    if (!ctx || !out) return RPT_ERR_ARG;
    if (!ctx->event_frame.rendered() || !ctx->event_frame.buffer) return fail(ctx, RPT_ERR_STATE, "rpt_pick: no event frame rendered yet");
    if (x < 0 || y < 0 || x >= ctx->event_frame.width || y >= ctx->event_frame.height) return fail(ctx, RPT_ERR_ARG, "rpt_pick: the pixel lies outside the last event frame");
    // the rows of the last event frame that were this context's: tile t is one iff (t - first_tile) mod tile_step < run
    const int tile = y / RPT_TILE_ROWS, rel = tile - ctx->events_first_tile;
    if (rel < 0 || rel % ctx->events_tile_step >= (1 << ctx->events_run_log2)) return fail(ctx, RPT_ERR_ARG, "rpt_pick: the row is not one of this context's (rpt_set_rows)");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RPT_HIP(ctx, hipMemcpy(out, (const rpt_event *)ctx->event_frame.buffer + ((size_t)y * ctx->event_frame.width + x), sizeof(rpt_event), hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_last_events_variant(const rpt_ctx *ctx) { return ctx ? ctx->last_events_variant : RPT_ERR_ARG; }      // (no event kernel is numbered 1)

int rpt_last_events_exact_rcp(const rpt_ctx *ctx, int *exact_out) {
    if (!ctx || !exact_out) return RPT_ERR_ARG;
    *exact_out = ctx->last_events_exact_rcp ? 1 : 0;
    return RPT_OK;
}

int rpt_set_overlay(rpt_ctx *ctx, const rpt_overlay_desc *desc_or_null) {
    if (!ctx) return RPT_ERR_ARG;
    if (!desc_or_null) {
        ctx->overlay = rpt_overlay_desc{};
        return RPT_OK;
    }
    const rpt_overlay_desc &d = *desc_or_null;
    const uint32_t known = RPT_OVERLAY_OUTLINES | RPT_OVERLAY_ISO_DELAY | RPT_OVERLAY_ISO_CLOCK | RPT_OVERLAY_LATTICE | RPT_OVERLAY_DELAY_TINT;
    if (d.layers & ~known) return fail(ctx, RPT_ERR_ARG, "rpt_set_overlay: unknown layer bits (the layers are RPT_OVERLAY_*)");
    const auto step_ok = [](float s) { return std::isfinite(s) && s > 0.0f; };
    if ((d.layers & RPT_OVERLAY_ISO_DELAY) && !step_ok(d.delay_step)) return fail(ctx, RPT_ERR_ARG, "rpt_set_overlay: delay_step must be finite and > 0 while RPT_OVERLAY_ISO_DELAY is on");
    if ((d.layers & RPT_OVERLAY_ISO_CLOCK) && !step_ok(d.clock_step)) return fail(ctx, RPT_ERR_ARG, "rpt_set_overlay: clock_step must be finite and > 0 while RPT_OVERLAY_ISO_CLOCK is on");
    if (d.layers & RPT_OVERLAY_LATTICE) {
        bool any = false;
        for (int k = 0; k < 3; k++) {
            if (d.lattice_step[k] == 0.0f) continue;
            if (!step_ok(d.lattice_step[k])) return fail(ctx, RPT_ERR_ARG, "rpt_set_overlay: every lattice_step is finite and > 0, or 0 to skip its axis, while RPT_OVERLAY_LATTICE is on");
            any = true;
        }
        if (!any) return fail(ctx, RPT_ERR_ARG, "rpt_set_overlay: RPT_OVERLAY_LATTICE needs a step > 0 on at least one axis");
    }
    if (!std::isfinite(d.tint_t_max) || d.tint_t_max < 0.0f) return fail(ctx, RPT_ERR_ARG, "rpt_set_overlay: tint_t_max is > 0, or 0 for the frame's largest delay");
    ctx->overlay = d;
    return RPT_OK;
}

int rpt_render_overlay_async(rpt_ctx *ctx) { return render_pass(ctx, launch_overlay, false); }
int rpt_render_overlay(rpt_ctx *ctx) { return render_pass(ctx, launch_overlay, true); }

int rpt_last_overlay_pixels(rpt_ctx *ctx, unsigned long long *pixels) { return tally_read(ctx, TALLY_OVERLAY, pixels, 1); }

// The displays go to the device here, once, in stream order (a pass in flight keeps the table it was launched with); a call refused
// for its arguments has changed nothing, one that fails on the device (RPT_ERR_DEVICE) leaves no setting.
int rpt_set_readouts(rpt_ctx *ctx, const rpt_readout *per_object_or_null, int count) {
    if (!ctx || count < 0) return RPT_ERR_ARG;
    if (!per_object_or_null || count == 0) {
        ctx->readouts.clear();
        ctx->readout_low_mask = 0;
        return RPT_OK;
    }
    static const float pow10[7] = {1.0f, 10.0f, 100.0f, 1000.0f, 10000.0f, 100000.0f, 1000000.0f};
    std::vector<rptd::ReadoutDisplay> table((size_t)count);
    unsigned long long low_mask = 0;
    for (int i = 0; i < count; i++) {
        const rpt_readout &r = per_object_or_null[i];
        const std::string which = "rpt_set_readouts: entry " + std::to_string(i) + ": ";
        for (float f : {r.rate, r.offset, r.u0, r.v0, r.u1, r.v1})
            if (!std::isfinite(f)) return fail(ctx, RPT_ERR_ARG, which + "rate, offset and the rectangle must be finite");
        if (r.digits > 9) return fail(ctx, RPT_ERR_ARG, which + "digits is 0 (no display) or 1..9");
        rptd::ReadoutDisplay &d = table[(size_t)i];
        std::memset(&d, 0, sizeof d);
        if (r.digits == 0) continue;
        if (r.decimals > 6 || r.decimals >= r.digits) return fail(ctx, RPT_ERR_ARG, which + "decimals is 0..6 and below digits");
        if (r.u0 == r.u1 || r.v0 == r.v1) return fail(ctx, RPT_ERR_ARG, which + "the rectangle is empty (u0 == u1 or v0 == v1)");
        d.rate = r.rate;
        d.offset = r.offset;
        d.scale = pow10[r.decimals];
        d.digits = (uint32_t)r.digits | ((uint32_t)r.decimals << 8);
        d.u0 = r.u0;
        d.v0 = r.v0;
        d.inv_w = 1.0f / (r.u1 - r.u0);
        d.inv_h = 1.0f / (r.v1 - r.v0);
        d.on_rgba = packed_rgba(r.on_rgba);
        d.off_rgba = packed_rgba(r.off_rgba);
        if (i < 64) low_mask |= 1ull << i;
    }
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    void *host = nullptr;
    const size_t bytes = table.size() * sizeof(rptd::ReadoutDisplay);
    int rc = staged_host(ctx, ctx->readout_table, bytes, &host);
    if (!rc) {
        std::memcpy(host, table.data(), bytes);
        rc = staged_copy(ctx, ctx->readout_table);
    }
    if (rc) {       // a device error: the table may be gone or half written, so no setting is left rather than one that does not match it
        ctx->readouts.clear();
        ctx->readout_low_mask = 0;
        return rc;
    }
    ctx->readouts.assign(per_object_or_null, per_object_or_null + count);
    ctx->readout_low_mask = low_mask;
    return RPT_OK;
}

int rpt_render_readouts_async(rpt_ctx *ctx) { return render_pass(ctx, launch_readouts, false); }
int rpt_render_readouts(rpt_ctx *ctx) { return render_pass(ctx, launch_readouts, true); }

int rpt_last_readout_pixels(rpt_ctx *ctx, unsigned long long *pixels) { return tally_read(ctx, TALLY_READOUTS, pixels, 1); }

// The star-field pass.  The catalogue goes to the device once, here (set_records)
int rpt_set_stars(rpt_ctx *ctx, const rpt_star *stars_or_null, int count) {
    if (!ctx) return RPT_ERR_ARG;
    SplatPass &p = ctx->splat[SPLAT_STARS];
    return set_records(ctx, "rpt_set_stars", p.table, p.count, p.largest_object, stars_or_null, count, rpts::kMaxStars, rpts::catalogue_fault, rpts::prepare_catalogue);
}

int rpt_render_stars_async(rpt_ctx *ctx) { return render_pass(ctx, launch_stars, false); }
int rpt_render_stars(rpt_ctx *ctx) { return render_pass(ctx, launch_stars, true); }

int rpt_last_stars(rpt_ctx *ctx, unsigned long long out[2]) { return tally_read(ctx, TALLY_STARS, out, 2); }

int rpt_set_stars_measurement(rpt_ctx *ctx, int timed) { return set_splat_measurement(ctx, SPLAT_STARS, timed); }
int rpt_last_stars_ms(rpt_ctx *ctx, float ms[2]) { return last_splat_ms(ctx, SPLAT_STARS, ms, "stars", "star-field"); }

// Glare.  rpt_glare_taps: rule G1, host code, no device.  The off-centre taps are rounded from the normalised Gaussian
// in double; the centre tap is what is left of 65536, so the taps sum to it exactly.
int rpt_glare_taps(double sigma, unsigned int taps65_out[2 * RPT_GLARE_RADIUS_MAX + 1], int *radius_out) {
    if (!taps65_out || !radius_out || !(sigma >= 0.5) || !(sigma <= 32.0 / 3.0)) return RPT_ERR_ARG;
    const double r = std::ceil(3.0 * sigma);
    const int R = r < (double)RPT_GLARE_RADIUS_MAX ? (int)r : RPT_GLARE_RADIUS_MAX;
    double g[RPT_GLARE_RADIUS_MAX + 1], sum = 0.0;
    for (int j = 0; j <= R; j++) g[j] = std::exp(-(double)(j * j) / (2.0 * sigma * sigma));
    for (int j = -R; j <= R; j++) sum += g[j < 0 ? -j : j];
    for (int k = 0; k < 2 * RPT_GLARE_RADIUS_MAX + 1; k++) taps65_out[k] = 0u;
    unsigned int off_centre = 0u;
    for (int j = 1; j <= R; j++) {
        const unsigned int t = (unsigned int)std::floor(65536.0 * g[j] / sum + 0.5);
        taps65_out[RPT_GLARE_RADIUS_MAX + j] = taps65_out[RPT_GLARE_RADIUS_MAX - j] = t;
        off_centre += 2u * t;
    }
    taps65_out[RPT_GLARE_RADIUS_MAX] = 65536u - off_centre;      // (no underflow: the off-centre taps sum to less than 65536 (1 - g_0 / sum) + R)
    *radius_out = R;
    return RPT_OK;
}

// Rule G0.  Nothing touches the device: the integers ride in the arguments of kernels 1170 and 1171 from the next pass on
int rpt_set_glare(rpt_ctx *ctx, const rpt_glare *desc_or_null) {
    if (!ctx) return RPT_ERR_ARG;
    if (!desc_or_null || desc_or_null->layers == 0) {
        ctx->glare_layers = 0;
        return RPT_OK;
    }
    const rpt_glare &d = *desc_or_null;
    if (d.layers < 0 || d.layers > RPT_GLARE_LAYERS_MAX)
        return fail(ctx, RPT_ERR_ARG, "rpt_set_glare: " + std::to_string(d.layers) + " layers; there are 0 .. " + std::to_string(RPT_GLARE_LAYERS_MAX));
    unsigned int weight[1 + RPT_GLARE_LAYERS_MAX] = {0u, 0u, 0u, 0u}, taps[RPT_GLARE_LAYERS_MAX][2 * RPT_GLARE_RADIUS_MAX + 1];
    int radius[RPT_GLARE_LAYERS_MAX] = {0, 0, 0};
    long long core = 65536;
    for (int k = 0; k < d.layers; k++) {
        const std::string layer = "rpt_set_glare: layer " + std::to_string(k);
        if (!(d.weight[k] > 0.0) || !(d.weight[k] <= 1.0)) return fail(ctx, RPT_ERR_ARG, layer + ": the weight is " + std::to_string(d.weight[k]) + ", not in (0, 1]");
        if (rpt_glare_taps(d.sigma[k], taps[k], &radius[k]) != RPT_OK)
            return fail(ctx, RPT_ERR_ARG, layer + ": sigma is " + std::to_string(d.sigma[k]) + ", not in [0.5, 32/3]");
        weight[1 + k] = (unsigned int)std::floor(d.weight[k] * 65536.0 + 0.5);
        core -= (long long)weight[1 + k];
    }
    if (core < 0) return fail(ctx, RPT_ERR_ARG, "rpt_set_glare: the weights sum to more than 1 (the core would keep " + std::to_string(core) + " / 65536)");
    weight[0] = (unsigned int)core;
    ctx->glare_layers = d.layers;
    std::memcpy(ctx->glare_weight, weight, sizeof weight);
    std::memcpy(ctx->glare_radius, radius, sizeof radius);
    std::memset(ctx->glare_taps, 0, sizeof ctx->glare_taps);
    for (int k = 0; k < d.layers; k++)
        for (int j = 0; j <= radius[k]; j++) ctx->glare_taps[k][j] = taps[k][RPT_GLARE_RADIUS_MAX + j];
    return RPT_OK;
}

// The particle pass.  The set goes to the device once, here (set_records)
int rpt_set_particles(rpt_ctx *ctx, const rpt_particle *particles_or_null, int count) {
    if (!ctx) return RPT_ERR_ARG;
    SplatPass &p = ctx->splat[SPLAT_PARTICLES];
    return set_records(ctx, "rpt_set_particles", p.table, p.count, p.largest_object, particles_or_null, count, rptp::kMaxParticles, rptp::set_fault, rptp::prepare_set,
                       rptp::largest_object);
}

// rpt_set_particle_options, _ballistic_, _rocket_: one rule (rptp::options_fault), each pass's own pair
static int set_splat_options(rpt_ctx *ctx, int which, const char *call, int flags, float depth_bias) {
    if (!ctx) return RPT_ERR_ARG;
    const std::string fault = rptp::options_fault(flags, depth_bias);
    if (!fault.empty()) return fail(ctx, RPT_ERR_ARG, std::string(call) + ": " + fault);
    ctx->splat[which].flags = flags;
    ctx->splat[which].depth_bias = depth_bias;
    return RPT_OK;
}

int rpt_set_particle_options(rpt_ctx *ctx, int flags, float depth_bias) { return set_splat_options(ctx, SPLAT_PARTICLES, "rpt_set_particle_options", flags, depth_bias); }

int rpt_set_particle_lighting(rpt_ctx *ctx, int flags) {
    if (!ctx) return RPT_ERR_ARG;
    const std::string fault = rptl::lighting_fault(flags);
    if (!fault.empty()) return fail(ctx, RPT_ERR_ARG, "rpt_set_particle_lighting: " + fault);
    ctx->particle_lighting = flags;
    return RPT_OK;
}

int rpt_last_particle_lighting(rpt_ctx *ctx, unsigned long long out[2]) {
    unsigned long long all[4] = {0, 0, 0, 0};
    if (!out) return RPT_ERR_ARG;
    if (int rc = tally_read(ctx, TALLY_PARTICLES, all, 4)) return rc;
    out[0] = all[2];
    out[1] = all[3];
    return RPT_OK;
}

int rpt_render_particles_async(rpt_ctx *ctx) { return render_pass(ctx, launch_particles, false); }
int rpt_render_particles(rpt_ctx *ctx) { return render_pass(ctx, launch_particles, true); }

int rpt_last_particles(rpt_ctx *ctx, unsigned long long out[2]) { return tally_read(ctx, TALLY_PARTICLES, out, 2); }

int rpt_set_particles_measurement(rpt_ctx *ctx, int timed) { return set_splat_measurement(ctx, SPLAT_PARTICLES, timed); }
int rpt_last_particles_ms(rpt_ctx *ctx, float ms[2]) { return last_splat_ms(ctx, SPLAT_PARTICLES, ms, "particles", "particle"); }

// rpt_set_star_temperatures and rpt_set_particle_temperatures: the array goes to the device as x_G per source (set_records).  Whether
// its count matches the catalogue's or the set's is asked at the launch, not here.
static int set_temperatures(rpt_ctx *ctx, const char *call, int which, const float *kelvin_or_null, int count) {
    if (!ctx) return RPT_ERR_ARG;
    SplatPass &p = ctx->splat[which];
    int none = -1;
    return set_records(ctx, call, p.thermal_table, p.thermal_count, none, kelvin_or_null, count, rptt::kMaxTemperatures, rptt::temperatures_fault, rptt::prepare_temperatures);
}

int rpt_set_star_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count) { return set_temperatures(ctx, "rpt_set_star_temperatures", SPLAT_STARS, kelvin_or_null, count); }
int rpt_set_particle_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count) { return set_temperatures(ctx, "rpt_set_particle_temperatures", SPLAT_PARTICLES, kelvin_or_null, count); }
int rpt_set_ballistic_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count) { return set_temperatures(ctx, "rpt_set_ballistic_temperatures", SPLAT_BALLISTICS, kelvin_or_null, count); }

// The ballistic pass.  The set goes to the device once, here (set_records)
int rpt_set_ballistics(rpt_ctx *ctx, const rpt_ballistic *records_or_null, int count) {
    if (!ctx) return RPT_ERR_ARG;
    SplatPass &p = ctx->splat[SPLAT_BALLISTICS];
    return set_records(ctx, "rpt_set_ballistics", p.table, p.count, p.largest_object, records_or_null, count, rptb::kMaxBallistics, rptb::set_fault, rptb::prepare_set,
                       rptb::largest_object);
}

int rpt_set_ballistic_options(rpt_ctx *ctx, int flags, float depth_bias) { return set_splat_options(ctx, SPLAT_BALLISTICS, "rpt_set_ballistic_options", flags, depth_bias); }

int rpt_render_ballistics_async(rpt_ctx *ctx) { return render_pass(ctx, launch_ballistics, false); }
int rpt_render_ballistics(rpt_ctx *ctx) { return render_pass(ctx, launch_ballistics, true); }

int rpt_last_ballistics(rpt_ctx *ctx, unsigned long long out[2]) { return tally_read(ctx, TALLY_BALLISTICS, out, 2); }

int rpt_set_ballistics_measurement(rpt_ctx *ctx, int timed) { return set_splat_measurement(ctx, SPLAT_BALLISTICS, timed); }
int rpt_last_ballistics_ms(rpt_ctx *ctx, float ms[2]) { return last_splat_ms(ctx, SPLAT_BALLISTICS, ms, "ballistics", "ballistic"); }

// The rocket pass.  The set goes to the device once, here (set_records)
int rpt_set_rockets(rpt_ctx *ctx, const rpt_rocket *records_or_null, int count) {
    if (!ctx) return RPT_ERR_ARG;
    SplatPass &p = ctx->splat[SPLAT_ROCKETS];
    return set_records(ctx, "rpt_set_rockets", p.table, p.count, p.largest_object, records_or_null, count, rptr::kMaxRockets, rptr::set_fault, rptr::prepare_set,
                       rptr::largest_object);
}

int rpt_set_rocket_options(rpt_ctx *ctx, int flags, float depth_bias) { return set_splat_options(ctx, SPLAT_ROCKETS, "rpt_set_rocket_options", flags, depth_bias); }

int rpt_set_rocket_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count) { return set_temperatures(ctx, "rpt_set_rocket_temperatures", SPLAT_ROCKETS, kelvin_or_null, count); }

int rpt_render_rockets_async(rpt_ctx *ctx) { return render_pass(ctx, launch_rockets, false); }
int rpt_render_rockets(rpt_ctx *ctx) { return render_pass(ctx, launch_rockets, true); }

int rpt_last_rockets(rpt_ctx *ctx, unsigned long long out[2]) { return tally_read(ctx, TALLY_ROCKETS, out, 2); }

int rpt_set_rockets_measurement(rpt_ctx *ctx, int timed) { return set_splat_measurement(ctx, SPLAT_ROCKETS, timed); }
int rpt_last_rockets_ms(rpt_ctx *ctx, float ms[2]) { return last_splat_ms(ctx, SPLAT_ROCKETS, ms, "rockets", "rocket"); }

// The segment pass.  The set goes to the device once, here (set_records); the count is held against the pieces first (rptg::load_fault)
int rpt_set_segments(rpt_ctx *ctx, const rpt_segment *segments_or_null, int count) {
    if (!ctx) return RPT_ERR_ARG;
    SplatPass &p = ctx->splat[SPLAT_SEGMENTS];
    const int pieces = ctx->segment_pieces;
    const auto fault = [pieces](const rpt_segment *segments, int n) { return rptg::set_fault(segments, n, pieces); };
    if (count < 0 || !rptg::load_fault(count, pieces).empty()) return fail(ctx, RPT_ERR_ARG, "rpt_set_segments: " + fault(nullptr, count));
    return set_records(ctx, "rpt_set_segments", p.table, p.count, p.largest_object, segments_or_null, count, (int)rptg::kMaxPieces, fault, rptg::prepare_set, rptg::largest_object);
}

int rpt_set_segment_options(rpt_ctx *ctx, int flags, float depth_bias, int pieces) {
    if (!ctx) return RPT_ERR_ARG;
    const std::string fault = rptg::options_fault(flags, depth_bias, pieces, ctx->splat[SPLAT_SEGMENTS].count);
    if (!fault.empty()) return fail(ctx, RPT_ERR_ARG, "rpt_set_segment_options: " + fault);
    ctx->splat[SPLAT_SEGMENTS].flags = flags;
    ctx->splat[SPLAT_SEGMENTS].depth_bias = depth_bias;
    ctx->segment_pieces = pieces;
    return RPT_OK;
}

int rpt_render_segments_async(rpt_ctx *ctx) { return render_pass(ctx, launch_segments, false); }
int rpt_render_segments(rpt_ctx *ctx) { return render_pass(ctx, launch_segments, true); }

int rpt_last_segments(rpt_ctx *ctx, unsigned long long out[2]) { return tally_read(ctx, TALLY_SEGMENTS, out, 2); }

int rpt_set_segments_measurement(rpt_ctx *ctx, int timed) { return set_splat_measurement(ctx, SPLAT_SEGMENTS, timed); }
int rpt_last_segments_ms(rpt_ctx *ctx, float ms[2]) { return last_splat_ms(ctx, SPLAT_SEGMENTS, ms, "segments", "segment"); }

void *rpt_output_ptr(rpt_ctx *ctx) {
    if (!ctx) return nullptr;
    return ctx->external_out ? ctx->external_out : ctx->owned_out.ptr;
}

size_t rpt_output_bytes(rpt_ctx *ctx) { return ctx ? (size_t)ctx->width * ctx->height * 16 : 0; }

void *rpt_colour_plane_ptr(rpt_ctx *ctx) { return ctx ? (ctx->external_plane ? ctx->external_plane : ctx->owned_plane.ptr) : nullptr; }

int rpt_read_framebuffer(rpt_ctx *ctx, void *host_dst, size_t bytes) {
    if (!ctx || !host_dst) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const void *src = ctx->colour_plane ? rpt_colour_plane_ptr(ctx) : rpt_output_ptr(ctx);
    const size_t have = ctx->colour_plane ? (size_t)local_tile_count(ctx) * RPT_TILE_ROWS * ctx->width * 4 : rpt_output_bytes(ctx);
    if (!src || !ctx->colour_frame.rendered()) return fail(ctx, RPT_ERR_STATE, "rpt_read_framebuffer: nothing rendered yet");
    if (bytes > have) return fail(ctx, RPT_ERR_ARG, "rpt_read_framebuffer: more bytes requested than the framebuffer holds");
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RPT_HIP(ctx, hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_read_debug_rgb(rpt_ctx *ctx, void *host_dst, size_t bytes) {
    if (!ctx || !host_dst) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const void *src = ctx->external_rgb ? ctx->external_rgb : (ctx->want_owned_rgb ? ctx->owned_rgb.ptr : nullptr);
    if (!src || !ctx->colour_frame.rendered()) return fail(ctx, RPT_ERR_STATE, "rpt_read_debug_rgb: debug RGB is not enabled or nothing rendered");
    if (bytes > (size_t)ctx->width * ctx->height * 12) return fail(ctx, RPT_ERR_ARG, "rpt_read_debug_rgb: too many bytes");
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RPT_HIP(ctx, hipMemcpy(host_dst, src, bytes, hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_last_frame_ms(rpt_ctx *ctx, float *ms) {
    if (!ctx || !ms) return RPT_ERR_ARG;
    if (!ctx->colour_frame.rendered()) return fail(ctx, RPT_ERR_STATE, "rpt_last_frame_ms: nothing rendered yet");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    RPT_HIP(ctx, hipEventSynchronize(ctx->ev_end));
    RPT_HIP(ctx, hipEventElapsedTime(&ctx->last_ms, ctx->ev_begin, ctx->ev_end));
    *ms = ctx->last_ms;
    return RPT_OK;
}

int rpt_timed_frames(rpt_ctx *ctx, int frames, float *avg_ms) {
    if (!ctx || frames <= 0 || !avg_ms) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    for (int w = 0; w < 2; w++) {          // untimed: allocate outputs, warm caches, measure the row costs
        if (int rc = launch(ctx, Call{CallKind::in_flight, false})) return rc;
        RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    RPT_HIP(ctx, hipEventRecord(ctx->ev_begin, ctx->stream));
    for (int i = 0; i < frames; i++)
        if (int rc = launch(ctx, Call{CallKind::in_flight, false})) return rc;
    RPT_HIP(ctx, hipEventRecord(ctx->ev_end, ctx->stream));
    RPT_HIP(ctx, hipEventSynchronize(ctx->ev_end));
    float ms = 0;
    RPT_HIP(ctx, hipEventElapsedTime(&ms, ctx->ev_begin, ctx->ev_end));
    mark_colour_frame(ctx);
    ctx->last_ms = ms / frames;
    *avg_ms = ctx->last_ms;
    return RPT_OK;
}

int rpt_scatter_colour_plane_on(rpt_ctx *ctx, void *hip_stream, const void *planes, void *out16, int width, int height,
                                int n_ranks, int plane_stride_words);

int rpt_scatter_colour_plane(rpt_ctx *ctx, const void *planes, void *out16, int width, int height, int n_ranks,
                             int plane_stride_words, int reserved) {
    return rpt_scatter_colour_plane_on(ctx, ctx ? (void *)ctx->stream : nullptr, planes, out16, width, height, n_ranks, plane_stride_words);
}

int rpt_scatter_colour_plane_on(rpt_ctx *ctx, void *hip_stream, const void *planes, void *out16, int width, int height,
                                int n_ranks, int plane_stride_words) {
    if (!ctx || !planes || !out16 || width <= 0 || height <= 0 || n_ranks <= 0 || plane_stride_words < 0) return RPT_ERR_ARG;
    const int tiles = (height + RPT_TILE_ROWS - 1) / RPT_TILE_ROWS;
    const long long need = (long long)((tiles + n_ranks - 1) / n_ranks) * RPT_TILE_ROWS * width;
    if ((long long)plane_stride_words < need) return fail(ctx, RPT_ERR_ARG, "rpt_scatter_colour_plane: plane stride smaller than one rank's plane");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid((width + 255) / 256, height);
    hipLaunchKernelGGL(rptd::rpt_scatter_plane_kernel, grid, dim3(256), 0, hip_stream ? (hipStream_t)hip_stream : ctx->stream, (const uint32_t *)planes,
                       (rpt_pixel *)out16, width, height, n_ranks, (size_t)plane_stride_words);
    RPT_HIP(ctx, hipGetLastError());
    return RPT_OK;
}

int rpt_pack_colour_plane3_on(rpt_ctx *ctx, void *hip_stream, const void *plane4, void *plane3, size_t pixels) {
    if (!ctx || !plane4 || !plane3) return RPT_ERR_ARG;
    if (pixels % 4) return fail(ctx, RPT_ERR_ARG, "rpt_pack_colour_plane3: pixel count is not a multiple of 4");
    if (pixels == 0) return RPT_OK;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const size_t quads = pixels / 4;
    hipLaunchKernelGGL(rptd::rpt_pack_plane3_kernel, dim3((unsigned int)((quads + 255) / 256)), dim3(256), 0,
                       hip_stream ? (hipStream_t)hip_stream : ctx->stream, (const uint4 *)plane4, (uint32_t *)plane3, quads);
    RPT_HIP(ctx, hipGetLastError());
    return RPT_OK;
}

int rpt_scatter_colour_plane3_on(rpt_ctx *ctx, void *hip_stream, const void *planes3, void *out16, int width, int height,
                                 int n_ranks, size_t plane_stride_bytes) {
    if (!ctx || !planes3 || !out16 || width <= 0 || height <= 0 || n_ranks <= 0) return RPT_ERR_ARG;
    const int tiles = (height + RPT_TILE_ROWS - 1) / RPT_TILE_ROWS;
    const unsigned long long need = 3ull * (unsigned long long)((tiles + n_ranks - 1) / n_ranks) * RPT_TILE_ROWS * (unsigned long long)width;
    if ((unsigned long long)plane_stride_bytes < need) return fail(ctx, RPT_ERR_ARG, "rpt_scatter_colour_plane3: plane stride smaller than one rank's plane");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid((width + 255) / 256, height);
    hipLaunchKernelGGL(rptd::rpt_scatter_plane3_kernel, grid, dim3(256), 0, hip_stream ? (hipStream_t)hip_stream : ctx->stream,
                       (const uint8_t *)planes3, (rpt_pixel *)out16, width, height, n_ranks, plane_stride_bytes);
    RPT_HIP(ctx, hipGetLastError());
    return RPT_OK;
}

int rpt_scatter_helper_planes3_on(rpt_ctx *ctx, void *hip_stream, const void *planes3, void *out16, int width, int height,
                                  int n_ranks, int root_run, size_t plane_stride_bytes) {
    if (!ctx || !planes3 || !out16 || width <= 0 || height <= 0 || n_ranks < 1 || root_run < 1) return RPT_ERR_ARG;
    const int period = root_run + n_ranks - 1;
    const int tiles = (height + RPT_TILE_ROWS - 1) / RPT_TILE_ROWS;
    const unsigned long long need = 3ull * (unsigned long long)((tiles + period - 1) / period) * RPT_TILE_ROWS * (unsigned long long)width;
    if ((unsigned long long)plane_stride_bytes < need) return fail(ctx, RPT_ERR_ARG, "rpt_scatter_helper_planes3: plane stride smaller than one helper's plane");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    const dim3 grid((width + 255) / 256, height);
    hipLaunchKernelGGL(rptd::rpt_scatter_helper_planes3_kernel, grid, dim3(256), 0, hip_stream ? (hipStream_t)hip_stream : ctx->stream,
                       (const uint8_t *)planes3, (rpt_pixel *)out16, width, height, period, root_run, plane_stride_bytes);
    RPT_HIP(ctx, hipGetLastError());
    return RPT_OK;
}

int rpt_read_counters(rpt_ctx *ctx, unsigned long long out[16]) {
    if (!ctx || !out) return RPT_ERR_ARG;
    if (!ctx->counters.ptr) return fail(ctx, RPT_ERR_STATE, "rpt_read_counters: render with the diagnostic variant (7) first");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    RPT_HIP(ctx, hipMemcpy(out, ctx->counters.ptr, 16 * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    return RPT_OK;
}

int rpt_read_wave_times(rpt_ctx *ctx, unsigned long long *out, size_t max_words, size_t *words) {
    if (!ctx || !out || !words) return RPT_ERR_ARG;
    if (!ctx->wave_times.ptr) return fail(ctx, RPT_ERR_STATE, "rpt_read_wave_times: render with the diagnostic variant (7) first");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));
    size_t n = ctx->wave_times.bytes / sizeof(unsigned long long);
    if (n > max_words) n = max_words;
    RPT_HIP(ctx, hipMemcpy(out, ctx->wave_times.ptr, n * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    *words = n;
    return RPT_OK;
}

int rpt_probe(rpt_ctx *ctx, int which, const void *host_in, void *host_out, int n) {
    static const int in_w[9] = {15, 12, 4, 3, 3, 6, 5, 3, 6}, out_w[9] = {4, 5, 3, 3, 2, 12, 3, 5, 3};
    if (!ctx || which < 0 || which > 8 || !host_in || !host_out || n <= 0) return RPT_ERR_ARG;
    if (which == 7 && !ctx->env_on) return fail(ctx, RPT_ERR_STATE, "rpt_probe 7: the context has no environment (rpt_set_environment)");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    float *d_in = nullptr, *d_out = nullptr;
    RPT_HIP(ctx, hipMalloc((void **)&d_in, sizeof(float) * in_w[which] * n));
    if (hipMalloc((void **)&d_out, sizeof(float) * out_w[which] * n) != hipSuccess) {
        (void)hipFree(d_in);
        return fail(ctx, RPT_ERR_NOMEM, "rpt_probe: hipMalloc");
    }
    int rc = RPT_OK;
    if (hipMemcpy(d_in, host_in, sizeof(float) * in_w[which] * n, hipMemcpyHostToDevice) != hipSuccess) rc = RPT_ERR_DEVICE;
    if (!rc) {
        if (which == 6) hipLaunchKernelGGL(rptd::rpt_probe_doppler_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_in, d_out, n);
        else if (which == 8) hipLaunchKernelGGL(rptd::rpt_probe_thermal_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, d_in, d_out, n);
        else if (which == 7) hipLaunchKernelGGL(rptd::rpt_probe_environment_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, (const uint32_t *)ctx->env.device.ptr, ctx->env_width, ctx->env_height, d_in, d_out, n);
        else hipLaunchKernelGGL(rptd::rpt_probe_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, which, d_in, d_out, n);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
            hipMemcpy(host_out, d_out, sizeof(float) * out_w[which] * n, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(ctx, RPT_ERR_DEVICE, "rpt_probe: device error");
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

int rpt_probe_walk(rpt_ctx *ctx, int object_index, const float *host_rays, float *host_out, int n) {
    if (!ctx || !host_rays || !host_out || n <= 0) return RPT_ERR_ARG;
    if (!ctx->scene_uploaded || ctx->object_count <= 0) return fail(ctx, RPT_ERR_STATE, "rpt_probe_walk before rpt_upload_scene / rpt_set_objects");
    if (object_index < 0 || object_index >= ctx->object_count || ctx->host_objects.size() < (size_t)(object_index + 1) * sizeof(rpt_object) ||
        ((const rpt_object *)ctx->host_objects.data())[object_index].type != RPT_MESH)
        return fail(ctx, RPT_ERR_ARG, "rpt_probe_walk: not a mesh object");
    if (!ctx->geo->compact_ok) return fail(ctx, RPT_ERR_STATE, "rpt_probe_walk: this octree has no derived layout (children not consecutive)");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    rptd::KernelArgs a;
    probe_kernel_args(ctx, a);
    float *d_in = nullptr, *d_out = nullptr;
    RPT_HIP(ctx, hipMalloc((void **)&d_in, sizeof(float) * 6 * (size_t)n));
    if (hipMalloc((void **)&d_out, sizeof(float) * 24 * (size_t)n) != hipSuccess) {
        (void)hipFree(d_in);
        return fail(ctx, RPT_ERR_NOMEM, "rpt_probe_walk: hipMalloc");
    }
    int rc = RPT_OK;
    if (hipMemcpy(d_in, host_rays, sizeof(float) * 6 * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) rc = RPT_ERR_DEVICE;
    if (!rc) {
        hipLaunchKernelGGL(rptd::rpt_probe_walk_kernel, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, a, object_index, d_in, d_out, n,
                           ctx->geo->exact_rcp_ok ? 1 : 0);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
            hipMemcpy(host_out, d_out, sizeof(float) * 24 * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(ctx, RPT_ERR_DEVICE, "rpt_probe_walk: device error");
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

int rpt_probe_reciprocal(rpt_ctx *ctx, float lo, float hi, unsigned long long counts_out[5], float *samples_out, int max_samples) {
    if (!ctx || !counts_out || !(lo > 0.0f) || !(hi >= lo) || !(hi <= 0x1p127f) || max_samples < 0) return RPT_ERR_ARG;
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    uint32_t lo_bits, hi_bits;
    std::memcpy(&lo_bits, &lo, 4);
    std::memcpy(&hi_bits, &hi, 4);
    const unsigned long long per_sign = (unsigned long long)(hi_bits - lo_bits) + 1ull;
    unsigned long long *d_counts = nullptr;
    float *d_samples = nullptr;
    RPT_HIP(ctx, hipMalloc((void **)&d_counts, 5 * sizeof(unsigned long long)));
    if (max_samples > 0 && samples_out && hipMalloc((void **)&d_samples, sizeof(float) * 2 * (size_t)max_samples) != hipSuccess) {
        (void)hipFree(d_counts);
        return fail(ctx, RPT_ERR_NOMEM, "rpt_probe_reciprocal: hipMalloc");
    }
    int rc = RPT_OK;
    if (hipMemsetAsync(d_counts, 0, 5 * sizeof(unsigned long long), ctx->stream) != hipSuccess) rc = RPT_ERR_DEVICE;
    if (!rc && d_samples && hipMemsetAsync(d_samples, 0, sizeof(float) * 2 * (size_t)max_samples, ctx->stream) != hipSuccess) rc = RPT_ERR_DEVICE;
    if (!rc) {
        // every bit pattern of [lo, hi], both signs: 2^30 lanes at most (hi_bits - lo_bits < 2^31), a fixed grid striding over them
        const unsigned int blocks = 16384;
        hipLaunchKernelGGL(rptd::rpt_probe_reciprocal_kernel, dim3(blocks), dim3(256), 0, ctx->stream, lo_bits, per_sign, d_counts, d_samples, max_samples);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
            hipMemcpy(counts_out, d_counts, 5 * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess ||
            (d_samples && hipMemcpy(samples_out, d_samples, sizeof(float) * 2 * (size_t)max_samples, hipMemcpyDeviceToHost) != hipSuccess))
            rc = fail(ctx, RPT_ERR_DEVICE, "rpt_probe_reciprocal: device error");
    }
    (void)hipFree(d_counts);
    if (d_samples) (void)hipFree(d_samples);
    return rc;
}

int rpt_probe_object(rpt_ctx *ctx, int which, int object_index, const float *host_in, float *host_out, int n) {
    if (!ctx || !host_in || !host_out || n <= 0 || which < 0 || which > 3) return RPT_ERR_ARG;
    if (!ctx->scene_uploaded || ctx->object_count <= 0) return fail(ctx, RPT_ERR_STATE, "rpt_probe_object before rpt_upload_scene / rpt_set_objects");
    if (object_index < 0 || object_index >= ctx->object_count) return fail(ctx, RPT_ERR_ARG, "rpt_probe_object: no such object");
    if (!ctx->geo->compact_ok) return fail(ctx, RPT_ERR_STATE, "rpt_probe_object: this octree has no derived layout (children not consecutive)");
    RPT_HIP(ctx, hipSetDevice(ctx->device));
    rptd::KernelArgs a;
    probe_kernel_args(ctx, a);
    const size_t in_floats = which == 0 ? 8 : which == 1 ? 9 : which == 2 ? 4 : 3, out_floats = which == 1 ? 2 : which == 2 ? 16 : 8;
    float *d_in = nullptr, *d_out = nullptr;
    RPT_HIP(ctx, hipMalloc((void **)&d_in, sizeof(float) * in_floats * (size_t)n));
    if (hipMalloc((void **)&d_out, sizeof(float) * out_floats * (size_t)n) != hipSuccess) {
        (void)hipFree(d_in);
        return fail(ctx, RPT_ERR_NOMEM, "rpt_probe_object: hipMalloc");
    }
    int rc = RPT_OK;
    if (hipMemcpy(d_in, host_in, sizeof(float) * in_floats * (size_t)n, hipMemcpyHostToDevice) != hipSuccess) rc = RPT_ERR_DEVICE;
    if (!rc) {
        hipLaunchKernelGGL(rptd::rpt_probe_object_kernel, dim3((n + 63) / 64), dim3(64), 0, ctx->stream, a, which, object_index, d_in, d_out, n);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
            hipMemcpy(host_out, d_out, sizeof(float) * out_floats * (size_t)n, hipMemcpyDeviceToHost) != hipSuccess)
            rc = fail(ctx, RPT_ERR_DEVICE, "rpt_probe_object: device error");
    }
    (void)hipFree(d_in);
    (void)hipFree(d_out);
    return rc;
}

}  // extern "C"

// ---------------------------------------------------------------------------------------------
// GPU octree build: replaces Mesh::GenerateOctree (Mesh.cpp:5-28) + Subdivide
// (Octree.cpp:171-248).  The triangle/box classification of each level runs on the device
// (rpt_octree_build.hip.h); the O(nodes) bookkeeping — child boxes, the valence stop rule, the reference's
// depth-first numbering of nodes and lists, neighbour links — is done here with the host builder's
// arithmetic, so the output is byte-identical to csrc/host/rpt_octree.cpp.
namespace {

struct BuildNode {
    float mn[3], mx[3];
    unsigned int list_begin = 0, list_count = 0;   // in its level's list buffer
    int min_tris = 0, depth = 0;
    int first_child = -1;                           // index in the next level's node array, -1 = not split
    int valence = 0;
};

struct DevTemp {
    void *p = nullptr;
    ~DevTemp() { if (p) (void)hipFree(p); }
};

}  // namespace

extern "C" void rpt_free_host(void *p) { std::free(p); }

extern "C" int rpt_build_octree(rpt_ctx *ctx, const rpt_float3 *vertices, size_t vertex_count, const uint32_t *triangles,
                                size_t triangle_words, size_t first_triangle_word, int node_index_base, int tri_index_base,
                                rpt_octree **nodes_out, size_t *node_count, int32_t **tris_out, size_t *tri_count) {
    if (!ctx || !vertices || !triangles || !nodes_out || !node_count || !tris_out || !tri_count) return RPT_ERR_ARG;
    if (triangle_words % 9 || first_triangle_word % 9 || first_triangle_word >= triangle_words)
        return fail(ctx, RPT_ERR_ARG, "rpt_build_octree: triangle words must be a multiple of 9 and the mesh must have triangles");
    const size_t n_tris_total = triangle_words / 9;
    if (n_tris_total > (size_t)0x3fffffff) return fail(ctx, RPT_ERR_ARG, "rpt_build_octree: too many triangles");
    for (size_t w = 0; w < triangle_words; w += 3)
        if (triangles[w] >= vertex_count) return fail(ctx, RPT_ERR_SCENE, "rpt_build_octree: vertex index out of range");
    RPT_HIP(ctx, hipSetDevice(ctx->device));

    // root (Mesh.cpp:6-21): bounds over this mesh's face-corner vertices, list = every triangle imported so far
    rptb::BNode root;
    std::memset(&root, 0, sizeof root);
    {
        const rpt_float3 v0 = vertices[triangles[first_triangle_word]];
        root.mn[0] = root.mx[0] = v0.x; root.mn[1] = root.mx[1] = v0.y; root.mn[2] = root.mx[2] = v0.z;
        for (size_t i = first_triangle_word / 3; i < triangle_words / 3; i++) {
            const rpt_float3 v = vertices[triangles[3 * i]];
            const float c[3] = {v.x, v.y, v.z};
            for (int k = 0; k < 3; k++) {
                root.mn[k] = root.mn[k] < c[k] ? root.mn[k] : c[k];
                root.mx[k] = root.mx[k] > c[k] ? root.mx[k] : c[k];
            }
        }
        root.list_begin = 0;
        root.list_count = (unsigned int)n_tris_total;
        root.min_tris = 0;
        root.depth = 6;
        root.first_child = -1;
        root.valence = 0;
    }
    const int max_depth = root.depth;                                  // levels 0 .. max_depth
    size_t level_nodes[8], node_offset[8], nodes_total = 0;           // at most 8^level nodes on a level
    for (int l = 0; l <= max_depth; l++) {
        level_nodes[l] = (size_t)1 << (3 * l);
        node_offset[l] = nodes_total;
        nodes_total += level_nodes[l];
    }

    DevTemp d_vertices, d_triangles;
    RPT_HIP(ctx, hipMalloc(&d_vertices.p, vertex_count * sizeof(rpt_float3)));
    RPT_HIP(ctx, hipMalloc(&d_triangles.p, triangle_words * sizeof(uint32_t)));
    RPT_HIP(ctx, hipMemcpy(d_vertices.p, vertices, vertex_count * sizeof(rpt_float3), hipMemcpyHostToDevice));
    RPT_HIP(ctx, hipMemcpy(d_triangles.p, triangles, triangle_words * sizeof(uint32_t), hipMemcpyHostToDevice));

    auto T0 = std::chrono::steady_clock::now();
    auto lap = [&](const char *what) { if (std::getenv("RPT_OCTREE_TIMING")) { auto t = std::chrono::steady_clock::now(); std::fprintf(stderr, "  octree %-10s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t - T0).count()); T0 = t; } };
    std::vector<std::vector<BuildNode>> levels;
    std::vector<std::vector<int32_t>> lists;          // host copies of every level's concatenated lists
    // One submission per attempt; an attempt whose lists outgrow `cap` entries per level says so in the header and is repeated.
    size_t cap = std::max<size_t>(16 * n_tris_total, 4096);
    if (const char *e = std::getenv("RPT_OCTREE_LIST_CAP"))            // test hook: start small, so that the repeat path runs
        cap = std::max<size_t>(n_tris_total, (size_t)std::strtoull(e, nullptr, 10));
    for (int attempt = 0;; attempt++) {
        if (8 * cap > 0xffffffffull) return fail(ctx, RPT_ERR_NOMEM, "rpt_build_octree: triangle lists exceed what the builder indexes with 32 bits");
        size_t hash_slots = 1;
        while (hash_slots < 6 * cap) hash_slots <<= 1;                 // three vertex occurrences per entry, at most half full
        const size_t chunk_cap = cap / 32 + level_nodes[max_depth] + 8; // 8 * (entries / 256 + splitting nodes), rounded up
        // one arena for everything the levels need
        size_t arena_bytes = 0;
        auto carve = [&](size_t bytes) { const size_t at = arena_bytes; arena_bytes += (bytes + 255) & ~(size_t)255; return at; };
        const size_t o_hdr = carve(sizeof(rptb::BuildHeader)), o_nodes = carve(nodes_total * sizeof(rptb::BNode)),
                     o_lists = carve((size_t)(max_depth + 1) * cap * sizeof(int32_t)), o_children = carve(level_nodes[max_depth] * sizeof(rptb::ChildDesc)),
                     o_split = carve(level_nodes[max_depth] / 8 * sizeof(unsigned int) + 16), o_flags = carve(8 * cap + 16),
                     o_counts = carve(chunk_cap * sizeof(unsigned int)), o_chunk_out = carve(chunk_cap * sizeof(unsigned int)),
                     o_keys = carve(hash_slots * sizeof(unsigned long long)), o_hits = carve(hash_slots * sizeof(unsigned int));
        DevTemp arena;
        RPT_HIP(ctx, hipMalloc(&arena.p, arena_bytes));
        struct Part { void *p; } d_hdr{(char *)arena.p + o_hdr}, d_nodes{(char *)arena.p + o_nodes}, d_lists{(char *)arena.p + o_lists},
            d_children{(char *)arena.p + o_children}, d_split{(char *)arena.p + o_split}, d_flags{(char *)arena.p + o_flags},
            d_counts{(char *)arena.p + o_counts}, d_chunk_out{(char *)arena.p + o_chunk_out}, d_keys{(char *)arena.p + o_keys},
            d_hits{(char *)arena.p + o_hits};
        lap("alloc");
        rptb::BNode *nodes_dev = (rptb::BNode *)d_nodes.p;
        int32_t *lists_dev = (int32_t *)d_lists.p;
        rptb::BuildHeader *hdr_dev = (rptb::BuildHeader *)d_hdr.p;

        rptb::BuildHeader hdr;
        std::memset(&hdr, 0, sizeof hdr);
        hdr.n_nodes[0] = 1;
        hdr.list_len[0] = (unsigned int)n_tris_total;
        RPT_HIP(ctx, hipMemcpyAsync(hdr_dev, &hdr, sizeof hdr, hipMemcpyHostToDevice, ctx->stream));
        RPT_HIP(ctx, hipMemcpyAsync(nodes_dev, &root, sizeof root, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL(rptb::iota_kernel, dim3((unsigned int)((n_tris_total + 255) / 256)), dim3(256), 0, ctx->stream, lists_dev,
                           (unsigned int)n_tris_total);
        const unsigned int entry_blocks = (unsigned int)((cap + 255) / 256);
        for (int l = 0; l < max_depth; l++) {
            rptb::BNode *nodes_l = nodes_dev + node_offset[l], *nodes_next = nodes_dev + node_offset[l + 1];
            int32_t *list_l = lists_dev + (size_t)l * cap, *list_next = lists_dev + (size_t)(l + 1) * cap;
            const size_t chunks_l = std::min(chunk_cap, cap / 32 + level_nodes[l + 1] + 8);
            RPT_HIP(ctx, hipMemsetAsync(d_keys.p, 0xff, hash_slots * sizeof(unsigned long long), ctx->stream));
            RPT_HIP(ctx, hipMemsetAsync(d_hits.p, 0, hash_slots * sizeof(unsigned int), ctx->stream));
            hipLaunchKernelGGL(rptb::valence_kernel, dim3(entry_blocks), dim3(256), 0, ctx->stream, (const uint32_t *)d_triangles.p,
                               (const int32_t *)list_l, nodes_l, (const rptb::BuildHeader *)hdr_dev, l, (unsigned long long *)d_keys.p,
                               (unsigned int *)d_hits.p, (unsigned int)(hash_slots - 1));
            hipLaunchKernelGGL(rptb::split_kernel, dim3(1), dim3(1024), 0, ctx->stream, nodes_l, hdr_dev, l, (rptb::ChildDesc *)d_children.p,
                               (unsigned int *)d_split.p, (unsigned int)level_nodes[l + 1]);
            hipLaunchKernelGGL(rptb::sat_flag_kernel, dim3((unsigned int)chunks_l), dim3(256), 0, ctx->stream, (const rpt_float3 *)d_vertices.p,
                               (const uint32_t *)d_triangles.p, (const int32_t *)list_l, (const rptb::ChildDesc *)d_children.p,
                               (const rptb::BuildHeader *)hdr_dev, (unsigned char *)d_flags.p, (unsigned int *)d_counts.p);
            hipLaunchKernelGGL(rptb::chunk_scan_kernel, dim3(1), dim3(1024), 0, ctx->stream, (const unsigned int *)d_counts.p,
                               (unsigned int *)d_chunk_out.p, hdr_dev, l, (unsigned int)cap);
            hipLaunchKernelGGL(rptb::sat_compact_kernel, dim3((unsigned int)chunks_l), dim3(256), 0, ctx->stream, (const int32_t *)list_l,
                               (const rptb::ChildDesc *)d_children.p, (const rptb::BuildHeader *)hdr_dev, (const unsigned char *)d_flags.p,
                               (const unsigned int *)d_chunk_out.p, list_next, (unsigned int)cap);
            hipLaunchKernelGGL(rptb::next_nodes_kernel, dim3((unsigned int)((level_nodes[l + 1] + 255) / 256)), dim3(256), 0, ctx->stream,
                               (const rptb::BNode *)nodes_l, (const rptb::ChildDesc *)d_children.p, (const unsigned int *)d_split.p,
                               (const unsigned int *)d_chunk_out.p, (const rptb::BuildHeader *)hdr_dev, l, nodes_next);
        }
        RPT_HIP(ctx, hipGetLastError());
        lap("submit");
        RPT_HIP(ctx, hipMemcpyAsync(&hdr, hdr_dev, sizeof hdr, hipMemcpyDeviceToHost, ctx->stream));
        RPT_HIP(ctx, hipStreamSynchronize(ctx->stream));             // the only wait of the build
        lap("wait");
        if (hdr.overflow) {
            // the level that overflowed said how many entries it wanted; deeper levels can want more still (at most 8x per level in
            // theory, ~1.3x in practice), so that figure gets a quarter on top, and the build may be repeated up to six times
            if (attempt >= 6) return fail(ctx, RPT_ERR_NOMEM, "rpt_build_octree: triangle lists keep outgrowing their buffers");
            cap = std::max<size_t>(cap * 2, (size_t)hdr.needed + (size_t)hdr.needed / 4);
            continue;
        }
        // read the levels back: nodes and lists of every level that has nodes
        levels.clear();
        lists.clear();
        for (int l = 0; l <= max_depth && hdr.n_nodes[l] > 0; l++) {
            if (hdr.n_nodes[l] > level_nodes[l] || hdr.list_len[l] > cap) return fail(ctx, RPT_ERR_DEVICE, "rpt_build_octree: inconsistent level sizes");
            std::vector<rptb::BNode> dev_nodes(hdr.n_nodes[l]);
            RPT_HIP(ctx, hipMemcpy(dev_nodes.data(), nodes_dev + node_offset[l], dev_nodes.size() * sizeof(rptb::BNode), hipMemcpyDeviceToHost));
            std::vector<BuildNode> nodes(dev_nodes.size());
            for (size_t i = 0; i < nodes.size(); i++) {
                const rptb::BNode &d = dev_nodes[i];
                BuildNode &b = nodes[i];
                for (int k = 0; k < 3; k++) { b.mn[k] = d.mn[k]; b.mx[k] = d.mx[k]; }
                b.list_begin = d.list_begin; b.list_count = d.list_count;
                b.min_tris = d.min_tris; b.depth = d.depth; b.first_child = d.first_child; b.valence = d.valence;
                if ((size_t)d.list_begin + d.list_count > hdr.list_len[l] || (d.first_child >= 0 && (l == max_depth || (size_t)d.first_child + 8 > hdr.n_nodes[l + 1])))
                    return fail(ctx, RPT_ERR_DEVICE, "rpt_build_octree: inconsistent node record");
            }
            std::vector<int32_t> list(hdr.list_len[l]);
            if (!list.empty())
                RPT_HIP(ctx, hipMemcpy(list.data(), lists_dev + (size_t)l * cap, list.size() * sizeof(int32_t), hipMemcpyDeviceToHost));
            levels.push_back(std::move(nodes));
            lists.push_back(std::move(list));
        }
        lap("readback");
        break;
    }
    lap("free");

    // the reference's numbering: a node's eight children and their lists are appended when the node is split,
    // and the children are then visited depth first (Octree.cpp:191-246)
    std::vector<rpt_octree> out_nodes;
    std::vector<int32_t> out_tris;
    {
        size_t n_nodes_all = 0, n_entries_all = 0;
        for (size_t l = 0; l < levels.size(); l++) { n_nodes_all += levels[l].size(); n_entries_all += lists[l].size(); }
        out_nodes.reserve(n_nodes_all);
        out_tris.reserve(n_entries_all);
    }
    auto make_node = [&](const BuildNode &b, const std::vector<int32_t> &list) {
        rpt_octree o;
        std::memset(&o, 0, sizeof o);
        o.min.x = b.mn[0]; o.min.y = b.mn[1]; o.min.z = b.mn[2];
        o.max.x = b.mx[0]; o.max.y = b.mx[1]; o.max.z = b.mx[2];
        o.trisIndex = tri_index_base + (int)out_tris.size();
        o.trisCount = (int)b.list_count;
        for (int &c : o.children) c = -1;
        for (int &n : o.neighbors) n = -1;
        out_tris.insert(out_tris.end(), list.begin() + b.list_begin, list.begin() + b.list_begin + b.list_count);
        out_nodes.push_back(o);
    };
    make_node(levels[0][0], lists[0]);
    struct Frame { size_t level; int index; int out; };
    // explicit recursion: emit(level, index in level, output index)
    std::function<void(size_t, int, int)> emit = [&](size_t level, int index, int out) {
        const BuildNode &b = levels[level][index];
        if (b.first_child < 0) return;
        int child_out[8];
        for (int k = 0; k < 8; k++) {
            child_out[k] = (int)out_nodes.size();
            out_nodes[out].children[k] = node_index_base + child_out[k];
            make_node(levels[level + 1][b.first_child + k], lists[level + 1]);
        }
        const rpt_octree parent = out_nodes[out];
        for (int k = 0; k < 8; k++) {        // neighbour links (Octree.cpp:213-244): -z,+z,-x,+x,-y,+y
            const int bit[3] = {k & 1, (k >> 2) & 1, (k >> 1) & 1}, step[3] = {1, 4, 2};
            rpt_octree &c = out_nodes[child_out[k]];
            for (int axis = 0; axis < 3; axis++) {
                const int lo = 2 * axis, hi = 2 * axis + 1;
                if (bit[axis] == 0) { c.neighbors[lo] = parent.neighbors[lo]; c.neighbors[hi] = parent.children[k + step[axis]]; }
                else { c.neighbors[lo] = parent.children[k - step[axis]]; c.neighbors[hi] = parent.neighbors[hi]; }
            }
        }
        for (int k = 0; k < 8; k++) emit(level + 1, b.first_child + k, child_out[k]);
    };
    emit(0, 0, 0);

    lap("emit");
    rpt_octree *nodes_host = (rpt_octree *)std::malloc(out_nodes.size() * sizeof(rpt_octree));
    int32_t *tris_host = (int32_t *)std::malloc((out_tris.size() ? out_tris.size() : 1) * sizeof(int32_t));
    if (!nodes_host || !tris_host) {
        std::free(nodes_host);
        std::free(tris_host);
        return fail(ctx, RPT_ERR_NOMEM, "rpt_build_octree: out of host memory");
    }
    std::memcpy(nodes_host, out_nodes.data(), out_nodes.size() * sizeof(rpt_octree));
    if (!out_tris.empty()) std::memcpy(tris_host, out_tris.data(), out_tris.size() * sizeof(int32_t));
    *nodes_out = nodes_host;
    *node_count = out_nodes.size();
    *tris_out = tris_host;
    *tri_count = out_tris.size();
    return RPT_OK;
}
