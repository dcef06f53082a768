/*
 * rpt.h — C-ABI of librpt_hip.so: the per-pixel render path of the Relativity Path Tracer as
 * hand-written HIP for MI355X (gfx950).
 *
 * The reference has no plugin/FFI interface for this path; its boundary is the sequence of OpenCL
 * calls its C++ host makes.  Each entry point below replaces one of those call sites (file:line
 * under the reference root), keeps the reference's buffer layouts (rpt_layout.h) and its
 * conventions: the host owns every source array and the library copies (the reference uses
 * blocking writes everywhere); calls are externally blocking unless named *_async; one host thread
 * per context; every call returns 0 on success / nonzero on failure and never throws or aborts
 * across the boundary (the reference ignores every cl_int; here they are reported).
 *
 *   rpt_create / rpt_destroy   initOpenCL()                        CLSetup.cpp:64-135
 *   rpt_upload_scene           8x cl::Buffer + enqueueWriteBuffer   main.cpp:33-55
 *   rpt_share_scene            (none: the reference keeps one frame in flight)
 *   rpt_set_objects            per-frame write of Object[] + setArg(0)   Render.cpp:202-203
 *   rpt_set_params             initCLKernel() setArg 1,9..13; resize/interval re-binds
 *                                                                   CLSetup.cpp:150-163, Render.cpp:116-117,141
 *   rpt_set_output             cl::BufferGL(vbo) + setArg(14)       main.cpp:58, Render.cpp:114-118
 *   rpt_render                 runKernel()                          CLSetup.cpp:167-191
 *
 * Not in the reference (it never reads back, has one device and no timing): rpt_read_framebuffer,
 * rpt_last_frame_ms, rpt_timed_frames, rpt_timing_*, the *_async/stream calls, rpt_create_multi, rpt_set_rows /
 * rpt_set_tile_pattern (pixel-row tiles for multi-GPU sharding), rpt_pack_/rpt_scatter_* (the exchange's two kernels),
 * rpt_build_octree (GPU counterpart of Mesh::GenerateOctree) and the test hooks rpt_probe, rpt_probe_walk, rpt_probe_object,
 * rpt_set_debug_rgb, rpt_verify_frame, rpt_object_screen_rect / _bounds / _bounds_proposed,
 * rpt_certify_screen_bounds and rpt_mesh_segment_cull_record (the last five are host code: no device needed), and the opt-in
 * relativistic Doppler shift and searchlight beaming, which the reference does not render: rpt_set_doppler with its test hooks
 * rpt_set_debug_doppler / rpt_read_debug_doppler and rpt_probe which = 6 ("Doppler and beaming"), and the opt-in
 * equirectangular panorama camera, which the reference (a fixed pinhole looking down +z) does not have: rpt_set_projection and
 * rpt_projection_tables (host code, no device needed; DESIGN.md, "Panorama camera"), and the opt-in sky environment map, seen through a
 * Lorentz matrix of its own (the reference paints every miss one constant colour): rpt_set_environment, rpt_set_environment_frame and
 * rpt_probe which = 7 ("Environment map"), and the opt-in free-look camera — an orientation and a pinhole zoom: rpt_set_orientation,
 * rpt_set_field_of_view, and rpt_orient_objects / rpt_orient_matrix (host code, no device needed; DESIGN.md, "Free-look camera"), and the
 * opt-in event pass — per pixel the object hit, the distance, the emission event in the object's rest frame and the surface (u, v), which
 * the reference computes and discards: rpt_set_events_output, rpt_render_events / rpt_render_events_async, rpt_read_events, rpt_pick,
 * rpt_last_events_variant and rpt_last_events_exact_rcp ("Event pass"), and opt-in adaptive anti-aliasing in every camera and
 * colour mode (the reference's MSAASAMPLES is a compile-time constant, 1 as shipped): rpt_set_adaptive_aa, rpt_last_aa_refined and
 * rpt_last_aa_variant ("Adaptive anti-aliasing"), and the opt-in overlay pass — outlines, isochrones, rest-frame grids and a tint
 * by light delay drawn on the rendered frame from the event records: rpt_set_overlay, rpt_render_overlay / rpt_render_overlay_async and
 * rpt_last_overlay_pixels ("Overlay pass"), and the opt-in ray-map camera — one direction per pixel, for fisheyes, the
 * stereographic view, cube strips and calibrated lenses: rpt_set_raymap, RPT_PROJECTION_RAYMAP and rpt_raymap_fill (host code, no device
 * needed; DESIGN.md, "Ray-map camera"), and opt-in per-object time windows — objects and lights that begin and end, from which
 * piecewise-inertial worldlines are built: rpt_set_object_windows ("Time windows"), and the opt-in readout pass — seven-segment
 * displays on the objects' surfaces that show each object's own proper time: rpt_set_readouts, rpt_render_readouts /
 * rpt_render_readouts_async and rpt_last_readout_pixels ("Readout pass"), and the opt-in star-field pass — a catalogue of point
 * sources in the sky's rest frame, aberrated, Doppler-shifted and beamed as points: rpt_set_stars, rpt_render_stars /
 * rpt_render_stars_async and rpt_last_stars ("Star-field pass"), and the opt-in particle pass — point sources at a finite
 * distance, each at rest in an object's frame, seen with light delay and hidden behind what stands in front: rpt_set_particles,
 * rpt_set_particle_options, rpt_render_particles / rpt_render_particles_async and rpt_last_particles ("Particle pass"),
 * and the opt-in segment pass — straight rods at rest in an object's frame, drawn as a continuum of such point sources, so that a
 * rod bends on the screen as light delay bends it: rpt_set_segments, rpt_set_segment_options, rpt_render_segments /
 * rpt_render_segments_async and rpt_last_segments ("Segment pass").
 *
 * There is no CPU or OpenCL fallback: without a gfx950 device rpt_create fails.
 */
#ifndef RPT_H
#define RPT_H

#include "rpt_layout.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rpt_ctx rpt_ctx;

enum rpt_status {
    RPT_OK = 0,
    RPT_ERR_ARG = 1,        /* null / out-of-range argument */
    RPT_ERR_STATE = 2,      /* call made before the state it needs was set */
    RPT_ERR_SCENE = 3,      /* scene buffers fail validation (an index points outside its array) */
    RPT_ERR_DEVICE = 4,     /* HIP runtime error; see rpt_last_error */
    RPT_ERR_NOMEM = 5
};

#define RPT_TILE_ROWS 8     /* height of one pixel-row tile (the sharding unit of rpt_set_rows) */
/* rpt_render_async on a context that renders at most this many pixels per frame launches the latency kernel (43) like the
 * blocking call: so few walks do not fill the chip even with three frames in flight (measured crossover: 2560x1440). */
#define RPT_LATENCY_KERNEL_MAX_PIXELS 3000000

const char *rpt_version(void);

/* Create a context on HIP device `device_ordinal` (replaces platform/device pick, context+queue
 * creation and the run-time program build: the gfx950 code object is prebuilt). */
int rpt_create(rpt_ctx **out, int device_ordinal);
/* One context per listed device (multi-GPU hosts: SURVEY.md §8b); all or nothing — on failure every context already
 * created is destroyed, out[] is nulled and the first error is returned.  The same device may be listed more than once
 * (frame slots). */
int rpt_create_multi(rpt_ctx **out, const int *device_ordinals, int n);
void rpt_destroy(rpt_ctx *ctx);
const char *rpt_last_error(const rpt_ctx *ctx);

/* Upload the eight read-only scene arrays (copied; validated so that no index can leave its
 * array).  The Object[] in `scene` is taken as the first rpt_set_objects. */
int rpt_upload_scene(rpt_ctx *ctx, const rpt_scene_desc *scene);

/* Frames in flight (not in the reference, whose runKernel() finishes every frame before the next starts,
 * CLSetup.cpp:167-191).  One frame's critical path is the serial octree walk of its dearest pixel, which leaves
 * most of the GPU idle; a host that wants frame RATE keeps 2-3 frames in flight, one context per frame slot, each
 * with its own stream and output, rendering frame f in slot f mod n (rpt_set_objects + rpt_render_async, and
 * rpt_sync before the slot's output is consumed).  rpt_share_scene gives `ctx` the scene already resident in
 * `owner` (same device) instead of a second copy: the geometry is reference-counted, so either context may be
 * destroyed or given another scene at any time.  Object[] and the per-context settings are not shared. */
int rpt_share_scene(rpt_ctx *ctx, rpt_ctx *owner);

/* Refresh Object[] (count * 320 B, copied).  Called every frame by the reference's render(). */
int rpt_set_objects(rpt_ctx *ctx, const void *objects, int count);

/* Scalars: white_point (3 floats), ambient, width, height, interval (-1 or 0). */
int rpt_set_params(rpt_ctx *ctx, const float white_point[3], float ambient, int width, int height, int interval);

/* Output framebuffer: a device pointer to at least width*height*16 B (e.g. an interop buffer), or
 * NULL for a library-owned buffer (headless). */
int rpt_set_output(rpt_ctx *ctx, void *device_ptr_or_null);

/* Pixel-row tiles rendered by this context: tiles first_tile, first_tile+tile_step, ... of
 * RPT_TILE_ROWS rows each (default 0,1 = the whole frame).  With colour_plane != 0 the context
 * renders into a compact library-owned plane of 4 B/pixel (the packed R,G,B,1 word only), its
 * k-th local tile holding global tile first_tile + k*tile_step: the unit that is gathered. */
int rpt_set_rows(rpt_ctx *ctx, int first_tile, int tile_step, int colour_plane);
/* The general form: per period of `tile_step` tiles this context renders the `run` (a power of two, <= tile_step)
 * consecutive tiles that start at first_tile; local tile t is global tile (t / run) * tile_step + first_tile + t % run.
 * rpt_set_rows is run = 1.  Used for the WEIGHTED multi-GPU split: the root of the gather renders `run` tiles of every
 * period of run + N - 1 straight into the framebuffer (colour_plane = 0) and helper j the single tile run + j - 1 into
 * its plane — the root takes the larger share because its pixels need no exchange. */
int rpt_set_tile_pattern(rpt_ctx *ctx, int first_tile, int tile_step, int run, int colour_plane);

/* Launch on this HIP stream (hipStream_t as void*; NULL = the context's own stream).  The stream stays the caller's: it
 * must outlive every launch made on it (rpt_sync, or the caller's own synchronisation, before it is destroyed).  Switching
 * away from an external stream waits for the context's last launch through an event, not through the stream handle, and
 * rpt_destroy waits for the device — so a handle destroyed after its work has finished is never touched again. */
int rpt_set_stream(rpt_ctx *ctx, void *hip_stream);

/* Test hook: also write the tonemapped float RGB before 8-bit packing (3 floats/pixel, row-major,
 * width*height*12 B) to this device pointer; NULL disables. 1 = library-owned buffer. */
int rpt_set_debug_rgb(rpt_ctx *ctx, void *device_ptr_or_null_or_1);

/* Relativistic Doppler shift and searchlight beaming (not in the reference; DESIGN.md "Doppler and beaming"), per context, off by
 * default, not shared by rpt_share_scene.  flags: 0 (the reference), or RPT_DOPPLER_SHIFT and / or RPT_DOPPLER_BEAMING; anything
 * else is RPT_ERR_ARG.  With flags != 0 every kernel a frame would get is replaced by its Doppler twin — 3, 41, 43, 44, 48, 49 by
 * 203, 241, 243, 244, 248, 249 (rpt_last_variant reports these) — and the light colours and the surface colour seen by the camera
 * are shifted by the frequency ratios the Lorentz matrices imply.  Kernels without a twin (variants 1, 50, 51, and MSAA > 1, also
 * variant 0 on an octree whose children are not consecutive) make rpt_render / rpt_render_async / rpt_verify_frame return
 * RPT_ERR_ARG at the LAUNCH; the call itself accepts any valid flags.  With light propagation off (interval 0) or a scene at
 * rest the frame equals the reference's. */
#define RPT_DOPPLER_SHIFT 1
#define RPT_DOPPLER_BEAMING 2
int rpt_set_doppler(rpt_ctx *ctx, int flags);
/* Test hook, the shape of rpt_set_debug_rgb: while it is set and Doppler is on, frames are rendered by the un-culled Doppler
 * debug kernel (rpt_last_variant 240), which also writes 11 floats per pixel (row-major, width*height*44 B) to this device
 * pointer (1 = a library-owned buffer; NULL disables): {D_cam, D of the first light that contributed (1 if none), the reference's
 * linear colour (no Doppler) rgb, the colour after the light factors rgb, the final linear colour after S(D_cam) rgb}; a miss
 * pixel's record is all zero.  The product twins carry none of it.  rpt_read_debug_doppler copies the library-owned record of
 * the last frame (RPT_ERR_STATE if the last frame was not rendered by the debug kernel). */
int rpt_set_debug_doppler(rpt_ctx *ctx, void *device_ptr_or_null_or_1);
int rpt_read_debug_doppler(rpt_ctx *ctx, void *host_dst, size_t bytes);

/* The camera's projection (not in the reference; DESIGN.md "Panorama camera"), per context, RPT_PROJECTION_PINHOLE by default, not
 * shared by rpt_share_scene.  PINHOLE is the reference's camera (opencl_kernel.cl:55-73), params must be NULL.  EQUIRECT is a
 * panorama: params = {h_fov, v_fov, yaw} in radians with h_fov in (0, 2 pi], v_fov in (0, pi] (the floats nearest 2 pi and pi
 * included), yaw finite; NULL = {2 pi, pi, 0}, the full sphere.  Anything else is RPT_ERR_ARG at the call.
 * Pixel (x, y) of a W x H frame (row 0 the bottom, as everywhere) looks along normalize(p), p = (cos phi sin lambda, sin phi,
 * cos phi cos lambda) as three float products, with lambda = yaw + h_fov ((x + 0.5)/W - 0.5) and phi = v_fov ((y + 0.5)/H - 0.5)
 * evaluated in double and their sine and cosine rounded to float (rpt_projection_tables): yaw 0 puts the image centre on +z, the
 * reference's view direction, column x grows towards +x, and W = 2 H gives square pixels on the full sphere.
 * In panorama, variant 0 launches 344 (no mesh in Object[]) or 341 (the octree walk; with rpt_last_exact_rcp as for 41), variant 3
 * launches 303 (un-culled, what rpt_verify_frame compares with), and with Doppler on their twins 544 / 541 / 503, or the debug kernel 540
 * while rpt_set_debug_doppler is set.  They skip the per-object screen regions (proven on the pinhole's image plane only) and keep the
 * shadow-ray culls.  Every other variant, MSAA > 1 and an octree whose children are not consecutive make rpt_render /
 * rpt_render_async / rpt_verify_frame return RPT_ERR_ARG at the LAUNCH.  Back to PINHOLE, every kernel choice is the reference
 * camera's again. */
#define RPT_PROJECTION_PINHOLE 0
#define RPT_PROJECTION_EQUIRECT 1
int rpt_set_projection(rpt_ctx *ctx, int mode, const float *params);
/* Host code, no device: the two tables the panorama kernels read for a W x H frame.  cols_out gets 2 W floats {sin lambda_x,
 * cos lambda_x}, rows_out 2 H floats {sin phi_y, cos phi_y}.  mode must be RPT_PROJECTION_EQUIRECT (the pinhole has no tables), params
 * as for rpt_set_projection, 1 <= W, H and W H < 2^31; anything else is RPT_ERR_ARG. */
int rpt_projection_tables(int mode, const float *params, int width, int height, float *cols_out, float *rows_out);

/* The ray-map camera (not in the reference; DESIGN.md "Ray-map camera"): one direction per pixel, for the views that are not a function
 * of the column times a function of the row — fisheyes and dome masters, the stereographic view, a cube strip, a calibrated lens.
 * rpt_set_projection(ctx, RPT_PROJECTION_RAYMAP, NULL) selects it (params must be NULL); the directions are the context's map, which is
 * set FIRST: on a context that holds no map the call is RPT_ERR_ARG, as it was for every context before this camera existed.  (A map
 * dropped afterwards, or one of another size than the frame, is refused at the launch, below.)
 *
 * rpt_set_raymap: dirs3 holds width * height * 3 floats, row-major, row 0 the bottom as everywhere.  The map is COPIED and uploaded in
 * stream order (a frame in flight keeps the map it was launched with; the next launch sees the new one); it is per context and not shared
 * by rpt_share_scene; NULL drops it.  Pixel (x, y) looks along normalize(p), p = dirs3[3 (y W + x) ..], the float normalize of the
 * pinhole and the panorama.  p == (0, 0, 0), and only that, means the pixel has NO RAY: it is written as {x, y, rgba = 0, 0, 0, 1} —
 * black, with the constant alpha byte of every pixel — with a zero debug_rgb triple, whatever the colour mode, and it is a miss record in
 * the event pass.  A non-finite component, width < 1, height < 1 or 3 width height >= 2^31 is RPT_ERR_ARG at the call.
 * With RPT_PROJECTION_RAYMAP set, rpt_render / rpt_render_async / rpt_verify_frame / rpt_render_events[_async] return RPT_ERR_ARG at the
 * LAUNCH, with a message that starts "rpt_set_raymap:", while no map is set or the map's size is not the frame's; nothing is launched and
 * the context stays usable.  A turned camera composes as in panorama (p looks along R p); the sky's matrix, rows, tile patterns, the
 * colour plane, frames in flight and external streams need nothing: the map is addressed by global pixel.
 * Kernels (rpt_last_variant), each the panorama kernel of the same place with the direction read from the map — no object mask, the
 * shadow-ray culls kept:
 *
 *   colour \ form     un-culled   octree walk (IEEE form as for 41)   no mesh in Object[]
 *   plain              1203        1241                                1244
 *   Doppler twins      1213        1251                                1254
 *   environment        1223        1261                                1264
 *   event pass         (none)      1291                                1294               (rpt_last_events_variant)
 *
 * Variants 0, 41, 43 and 44 get the walk (or the last column without a mesh), variant 3 the un-culled form, which is what rpt_verify_frame
 * compares with.  Refused at the LAUNCH with RPT_ERR_ARG: a lens (rpt_set_field_of_view: the map has its own field of view), MSAA > 1,
 * adaptive anti-aliasing (message "rpt_set_adaptive_aa: ...": a map has no directions between its pixels), every other variant, the
 * Doppler debug kernel, and an octree whose children are not consecutive (unless Object[] holds no mesh). */
#define RPT_PROJECTION_RAYMAP 2
int rpt_set_raymap(rpt_ctx *ctx, const float *dirs3, int width, int height);
/* Host code, no device: fills dirs3_out (width * height * 3 floats, the layout above) with a standard map, everything evaluated in
 * double from the float parameters and rounded to float once per component.  With X = (2 (x + 0.5) - W) / S, Y = (2 (y + 0.5) - H) / S
 * and rho = sqrt(X^2 + Y^2), the azimuthal kinds take params = {fov, fit}: fit = 0 puts the image circle inside the frame, S = min(W, H);
 * fit = 1 makes it the frame's diagonal, S = sqrt(W^2 + H^2).  rho > 1 has no ray, (0, 0, 0); rho = 0 is (0, 0, 1); otherwise
 * p = (sin theta X / rho, sin theta Y / rho, cos theta) with
 *   RPT_RAYMAP_FISHEYE            theta = rho fov / 2                      (equidistant)      fov in (0, 2 pi]
 *   RPT_RAYMAP_FISHEYE_EQUISOLID  theta = 2 asin(rho sin(fov / 4))                            fov in (0, 2 pi]
 *   RPT_RAYMAP_STEREOGRAPHIC      theta = 2 atan(rho tan(fov / 4))                            fov in (0, 2 pi), the float nearest 2 pi excluded
 * RPT_RAYMAP_CUBE_STRIP (params NULL, W = 6 H): six square faces side by side, from the left +x, -x, +y, -y, +z, -z, each a 90-degree
 * pinhole: with a = (2 (x - f H + 0.5) - H) / H, b = (2 (y + 0.5) - H) / H pixel (x, y) of face f has p = forward + a right + b up,
 *   face      +x          -x          +y          -y          +z          -z
 *   forward   ( 1, 0, 0)  (-1, 0, 0)  ( 0, 1, 0)  ( 0,-1, 0)  ( 0, 0, 1)  ( 0, 0,-1)
 *   right     ( 0, 0,-1)  ( 0, 0, 1)  ( 1, 0, 0)  ( 1, 0, 0)  ( 1, 0, 0)  (-1, 0, 0)
 *   up        ( 0, 1, 0)  ( 0, 1, 0)  ( 0, 0,-1)  ( 0, 0, 1)  ( 0, 1, 0)  ( 0, 1, 0)
 * (the frame of a viewer standing inside the cube with +y up; the library's axes are left-handed: +x is on the right of +z).  A kind that
 * is none of these, a fov outside its range, a fit that is neither 0 nor 1, params where NULL is asked for (or the reverse), W != 6 H for
 * the strip, width < 1, height < 1, 3 W H >= 2^31 or a null output: RPT_ERR_ARG. */
#define RPT_RAYMAP_FISHEYE 0
#define RPT_RAYMAP_FISHEYE_EQUISOLID 1
#define RPT_RAYMAP_STEREOGRAPHIC 2
#define RPT_RAYMAP_CUBE_STRIP 3
int rpt_raymap_fill(int kind, const float *params, int width, int height, float *dirs3_out);

/* The sky (not in the reference; DESIGN.md "Environment map"), per context, off by default, not shared by rpt_share_scene.
 * rgb8 is an equirectangular image of width x height interleaved R, G, B bytes, row 0 the top (+y), as object textures are; it is
 * COPIED (the caller keeps its buffer).  NULL switches the sky off: the constant background and every kernel choice are those of a
 * context that never had one.  width < 1, height < 1 or 3 width height >= 2^31 is RPT_ERR_ARG.  The image may be replaced or switched
 * off while frames are in flight: the upload runs in stream order, so a frame already launched reads the image it was launched with.
 * With a sky, a primary ray that hits nothing is no longer painted (0.15, 0.15, 0.25).  Its look-back path (interval, n), n the
 * pixel's unit camera direction (pinhole or equirect), goes through the matrix E of rpt_set_environment_frame: k = E (interval, n),
 * d = normalize(k.yzw), u = 0.5 + atan2(d.z, d.x) / 2 pi, v = asin(clamp(d.y, -1, 1)) / pi + 0.5 (the textured sphere's own (u, v): the
 * image centre u = 1/2 looks down +x, +z is at u = 3/4, the seam u = 0 = 1 at -x), the colour is the bilinear fetch of the
 * object textures except that the column neighbour wraps around, and with rpt_set_doppler on and interval != 0 it goes through the
 * same colour operator with D = interval / k.x.  Then the tonemap, as for a hit pixel.  No ambient factor, no lights, no flash;
 * the sky lights nothing and shadow rays ignore it.
 * Kernels (rpt_last_variant): 641 / 643 / 644 / 603 stand in for 41 / 43 / 44 / 3, and 741 / 744 / 703 for the panorama's 341 / 344 /
 * 303; each serves Doppler off and on (no separate twin; rpt_last_exact_rcp as for 41).  rpt_verify_frame compares with 603 / 703.
 * Variants 1 and 48-51 set explicitly, MSAA > 1, the Doppler debug kernels (rpt_set_debug_doppler with Doppler on) and an octree whose
 * children are not consecutive make rpt_render / rpt_render_async / rpt_verify_frame return RPT_ERR_ARG at the LAUNCH. */
int rpt_set_environment(rpt_ctx *ctx, const unsigned char *rgb8, int width, int height);
/* E: the Lorentz matrix from the camera frame to the rest frame of the sky, row-major, four rows, t first: the layout and meaning of
 * Object.Lorentz.  For a sky at rest in the scene's frame it is the camera's inverse boost, inv_lorentz of
 * rpt_scene_get_camera_lorentz, to be set every frame next to rpt_set_objects.  NULL = the identity (the default: the sky moves with
 * the camera, a plain lookup of n).  A non-finite entry is RPT_ERR_ARG.  A kernel argument: a frame in flight keeps the matrix it
 * was launched with. */
int rpt_set_environment_frame(rpt_ctx *ctx, const float lorentz[16]);

/* The free-look camera (not in the reference, whose camera looks down +z through a fixed 90-degree lens; DESIGN.md "Free-look camera"):
 * an orientation and a pinhole zoom, per context, both off by default, not shared by rpt_share_scene.
 *
 * rpt_set_orientation: ypr = {yaw, pitch, roll} in radians, each finite (else RPT_ERR_ARG); NULL = none (the same as three zeros).
 * R = Ry(yaw) Rx(pitch) Rz(roll), evaluated in double from the float angles, with
 *     Ry = | c 0 s |    Rx = | 1  0 0 |    Rz = |  c s 0 |
 *          | 0 1 0 |         | 0  c s |         | -s c 0 |
 *          |-s 0 c |         | 0 -s c |         |  0 0 1 |
 * A direction n of the turned camera (pixel directions are formed exactly as before) is the direction R n of the camera the caller's
 * Object[] was computed for; the view direction is R (0, 0, 1).  The convention continues the panorama's yaw:
 *   yaw   = +pi/2 alone: R (0,0,1) = (1,0,0)  — the view has turned towards +x, what was on the right is in the image centre;
 *   pitch = +pi/2 alone: R (0,0,1) = (0,1,0)  — the view has turned towards +y, the camera looks straight up;
 *   roll  = +pi/2 alone: R (0,0,1) = (0,0,1), R (1,0,0) = (0,-1,0), R (0,1,0) = (1,0,0) — the view direction stays and the IMAGE turns
 *                        counter-clockwise by a quarter turn: what was up (+y) is drawn on the left.
 * The camera direction enters the path through Object.Lorentz (and leaves it through Object.InvLorentz) only, so the turn is a change
 * of basis of the camera frame, applied by the library to its COPY of every Object[] it is given from then on (rpt_set_objects, the
 * Object[] of rpt_upload_scene, the owner's objects in rpt_share_scene):
 *     Lorentz' = Lorentz diag(1, R),    InvLorentz' = diag(1, R^T) InvLorentz,    stationaryCam and everything else unchanged,
 * each entry the three-term sum, in double, of float entries times double entries of R, rounded to float once (rpt_orient_objects is
 * that arithmetic as host code).  Screen regions, their proofs, the per-object records and the shadow culls are derived from the
 * re-based objects like from any other Object[]; no kernel choice changes and nothing is refused.  The call itself re-derives them
 * at once from a kept copy of the caller's last Object[]: it takes effect at the next launch whether it comes before or after
 * rpt_set_objects.  With R = I the device holds the caller's bytes.  The sky's matrix is re-based at the launch (E' = E diag(1, R)): a
 * sky at rest in the scene stays at rest when the head turns.  In panorama the turn composes with the projection's own yaw: pixel
 * direction p of rpt_set_projection looks along R p.  The test hooks that read the context's objects (rpt_probe_object,
 * rpt_mesh_segment_cull_record, rpt_verify_frame) see the re-based ones.
 *
 * rpt_set_field_of_view: the pinhole's vertical field of view in radians, 0.01 <= v_fov <= 3.0 (else RPT_ERR_ARG); 0 = the reference's
 * lens (the default).  s = (float)tan((double)v_fov / 2); pixel (x, y) looks along normalize(s * fx2, s * fy2, 0.5f) with fx2, fy2 as
 * the reference forms them (opencl_kernel.cl:57-63): two more float products.  v_fov = (float)(pi/2) gives s = 1.0f and the
 * reference's frame bit for bit.  Frames with a lens set are rendered by the lens kernels (rpt_last_variant): 841 / 843 / 844 / 803
 * stand in for 41 / 43 / 44 / 3 (841 and 843 with IEEE forms, rpt_last_exact_rcp as for 41), 851 / 853 / 854 / 813 for their Doppler
 * twins and 861 / 863 / 864 / 823 for the environment kernels.  The culled ones run while the lens keeps every pixel inside the window
 * the screen regions are proven for (s <= 1 and s * width / height / 2 <= 2); a wider lens is rendered by the un-culled lens kernel.
 * With a lens set, the panorama (it has its own fields of view), MSAA > 1, variants other than 0, 3, 41, 43, 44, the Doppler debug
 * kernel (rpt_set_debug_doppler with Doppler on) and an octree whose children are not consecutive make rpt_render / rpt_render_async
 * / rpt_verify_frame return RPT_ERR_ARG at the LAUNCH; the call itself accepts any valid angle.  (rpt_verify_frame sets the record hook
 * aside and compares the Doppler twins, as it does without a lens: it never launches the debug kernel, so the hook does not refuse it.) */
int rpt_set_orientation(rpt_ctx *ctx, const float ypr[3]);
int rpt_set_field_of_view(rpt_ctx *ctx, float v_fov);
/* Host code, no device: the re-basing above on `count` 320-B objects (objects_out may be objects_in) and on one 4 x 4 matrix of the
 * layout of Object.Lorentz (E of rpt_set_environment_frame).  ypr = NULL or three zeros (any R that is exactly I): the output bytes
 * equal the input bytes.  A non-finite angle, a null pointer with count > 0, count < 0: RPT_ERR_ARG. */
int rpt_orient_objects(const void *objects_in, int count, const float ypr[3], void *objects_out);
int rpt_orient_matrix(const float lorentz_in[16], const float ypr[3], float lorentz_out[16]);

/* Kernel variant: 0 = default (fastest validated); the others select alternative implementations of the same path for
 * A/B measurement.  All produce identical results.
 *   0   default: 44 when the current Object[] holds no mesh; else 43 for the blocking rpt_render and for contexts of at
 *       most RPT_LATENCY_KERNEL_MAX_PIXELS, 41 for rpt_render_async above that; 1 when the octree's children are not stored
 *       consecutively
 *   1   reads the reference's Octree/triangle layouts only (any valid octree; no culling)
 *   3   derived layouts, every object tested for every pixel, 5 waves per SIMD: the NO-CULL escape hatch, and the frame
 *       rpt_verify_frame compares the culled kernels with
 *   41  every wavefront builds its own object mask from per-object image-plane rectangles (computed on the host in
 *       rpt_set_objects) with one lane-parallel test + __ballot, 6 waves per SIMD: what rpt_render_async launches
 *   43  41 with the band of tile rows that holds the meshes dispatched first (whole-frame contexts) and the latency form of
 *       the walk: triangle records asked for one iteration ahead, a leaf's first record together with its node record
 *       (a second copy of it, addressable by node index): what the blocking rpt_render launches
 *   44  41 without the octree walk compiled in (61 VGPRs, no scratch, 8 waves per SIMD): what frames without a mesh object
 *       get; asked for explicitly while Object[] holds a mesh, 41 is launched instead
 *   48, 49      41 / 43 with the triangle test's 1 / det as the IEEE division sequence whatever the scene.  41 and 43 themselves
 *               take it through the exact reciprocal (csrc/rpt_device_math.hip.h rcp_exact: the same float) when every triangle
 *               of the scene is in its domain (rpt_scene_exact_rcp), and launch 48's / 49's code otherwise
 *   50, 51      NOT bit-exact, opt-in only: 41 compiled with the arithmetic OpenCL C allows by default (fma contraction,
 *               2.5-ulp division, 3-ulp sqrt; csrc/rpt_relaxed.hip), 5 / 6 waves per SIMD.  Never chosen by variant 0.
 * Everything else — instrumented kernels (7 loop counters, 8 primary rays only, 11 per-wave timeline) and the measurement arms
 * of rounds 1-3 (26 prepass masks, 40 / 42 other occupancies, 141 / 143 round 2's walk, 60-63 persistent workgroups with LDS
 * staging and the per-workgroup ray queue, 256+ walk experiments) — is NOT in the product library:
 * `make -C relativitypathtracer_amd/csrc diag` builds librpt_hip_diag.so with them (csrc/rpt_diag_kernels.hip.h). */
int rpt_set_variant(rpt_ctx *ctx, int variant);
/* MSAASAMPLES of opencl_kernel.cl:7 — a compile-time constant of the reference, 1 as shipped; a maintainer who edits it gets
 * n x n camera rays per pixel at (x + i/n, y + j/n), summed and divided by n^2 before the tonemap (:641-648).  1 (default) = the
 * kernels above; 2..8 = the multi-sample form of the default kernel (in-wave cull; reported by rpt_last_variant as 46) or, with
 * variant 3, of the un-culled kernel (47); other variants refuse.  No reference output exists for any value but 1: the
 * arithmetic is the oracle's (tests/test_gpu_parity.py), its pin is the one-sample path's. */
int rpt_set_msaa(rpt_ctx *ctx, int samples_per_axis);
/* The kernel (a number of the list above) this context's last launch was made with; 0 before the first launch.  What
 * variant 0 resolved to: tests and bench.py name the kernel they measured from this, not from a copy of the rule. */
int rpt_last_variant(const rpt_ctx *ctx);
/* 1 if this context's last launch tested triangles with the exact reciprocal (41 / 43 on a scene inside its domain), else 0. */
int rpt_last_exact_rcp(const rpt_ctx *ctx);
/* 1 if this context's last launch was a sky split, else 0.  A split frame is two kernels on the context's stream: a fill that writes
 * {x, y, background, 0} to every pixel outside a box of 8x8 tiles, then the frame's own kernel (what rpt_last_variant reports, as ever)
 * over the box alone; the framebuffer's bytes are those of the single launch.  rect (may be NULL) receives the box in tiles, {x0, y0,
 * x1, y1} with x1 and y1 exclusive — outside it no tile's object mask (rpt_probe_tile_masks) holds an object — or four zeros.  Split are
 * frames in flight (rpt_render_async, rpt_timed_frames; never the blocking rpt_render) of more than 6 000 000 pixels:
 * plain pinhole frames of kernels 41 / 44 / 48 (not the band-first 43 / 49) with 1..64 objects whose box covers at most half of the frame's tiles, on a
 * context that renders whole frames into the 16-byte framebuffer; a lens, the panorama, a ray map, the sky image, Doppler, MSAA, time
 * windows, adaptive anti-aliasing, debug_rgb, a colour plane or rpt_set_rows / rpt_set_tile_pattern keep the single launch.  In the
 * environment, read when a context is created: RPT_SKY_SPLIT_SHARE=<percent> sets the largest box that is still split (0: never split,
 * the escape hatch), RPT_SKY_SPLIT_MIN_PIXELS=<n> the floor (frames of more than n pixels split; tests and the A/B).
 * rpt_verify_frame renders into colour planes and therefore checks the frame's kernel as ONE launch, never the box or the fill (those
 * are held against the un-culled kernel by tests/test_gpu_sky_split.py); after it this call reports 0, as of the launch it checked. */
int rpt_last_sky_split(const rpt_ctx *ctx, int rect[4]);
/* Host code, no device: 1 if every triangle the octrees' lists name has |e1| |e2| <= 2^60 (e1 = B - A, e2 = C - A in float, finite
 * vertices), the domain on which kernels 41 / 43 use the exact reciprocal; 0 if not; -RPT_ERR_ARG / -RPT_ERR_SCENE for a bad desc. */
int rpt_scene_exact_rcp(const rpt_scene_desc *s);

/* A culled-vs-un-culled self-check on the device (with Doppler on: the twin a frame would get against the un-culled twin, 203).  The default kernels drop objects per wavefront from conservatively
 * sampled screen bounds and shadow rays per wavefront from segment-vs-box tests; a wrong bound would make an object vanish from
 * a tile without any error.  rpt_verify_frame renders the context's CURRENT state (objects, parameters, rows) once with the
 * kernel a frame would get (rpt_render_async's choice, or the variant set) and once with the un-culled kernel (3) into scratch
 * buffers, compares the packed colours of every pixel on the device and returns the number of pixels that differ (0 = the cull
 * changed nothing).  The context's framebuffer is not touched.  Cost: two frames + one reduction; meant for tests, soak runs and
 * a host that wants to check a new kind of scene, not for every frame. */
int rpt_verify_frame(rpt_ctx *ctx, unsigned long long *differing_pixels);

/* The per-object cull record of the default kernel, exposed for tests (host code, needs no device): the rectangle
 * {u0, v0, u1, v1} on the camera's image plane z = 0.5 (pixel (x, y) of a W x H frame looks through
 * ((x/W - 0.5) * W/H, y/H - 0.5)) outside which no primary ray can reach `object` (one 320-B Object with its per-frame
 * Lorentz / stationaryCam fields set).  root_bounds: min.xyz, max.xyz of a mesh object's octree root, else NULL.
 * +-3e38 on every side = never culled; u0 > u1 = not visible at all. */
int rpt_object_screen_rect(const void *object, int interval, const float *root_bounds_or_null, float rect_out[4]);
/* The whole record: the rectangle, then the diagonal slabs {p_lo, p_hi} on u + v and {m_lo, m_hi} on u - v that cut its
 * corners where that pays (+-3e38 = no cut); the slabs hold for |u| <= 2, |v| <= 0.55 (frames up to 4 : 1). */
int rpt_object_screen_bounds(const void *object, int interval, const float *root_bounds_or_null, float bounds_out[8]);
/* Both calls above return what the kernel USES: the region proposed by the outline sampling of csrc/rpt_screen_bounds.hpp if
 * csrc/rpt_bounds_certify.hpp could PROVE it (no pixel of a frame of at most 4 : 1 outside it can make the kernel's float
 * arithmetic report a hit of the object; the argument is in that file's header), else the full plane — the object is then
 * tested for every pixel, as in the reference (opencl_kernel.cl:382-425).  The two calls below expose the halves, for tests
 * and tools: the raw proposal, and the proof attempt for ANY claimed region (1 = proven, 0 = not; stats_out, if not NULL,
 * receives {reason, segment tests used, deepest halving, boundary segments}: reason 0 proven, 1 non-finite input, 2 the
 * boosted directions do not cover the sphere once, 3 float noise too large, 4 ray origin inside or near the shape, 5 no
 * witness / witness outside the claim, 6 test budget exhausted, 7 a boundary point's exact ray meets the shape). */
/* Test hook (host code): the shadow-ray cull record of mesh object `object_index` of the context's current Object[] —
 * {half extents xyz of the root box as mesh_ray_misses_root uses them (< 0: no cull of this object), constant and slope of the
 * segment cull's margin (slope < 0: no segment cull: the mesh's triangles are too large for it to be provable, or a matrix is
 * too ill-conditioned), allowance of the segment's end per unit of the rest-frame origin's L1 norm and its constant part,
 * K = the mesh's largest |e1| |e2|, L = its longest edge, 1 if the mesh's lists stay inside its root box}
 * (csrc/rpt_kernels.hip.h: mesh_ray_misses_root, mesh_segment_apart; csrc/rpt_api.hip: mesh_segment_cull_record). */
int rpt_mesh_segment_cull_record(rpt_ctx *ctx, int object_index, float out[10]);
int rpt_object_screen_bounds_proposed(const void *object, int interval, const float *root_bounds_or_null, float bounds_out[8]);
int rpt_certify_screen_bounds(const void *object, int interval, const float *root_bounds_or_null, const float bounds[8], int stats_out[4]);
/* The tile bitmap of a still mesh (csrc/rpt_tile_bitmap.hpp; not in the reference): one bit per 8x8-pixel tile of the frame, 0 = no
 * primary ray of the tile can report a hit of the mesh — proven from the boxes of at most `max_boxes` (64 in a context) sub-trees of
 * its octree, for meshes whose triangles are small enough for the bound to be provable (bunny.obj is, pear.obj is not).  A context
 * builds it for an object once its record has been byte-identical in two consecutive rpt_set_objects calls, and drops it with the
 * first call in which it is not; the culled pinhole and lens kernels then skip the mesh in tiles whose bit is 0.
 * rpt_tile_bitmap_host (host code, no device): the bitmap of mesh object `object_index` of `scene` for a width x height frame under
 * lens_scale (1.0f: the reference's lens) into bits_out[words], bit ty * ceil(width / 8) + tx; boxes_or_null: n_boxes boxes (min.xyz,
 * max.xyz) to use instead of the mesh's own (tests).  1: built, 0: this object gets no bitmap, < 0: -RPT_ERR_*.  stats_out, if not
 * NULL: {boxes, boxes proven, tiles set, tiles, depth of the cut} of the sub-tree stage.  Without the caller's boxes bits_out is the
 * PRODUCT a context puts on the device: the sub-tree stage ANDed with the triangle stage — one proven region per distinct triangle of
 * the mesh, for meshes of at most 8 192 triangles — unless RPT_TILE_TRIANGLES=0 is set (a context reads it when it is created; this
 * call, which has no context, reads it on every call).
 * rpt_tile_bitmap_stage_host: one stage alone, stage 0 = the sub-tree stage, stage 1 = the triangle stage with at most `max_triangles`
 * triangles, stage 2 (FOR TESTS ONLY) = their product under that cap (what a context would build if its cap were `max_triangles`; the
 * sub-tree stage's statistics); the same returns; stats_out, if not NULL: {boxes, boxes proven, tiles set, tiles}.
 * rpt_tile_bitmap_state: out = {bit i = object i has a bitmap on the device for the current frame, bitmaps built so far, host
 * microseconds of the last build, dwords per bitmap}; bits_or_null receives the bitmap of `object_index` (an error if it has none). */
int rpt_tile_bitmap_host(const rpt_scene_desc *scene, int object_index, int interval, int width, int height, float lens_scale, int max_boxes,
                         const float *boxes_or_null, int n_boxes, uint32_t *bits_out, size_t words, int stats_out[5]);
int rpt_tile_bitmap_stage_host(const rpt_scene_desc *scene, int object_index, int interval, int width, int height, float lens_scale, int stage,
                               int max_triangles, uint32_t *bits_out, size_t words, int stats_out[4]);
/* FOR TESTS ONLY, not part of the supported interface.  The bitmap's rasterisation alone (host code): sets in bits_out[words] the tiles of a width x height frame whose square, grown by
 * a pixel and a half and scaled by lens_scale, touches the region bounds[8] = {u0, v0, u1, v1, p_lo, p_hi, m_lo, m_hi} (the four
 * diagonal sides only with `diagonals`).  1: done, 0: an empty region (nothing set), < 0: -RPT_ERR_*. */
int rpt_tile_rasterise_host(int width, int height, float lens_scale, int diagonals, const float bounds[8], uint32_t *bits_out, size_t words);
int rpt_tile_bitmap_state(rpt_ctx *ctx, unsigned long long out[4], int object_index, uint32_t *bits_or_null, size_t words);
/* Tests and diagnostics: contexts that share a scene (rpt_share_scene) share tile bitmap builds through a cache of 64 entries kept with
 * the scene; out = {bitmaps built for it, requests answered with a copy of an earlier build} since the scene's upload. */
int rpt_tile_bitmap_shared_state(rpt_ctx *ctx, unsigned long long out[2]);
/* The derived layouts of a scene as rpt_upload_scene would put them on the device, built on the host alone (no device; tests).
 * which = RPT_LAYOUT_NODES: one 64-B record per octree node in the derived, breadth-first numbering — {min.xyz, link, max.xyz, begin
 *   word, leafCount, nb[6], 0}: link = -1 for a leaf, else first child | leaf mask << 24; begin word = leafBegin | min(leafCount, 255)
 *   << 24; nb[] in the derived numbering;
 * RPT_LAYOUT_EXITS: one 32-B record per (node, side), record 6 node + side — {min.xyz, a, max.xyz, b} of the node nb[side] names: a
 *   leaf gives its box, a = its index and b = its begin word; an inner node its box, a = its link and b = RPT_EXIT_INNER; no neighbour
 *   gives zeros, a = -1 and b = RPT_EXIT_INNER (no leaf's begin word);
 * RPT_LAYOUT_HITS: one 64-B record per triangle id — normals A, B, C (9 floats), uvs A, B, C (6 floats), one spare word (0);
 * RPT_LAYOUT_NODE_INDEX: one int per node: the reference's node index -> the derived one.
 * *bytes_needed (if not NULL) receives the array's size; it is copied to `out` if out is not NULL and `bytes` holds it.
 * 1: built; 0: this scene has no derived layout (it renders with the reference-layout kernel); < 0: -RPT_ERR_*. */
#define RPT_LAYOUT_NODES 0
#define RPT_LAYOUT_EXITS 1
#define RPT_LAYOUT_HITS 2
#define RPT_LAYOUT_NODE_INDEX 3
#define RPT_EXIT_INNER 0x01ffffff
int rpt_derived_layout_host(const rpt_scene_desc *scene, int which, void *out, size_t bytes, size_t *bytes_needed);
/* Device probe: the object mask of every 8x8 tile of the current pinhole or lens frame as kernel 41 / 841 forms it, out[2 t] before and
 * out[2 t + 1] after the tile bitmaps (t = ty * ceil(width / 8) + tx; tiles = the number of tiles).  Prepares the frame as a launch does. */
int rpt_probe_tile_masks(rpt_ctx *ctx, unsigned long long *out, size_t tiles);

/* Render one frame and wait for it (the reference's runKernel + finish). */
int rpt_render(rpt_ctx *ctx);
/* Enqueue one frame on the context's stream without waiting; rpt_sync waits. */
int rpt_render_async(rpt_ctx *ctx);
int rpt_sync(rpt_ctx *ctx);

/* The event pass (not in the reference; DESIGN.md "Event pass"): a second kind of frame that holds, for every pixel, what its primary
 * ray sees, where and when — one 32-B rpt_event (rpt_layout.h): the index of the closest object hit (-1 = none, every other field 0),
 * Hit.dist (the camera-frame distance; interval * dist is the look-back time), the emission event stationaryCam + (Lorentz (interval,
 * n)) * dist of the hit object in ITS rest frame (event[0] is the proper-time coordinate the flash test of opencl_kernel.cl:479 reads)
 * and Hit.uv.  The closest hit is the frame's own: the same intersectors in the same object order with the same strict <, so the
 * records agree with the colour frame pixel for pixel.  Opt-in, per context; with it unused nothing changes.
 *
 * rpt_set_events_output: the record buffer, a caller-owned device pointer to width * height * 32 B, or NULL (the default) for a
 * library-owned buffer, allocated (and zeroed) on first use. */
int rpt_set_events_output(rpt_ctx *ctx, void *device_ptr_or_null);
/* rpt_render_events renders one event frame and waits; rpt_render_events_async enqueues it on the context's stream (rpt_sync waits).
 * Preconditions and validation are rpt_render's.  The pass uses the context's CURRENT objects, params, rows or tile pattern,
 * projection, orientation (the objects are the re-based ones, as everywhere) and lens.  Pixel (x, y) of this context's rows is written
 * at index y * width + x of the full-frame record buffer whatever colour_plane says; rows that are not this context's are not touched,
 * nor is the colour framebuffer, rpt_last_variant or rpt_last_frame_ms.  The settings of Doppler, the sky and debug_rgb are ignored:
 * they act on colour only.  The kernel (rpt_last_events_variant):
 *
 *   camera     un-culled                        octree walk + the wave's object mask        no mesh in Object[]
 *   pinhole    903                              941 (IEEE form as for 41)                   944
 *   panorama   (none needed: nothing is culled) 911 (IEEE form)                             914
 *   lens       923                              921 (IEEE form)                             924
 *
 * rpt_set_variant(3) selects the un-culled form; variants 0, 41, 43 and 44 the default choice (the walk's row with a mesh in Object[],
 * else the last column).  Frames outside the window the screen regions are proven for (wider than 4 : 1, a lens with tan(v_fov / 2) >
 * 1) get the un-culled form, as they get 3 / 803.  Only the throughput walk is built.  Refused at the LAUNCH with RPT_ERR_ARG and a
 * message that starts "rpt_render_events:" (the context stays usable): MSAA > 1, variants 1 and 48-51 set explicitly, a lens together
 * with the panorama, and an octree whose children are not consecutive (unless Object[] holds no mesh). */
int rpt_render_events(rpt_ctx *ctx);
int rpt_render_events_async(rpt_ctx *ctx);
/* Copy the first `bytes` (at most width * height * 32) of the last event frame's records to the host, after waiting for the stream.
 * RPT_ERR_STATE before the first event pass. */
int rpt_read_events(rpt_ctx *ctx, void *host_dst, size_t bytes);
/* One record of the last event frame (a host that picks with the mouse): waits for the stream and copies 32 B.  RPT_ERR_STATE before
 * the first event pass; RPT_ERR_ARG for (x, y) outside that frame and for a row that was not this context's (rpt_set_rows). */
int rpt_pick(rpt_ctx *ctx, int x, int y, rpt_event *out);
/* The event kernel (a number of the table above) the last event pass of this context ran with; 0 before the first one.  rpt_last_variant
 * keeps reporting render kernels only.  A null context: RPT_ERR_ARG, like every call here (no event kernel is numbered 1). */
int rpt_last_events_variant(const rpt_ctx *ctx);
/* Which form of that kernel ran, rpt_last_exact_rcp's question for the event pass: *exact_out = 1 if the last event pass tested triangles
 * with the exact reciprocal (941 / 911 / 921 on a scene inside its domain, rpt_scene_exact_rcp), 0 if it ran their IEEE-division form or
 * a kernel that has none (903, 923, the forms without a walk), and 0 before the first pass.  A status, like the other calls here:
 * RPT_ERR_ARG for a null context or a null exact_out. */
int rpt_last_events_exact_rcp(const rpt_ctx *ctx, int *exact_out);

/* Adaptive anti-aliasing (not in the reference; DESIGN.md "Adaptive anti-aliasing"): n x n samples where the picture has an edge, one
 * where it is flat, in every camera and colour mode.  Opt-in, per context; samples_per_axis = 1 (the default) is off, and with it off
 * nothing changes.  With n = 2..8 a colour frame (rpt_render, rpt_render_async) is two launches on the context's stream:
 *   pass A  the one-sample frame exactly as without the setting — the same kernel (rpt_last_variant), the same framebuffer bytes — which
 *           also writes its packed colours into a context-owned 4 B/pixel plane;
 *   pass B  a refine kernel (rpt_last_aa_variant) that reads that plane: a pixel is refined iff the largest absolute difference of its
 *           8-bit R, G, B to those of any of its four neighbours (x +- 1, y +- 1; neighbours outside the frame are ignored) is GREATER
 *           than `threshold` (-1 refines every pixel: full n x n supersampling; 255 refines none).  A refined pixel is rendered again
 *           with n^2 camera rays in the order of opencl_kernel.cl:641-648 — sample (sx, sy) at ((float)x + (float)sx / n, (float)y +
 *           (float)sy / n), colours summed sy outer, sx inner in float, a miss contributing the background (the sky of its own direction
 *           with rpt_set_environment), divided by n^2, tonemapped, packed — and its 16-B framebuffer pixel (and its debug_rgb triple)
 *           overwritten.  Every other pixel keeps pass A's bytes.
 * So adaptive(n, T) = where(mask_T(one-sample frame), supersampled(n), one-sample frame).  In panorama sample (sx, sy) of pixel (x, y)
 * looks along pixel (n x + sx, n y + sy) of the n W x n H panorama with the same parameters (rpt_projection_tables at that size); under a
 * lens the scaled image plane is sampled at the fractional coordinates; an orientation needs nothing.  Refine kernels (throughput forms):
 *
 *   colour \ camera    pinhole              lens                 panorama
 *   plain              1001 / 1004 / 1003   1031 / 1034 / 1033   1061 / 1064 / 1063      (octree walk + object mask, IEEE form as for 41
 *   Doppler            1011 / 1014 / 1013   1041 / 1044 / 1043   1071 / 1074 / 1073       / no mesh in Object[] / un-culled: wherever
 *   environment        1021 / 1024 / 1023   1051 / 1054 / 1053   1081 / 1084 / 1083       pass A ran un-culled, pass B does)
 *
 * Refused at the LAUNCH with RPT_ERR_ARG and a message that starts "rpt_set_adaptive_aa:" (nothing is launched, the context stays
 * usable): together with rpt_set_msaa > 1; a context restricted by rpt_set_rows / rpt_set_tile_pattern or rendering into a colour plane
 * (a tile's neighbour rows belong to another rank); the Doppler debug kernels (rpt_set_debug_doppler: 240 / 540); variants other than
 * 0, 3, 41, 43, 44; an octree the derived layout cannot hold.  rpt_set_msaa's own refusals are unchanged.  rpt_verify_frame keeps
 * comparing the one-sample pass, rpt_timed_frames keeps timing it, and the event pass is untouched.  The call itself returns RPT_ERR_ARG
 * for a null context, samples_per_axis outside 1..8 and threshold outside -1..255. */
int rpt_set_adaptive_aa(rpt_ctx *ctx, int samples_per_axis, int threshold);
/* The number of pixels pass B refined in this context's last FINISHED adaptive frame (counted on the device, one atomic add per wave,
 * copied back in stream order and read at rpt_sync or here once that copy has run); 0 before the first one and for a frame rendered with
 * the setting off.  RPT_ERR_ARG for a null context or a null `pixels`. */
int rpt_last_aa_refined(rpt_ctx *ctx, unsigned long long *pixels);
/* The refine kernel (a number of the table above) of this context's last colour frame; 0 if that frame had no pass B (or before the
 * first).  rpt_last_variant keeps reporting pass A's kernel. */
int rpt_last_aa_variant(const rpt_ctx *ctx);

/* The overlay pass (not in the reference; DESIGN.md "Overlay pass"): lines drawn ON the rendered frame from the event records — object
 * outlines, contours of the look-back time, of the hit object's own clock and of its rest-frame coordinates, and a tint by light delay.
 * Opt-in, per context, not shared by rpt_share_scene; with layers == 0 or the pass never called nothing changes.  The pass is enqueued
 * on the context's stream after a colour frame and an event frame of the same view and blends into the R, G, B bytes of the 16-B
 * framebuffer pixels in place (alpha, bytes 0-7 and 12-15, the debug planes and the record buffer are not written).  Every rule is
 * float32 and integer arithmetic without fused operations; relativitypathtracer_amd/events.py `overlay` restates them in numpy.
 *
 *   contour layers  scalar s per pixel — ISO_DELAY |(float)interval * dist|, ISO_CLOCK event[0], LATTICE event[1], event[2], event[3] per
 *                   axis with a non-zero step, ORed — and inv = 1.0f / step, computed once on the host.  cell(p) = floorf(s(p) * inv).  A HIT
 *                   pixel p is on a line iff some neighbour q of (x + 1, y), (x, y + 1) lies inside the frame, has the same object as p
 *                   and cell(q) != cell(p).  A pixel whose product s * inv is not finite or is >= 2^30 in magnitude is never on a line and
 *                   never makes its neighbour one.
 *   OUTLINES        a pixel (hit or miss) is on an outline iff some q of the same two neighbours inside the frame has a different object.
 *   DELAY_TINT      hit pixels only: d = |(float)interval * dist| (0 if not finite), x = clamp(d / t_max, 0, 1) (0 if t_max is 0), the ramp
 *                   r = clamp(1 - 2x, 0, 1), g = 1 - |2x - 1|, b = clamp(2x - 1, 0, 1), each lifted to 0.25f + 0.75f * c, times 255.0f,
 *                   rounded to nearest even, blended with tint_alpha.  tint_t_max == 0: t_max is the frame's largest d over hit pixels,
 *                   found by a reduction kernel on the same stream (a maximum is exact in any order).
 *   order           the tint, then LATTICE, ISO_CLOCK, ISO_DELAY, OUTLINES; each blends out = (c * a + old * (255 - a) + 127) / 255 per
 *                   R, G, B channel in integers, a = the layer's fourth colour byte (tint_alpha for the tint).
 *
 * rpt_set_overlay copies the description (NULL = off) and returns RPT_ERR_ARG for unknown layer bits, a step that is <= 0 or not finite for
 * a layer that is on (a lattice axis may be 0 = skipped; all three 0 is refused), and a tint_t_max that is negative or not finite.
 * rpt_render_overlay[_async]: RPT_ERR_STATE unless the context has enqueued (or finished) a colour frame and an event frame of the current
 * width x height, both after the last rpt_set_objects, rpt_set_params, rpt_set_projection, rpt_set_orientation or rpt_set_field_of_view;
 * RPT_ERR_ARG, with a message that starts "rpt_render_overlay:", for a context restricted by rpt_set_rows / rpt_set_tile_pattern or
 * rendering a colour plane (a tile's upper neighbour row belongs to another rank).  The context stays usable after either.  The buffers
 * read and written are those of rpt_set_output / rpt_set_events_output (caller-owned or the library's) that the two frames were rendered
 * into; naming another buffer after the frames is RPT_ERR_STATE too (it holds no frame).  With layers == 0 the call checks nothing, launches nothing
 * and succeeds.  Calling the pass twice on one frame blends twice: render the colour frame again for a fresh picture.
 * rpt_last_overlay_pixels: pixels whose RGBA bytes the last FINISHED overlay pass changed (counted on the device, one atomic add per workgroup,
 * copied back in stream order, read at rpt_sync or here once the copy has run); 0 before the first. */
#define RPT_OVERLAY_OUTLINES   1   /* object index differs from a neighbour's */
#define RPT_OVERLAY_ISO_DELAY  2   /* contours of the look-back time |interval * dist| */
#define RPT_OVERLAY_ISO_CLOCK  4   /* contours of event[0], the hit object's own time */
#define RPT_OVERLAY_LATTICE    8   /* contours of event[1..3], a grid at rest with the hit object */
#define RPT_OVERLAY_DELAY_TINT 16  /* delay_map's red-green-blue ramp, blended over the picture */

typedef struct rpt_overlay_desc {
    uint32_t layers;             /* OR of the above; 0 = off (default) */
    float    delay_step;         /* > 0 where its layer is on */
    float    clock_step;
    float    lattice_step[3];    /* per axis; 0 skips that axis */
    float    tint_t_max;         /* > 0, or 0 = this frame's largest delay, found on the device */
    uint8_t  outline_rgba[4], delay_rgba[4], clock_rgba[4], lattice_rgba[4];
    uint8_t  tint_alpha, _pad[3];
} rpt_overlay_desc;

int rpt_set_overlay(rpt_ctx *ctx, const rpt_overlay_desc *desc_or_null);
int rpt_render_overlay(rpt_ctx *ctx);        /* enqueue and wait */
int rpt_render_overlay_async(rpt_ctx *ctx);  /* enqueue; rpt_sync waits */
int rpt_last_overlay_pixels(rpt_ctx *ctx, unsigned long long *pixels);

/* Per-object time windows (not in the reference; DESIGN.md, "Time windows"): objects and lights that begin and end.  t0t1 holds count
 * pairs {t0, t1}, one per entry of Object[]; object i exists for emission times t IN ITS OWN REST FRAME with !(t < t0) && !(t >= t1) —
 * the coordinate the flash term uses and the event pass stores in event[0].  A primary hit, a shadow ray's occluder and a light's emission
 * event outside the window are not there (a primary ray that meets only the rejected surface of an object does not see that object:
 * no later surface is searched for).  -inf / +inf are legal and are the default; t0 >= t1 means never; a NaN bound is RPT_ERR_ARG.
 * The array is COPIED; the setting is per context and is NOT taken over by rpt_share_scene.  NULL (or count 0) clears it: the context then
 * launches exactly the kernels it launched before the setting existed.
 * While set, frames and event frames are rendered by the windowed kernels: rpt_last_variant / rpt_last_events_variant report 2000 + the
 * variant of the row of the same camera and colour whose form ran (2041, 2044, 2003; 2241.. with Doppler, 2641.. with the sky; 28xx
 * under a lens, 23xx / 25xx / 27xx in the panorama, 32xx through a ray map; events 2941.., 2921.., 2911.., 3291..).  A band-first
 * choice (43) gets the walk (2041).  With every window at its default the frame is the un-windowed frame in all 16 bytes of every pixel.
 * Refused at the LAUNCH with RPT_ERR_ARG, message "rpt_set_object_windows: ...", nothing launched: a count that is not the Object[]'s,
 * MSAA > 1, adaptive anti-aliasing, variants 1 / 50 / 51, the Doppler debug kernels, an octree whose children are not consecutive. */
int rpt_set_object_windows(rpt_ctx *ctx, const float *t0t1_or_null, int count);

/* The readout pass (not in the reference; DESIGN.md "Readout pass"): objects that display their own time.  A seven-segment display on an
 * object's surface shows offset + rate * event[0] — event[0] of the event pass: the hit object's rest-frame time at which it emitted the
 * light the pixel receives, the coordinate the flash term and the time windows act on.  A sibling of the overlay pass with the same
 * discipline: opt-in, per context, not shared by rpt_share_scene; enqueued on the context's stream after a colour frame and an event
 * frame of the same view; it blends into the R, G, B bytes of the 16-B framebuffer pixels in place (alpha, bytes 0-7 and 12-15, the debug
 * planes and the record buffer are not written).  The display is drawn OVER the picture; it is not lit or shaded.  Every rule is float32
 * and integer arithmetic, every float operation rounded on its own; relativitypathtracer_amd/events.py `readout` restates them in numpy.
 * They apply to a HIT pixel p whose object o has digits != 0; (u, v) = p's record's uv, e = its event[0].
 *
 *   value        sv = (rate * e + offset) * scale, scale = (float)10^decimals formed on the host.  neg = sv < 0.  !(fabsf(sv) < 1e9f)
 *                overflows (a NaN too); otherwise mag = (int)floorf(fabsf(sv)), and mag >= 10^(digits - neg) overflows as well.  Cell k
 *                (0 = leftmost) shows: on overflow segment g alone in every cell and no decimal point; when neg, g alone in cell 0;
 *                otherwise the digit (mag / 10^(digits-1-k)) % 10 (leading zeros are shown).  The decimal point is lit in cell
 *                digits-1-decimals when decimals > 0.  The value is per PIXEL, from p's own record: across a large moving face
 *                neighbouring pixels may show different values.  That is the relativity of simultaneity, and it is what is wanted.
 *   footprint    du_x = u(x+1, y) - u and dv_x = v(x+1, y) - v if pixel (x+1, y) is inside the frame and has the same object, else both 0;
 *                du_y, dv_y likewise from (x, y+1).
 *   sub-samples  16 of them, (i, j) in 0..3 x 0..3, a = {-0.375, -0.125, 0.125, 0.375}: us = (u + a_i du_x) + a_j du_y,
 *                vs = (v + a_i dv_x) + a_j dv_y; s = (us - u0) * inv_w, t = (vs - v0) * inv_h with inv_w = 1.0f / (u1 - u0) and inv_h formed
 *                on the host.  Inside the display iff s >= 0 && s < 1 && t >= 0 && t < 1.  cs = s * (float)digits,
 *                c = min((int)floorf(cs), digits - 1), lx = cs - (float)c.  Lit iff (lx, t) lies in [x0, x1) x [y0, y1) of a segment that
 *                cell c's mask lights.
 *   segments     in sixteenths of the cell (x0, x1; y0, y1):  a 3, 11; 13, 15   b 10, 12; 8, 14   c 10, 12; 2, 8   d 3, 11; 1, 3
 *                e 2, 4; 2, 8   f 2, 4; 8, 14   g 3, 11; 7, 9   point 13, 15; 1, 3.  Digit masks, a = bit 0 .. g = bit 6:
 *                0x3f 0x06 0x5b 0x4f 0x66 0x6d 0x7d 0x07 0x7f 0x6f.
 *   blend        n_in / n_on = the inside / the lit sub-samples.  now = blend(now, off_rgb, (off_a * n_in + 8) / 16), then
 *                now = blend(now, on_rgb, (on_a * n_on + 8) / 16); blend is the overlay's (c * a + old * (255 - a) + 127) / 255.
 *
 * rpt_set_readouts copies the array — one entry per entry of Object[] — and writes it to the device once, not per frame; NULL or count 0
 * clears the setting.  RPT_ERR_ARG, message "rpt_set_readouts: ...", the previous setting kept: a float of any entry that is not finite,
 * digits > 9, and in an entry with digits != 0: decimals > 6 or decimals >= digits, u0 == u1 or v0 == v1.
 * (A call that fails on the device, RPT_ERR_DEVICE, leaves NO setting: the table may no longer match the previous one.)
 * rpt_render_readouts[_async] follows rpt_render_overlay's rules: RPT_ERR_STATE unless the context has enqueued a colour frame and an
 * event frame of the current width x height, view (rpt_set_object_windows changes the view too) and buffers; RPT_ERR_ARG, message
 * "rpt_render_readouts: ...", for a context restricted by rpt_set_rows / rpt_set_tile_pattern or rendering a colour plane, and for a
 * count that is not the Object[]'s.  The context stays usable after either.  With nothing set the call checks nothing, launches nothing
 * and succeeds.  The pass is independent of rpt_render_overlay: either may run first and each blends over what is there; calling it twice
 * blends twice.  rpt_last_readout_pixels: pixels whose RGBA bytes the last FINISHED readout pass changed, as rpt_last_overlay_pixels. */
/* rpt_readout: include/rpt_layout.h (36 B; the scene front-end fills the same record, rpt_scene_get_readouts) */

int rpt_set_readouts(rpt_ctx *ctx, const rpt_readout *per_object_or_null, int count);
int rpt_render_readouts(rpt_ctx *ctx);         /* enqueue and wait */
int rpt_render_readouts_async(rpt_ctx *ctx);   /* enqueue; rpt_sync waits */
int rpt_last_readout_pixels(rpt_ctx *ctx, unsigned long long *pixels);

/* The star-field pass (not in the reference; DESIGN.md §19 "Star-field pass" gives every rule operation by operation): a catalogue of
 * point sources at rest in the sky's frame — the frame of rpt_set_environment_frame, whether or not a sky image is set, so stars and an
 * image stay registered — aberrated into the camera's frame, Doppler-shifted and beamed as POINT sources, and added to the miss pixels
 * of a rendered frame.  A third sibling of the overlay and the readout pass with the same discipline: opt-in, per context, not shared by
 * rpt_share_scene; enqueued on the context's stream after a colour frame and an event frame of the same view; in place into the R, G, B
 * bytes of the 16-B framebuffer pixels (alpha, bytes 0-7 and 12-15, the debug planes and the record buffer are not written).  The stars
 * are a display-space layer over the sky, as the overlay's lines are: they light nothing.
 *
 *   dir   the direction in which one looks to see the star, in the sky's rest frame (any non-zero length; normalised in double here).
 *   rgb   the star's linear colour at rest, on the scale of object colours before the tonemap: what one pixel gets when the whole star
 *         falls on it.
 *
 * In short (E' = the sky matrix as a launch re-bases it for the orientation; G = its inverse, formed in double and rounded to float once;
 * with interval == 0, G inverts E's spatial block only and D = 1): q = G (interval, dir), n = normalize(q.yzw), D = q.x / interval — a
 * star whose D is not finite or not > 0 is skipped; c = S_f(D, rgb) as rpt_set_doppler defines it, then divided by D^2 when
 * RPT_DOPPLER_BEAMING is set (a point source also loses solid angle: its flux goes with D, or D^2 without the shift, where a surface's
 * goes with D^3 or D^4); n is projected by the inverse of the camera's own pixel-to-direction map (pinhole and lens: pixel x AT X = x;
 * equirect: pixel centre at x + 0.5, column taps wrap when h_fov is the full circle); the four pixels around (X, Y) get c times their
 * bilinear weight, clamped to 65536 per tap and channel, in 2^-24 fixed point through integer atomic adds — sums that do not depend on
 * the order of arrival, so a frame is reproducible bit for bit; then every MISS pixel (record's object < 0) with a non-zero sum S gets
 * byte = min(255, byte + to_u8(min(hable(S) / hable(white_point), 1))) per channel.
 *
 * rpt_set_stars copies the catalogue, in its order (the sums do not depend on it), and writes it to the device once, in stream order, as
 * the sky image; NULL or count 0 switches the pass off.  RPT_ERR_ARG, message "rpt_set_stars: ...", the previous
 * catalogue kept: a component of dir or rgb that is not finite, a zero-length dir, a negative colour, count < 0 or count > 2^22.
 * rpt_render_stars[_async] refuses what rpt_render_overlay refuses, with messages that start "rpt_render_stars:", and also, with
 * RPT_ERR_ARG, RPT_PROJECTION_RAYMAP (a caller's ray map has no inverse) and a sky matrix that cannot be inverted.  The context stays
 * usable after a refusal.  With no catalogue the call checks nothing, launches nothing and succeeds.  Calling it twice adds the stars twice.
 * rpt_last_stars: of the last FINISHED pass, out[0] = stars with at least one of their four taps inside the frame (whatever its weight),
 * out[1] = pixels whose bytes changed; both 0 before the first. */
typedef struct rpt_star { float dir[3]; float rgb[3]; float _pad[2]; } rpt_star;   /* 32 B */
int rpt_set_stars(rpt_ctx *ctx, const rpt_star *stars_or_null, int count);
int rpt_render_stars(rpt_ctx *ctx);         /* enqueue and wait */
int rpt_render_stars_async(rpt_ctx *ctx);   /* enqueue; rpt_sync waits */
int rpt_last_stars(rpt_ctx *ctx, unsigned long long out[2]);
/* Measurement only (tools/stars_cost.py): timed != 0 brackets the two kernels of every pass with HIP events, and rpt_last_stars_ms waits
 * for the last pass and returns {splat, resolve} in milliseconds (RPT_ERR_STATE if that pass was not timed). */
int rpt_set_stars_measurement(rpt_ctx *ctx, int timed);
int rpt_last_stars_ms(rpt_ctx *ctx, float ms[2]);

/* The particle pass (not in the reference; DESIGN.md §20 "Particle pass" gives every rule operation by operation): point sources at a
 * FINITE distance, each at rest in the rest frame of one entry of Object[] — a lattice of lamps riding a body, runway lights, a dust
 * cloud, markers on a piecewise worldline — seen with light delay, aberrated, Doppler-shifted and beamed as point sources, and hidden
 * behind whatever surface stands in front of them.  A fourth sibling of the overlay, the readout and the star-field pass with the same
 * discipline: opt-in, per context, not shared by rpt_share_scene; enqueued on the context's stream after a colour frame and an event
 * frame of the same view; in place into the R, G, B bytes of the 16-B framebuffer pixels (alpha, bytes 0-7 and 12-15, the debug planes
 * and the record buffer are not written).  Particles light nothing, cast no shadow and do not hide one another: they add.
 *
 *   pos     the particle's position in the rest frame of Object[object]: the coordinates of rpt_event.event[1..3], so a particle
 *           placed on a record's event sits on the surface that pixel sees.
 *   object  the index of that object; the objects are those the frames of this view were rendered with (under rpt_set_orientation
 *           the re-based ones).
 *   rgb     the linear colour at rest, on the scale of object colours before the tonemap (as rpt_star.rgb).
 *
 * In short (L = Object[object]): w = pos - L.stationaryCam.yzw, r = |w|; the emission event lies on the camera's past light cone,
 * tau = -r (interval == -1), or on its simultaneity slice, tau = -(I0.yzw . w) / I0.x with I0 = L.InvLorentz[0] (interval == 0);
 * k = L.InvLorentz (tau, w), dist = |k.yzw| — the distance rpt_event.dist measures —, n = k.yzw / dist; a particle whose r or dist is
 * not finite or not > 0 is skipped, and so is, while rpt_set_object_windows is set, one whose emission time L.stationaryCam.x + tau lies
 * outside its object's window; D = dist / r, c = S_f(D, rgb) as rpt_set_doppler defines it, divided by D^2 when RPT_DOPPLER_BEAMING is
 * set (the star pass's point-source law) and by r^2 with RPT_PARTICLES_INVERSE_SQUARE; n is projected as a star's is (pinhole, lens,
 * equirect); each of the four pixels around (X, Y) whose record is a miss or has dist - depth_bias < record.dist gets c times its
 * bilinear weight into the star pass's fixed-point accumulator; then EVERY pixel with a non-zero sum S gets
 * byte = min(255, byte + to_u8(min(hable(S) / hable(white_point), 1))) per channel.  Integer sums: a frame does not depend on the
 * set's order.
 *
 * rpt_set_particles copies the set, in its order, and writes it to the device once, in stream order; NULL or count 0 switches the pass
 * off.  RPT_ERR_ARG, message "rpt_set_particles: ...", the previous set kept: a component of pos or rgb that is not finite, a negative
 * colour, object < 0, count < 0 or count > 2^22.  rpt_set_particle_options: flags = RPT_PARTICLES_INVERSE_SQUARE or 0, depth_bias >= 0
 * in units of dist (defaults 0, 0.0f); RPT_ERR_ARG for an unknown flag bit and a bias that is negative or not finite.
 * rpt_render_particles[_async] refuses what rpt_render_overlay refuses, with messages that start "rpt_render_particles:", and also, with
 * RPT_ERR_ARG, RPT_PROJECTION_RAYMAP, an interval other than -1 or 0 (the cone has no closed form for another) and a set whose largest
 * object index is not below the context's object count.  The context stays usable after a refusal.  With no set the call checks
 * nothing, launches nothing and succeeds.  Calling it twice adds the particles twice.
 * rpt_last_particles: of the last FINISHED pass, out[0] = particles that were not skipped and have at least one tap inside the frame
 * that passes the depth test, out[1] = pixels whose bytes changed; both 0 before the first. */
/* rpt_particle: include/rpt_layout.h (32 B) */
#define RPT_PARTICLES_INVERSE_SQUARE 1   /* divide the colour by the squared rest-frame distance r^2 */
int rpt_set_particles(rpt_ctx *ctx, const rpt_particle *particles_or_null, int count);
int rpt_set_particle_options(rpt_ctx *ctx, int flags, float depth_bias);   /* defaults 0, 0.0f */
int rpt_render_particles(rpt_ctx *ctx);         /* enqueue and wait */
int rpt_render_particles_async(rpt_ctx *ctx);   /* enqueue; rpt_sync waits */
int rpt_last_particles(rpt_ctx *ctx, unsigned long long out[2]);
/* Measurement only (tools/particles_cost.py): as rpt_set_stars_measurement / rpt_last_stars_ms, for the particle pass's two kernels. */
int rpt_set_particles_measurement(rpt_ctx *ctx, int timed);
int rpt_last_particles_ms(rpt_ctx *ctx, float ms[2]);

/* Thermal point sources (not in the reference; DESIGN.md §21 "Thermal point sources" gives the operator operation by operation): an
 * opt-in temperature per star and per particle.  S_f draws a piecewise-linear spectrum through a colour's three samples and cuts it to
 * zero beyond its outer knots, so with RPT_DOPPLER_SHIFT every source seen at D > 1.8 or D < 0.66 is black; a blackbody shifted by D is
 * a blackbody at D T and never leaves the band.  Where a source has a temperature and the shift is on, its colour rule is T_f in place
 * of S_f: with x_k = (h c / k) / (lambda_k T) at the three primaries (700.0, 546.1, 435.8 nm),
 *     o_k = c_k expm1(x_k) / (D^3 expm1(x_k / D))     RPT_DOPPLER_SHIFT
 *     o_k = c_k expm1(x_k) / expm1(x_k / D)           RPT_DOPPLER_SHIFT | RPT_DOPPLER_BEAMING: for c = A * Planck(T), A * Planck(D T)
 * D == 1 returns c bit for bit; RPT_DOPPLER_BEAMING alone is c D^4 as before; the point-source division by D^2 and the particles' 1 / r^2
 * follow unchanged; with interval == 0 or Doppler off the colour is untouched, as before.
 *
 * kelvin[i] belongs to entry i of the catalogue (the set): 0 = not thermal, the source keeps S_f; otherwise finite with
 * 500 <= T <= 1e8.  The array is per context, converted once (x_G = (h c / k) / (546.1 nm T), in double, rounded to float) and written
 * to the device once, in stream order; NULL or count 0 switches the thermal law off.  RPT_ERR_ARG, a message that starts with the
 * call's name and names the entry, the previous array kept: an entry that is not finite or outside the range, count < 0, count > 2^22.
 * Replacing the catalogue (the set) keeps the temperatures; rpt_render_stars / rpt_render_particles refuse with RPT_ERR_ARG, the context
 * still usable, while an array is set whose count differs from the catalogue's (the set's).  With no array set every launch is what it
 * was (kernels 1120 / 1130); with one, the splat is kernel 1122 / 1132: one more 4-byte load per source. */
int rpt_set_star_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count);
int rpt_set_particle_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count);

/* The segment pass (not in the reference; DESIGN.md §22 "Segment pass" gives every rule operation by operation): straight rods, each at
 * rest in the rest frame of one entry of Object[] — a lattice of rods, a wire-frame box, a ruler's edge, the track of a piecewise
 * worldline — drawn as a CONTINUUM OF PARTICLES: rgb is a linear colour per unit rest-frame length, and the element dl of a rod is a
 * particle (above) of colour rgb dl.  Every point of a rod is seen at its own emission time, so a rod is not straight on the screen: it
 * is cut into `pieces` equal parts, the pieces + 1 nodes are placed by the particle pass's rules 1-4, and between two placed nodes the
 * image is the chord, sampled about once per pixel.  A fifth sibling of the overlay, readout, star and particle passes with the same
 * discipline: opt-in, per context, not shared by rpt_share_scene; after a colour frame and an event frame of the same view; in place
 * into the R, G, B bytes.  Rods light nothing, cast no shadow and hide nothing: they add.
 *
 * In short, P = pieces, d = b - a, len = |d| / P (a segment whose len is not > 0 or not finite is skipped); node j = a + d (j / P),
 * node P = b; a node is placed as a particle at that position of colour rgb (Doppler, beaming with the point-source / D^2, the optional
 * / r^2, the window test, the projection with its n.z > 0 and 1e9 tests).  A piece needs both its nodes placed; on the panorama its
 * second node is brought within half a period Px = W (2 pi / h_fov) of the first; L = max(|X1 - X0|, |Y1 - Y0|) must be <=
 * RPT_SEGMENT_MAX_STEPS; m = max(1, ceil(L)) samples at u = (s + 0.5) / m interpolate X, Y, dist and the colour linearly, each of
 * colour c len / m, and are splatted as particles are: four bilinear taps, the seam wrap (once, either way), the frame test, the depth
 * test dist - depth_bias < record.dist or a miss, the star pass's accumulator; then the particle pass's resolve (kernel 1131).
 *
 * rpt_set_segments copies the set and writes it to the device once, in stream order; NULL or count 0 switches the pass off.
 * RPT_ERR_ARG, message "rpt_set_segments: ...", the previous set kept: a component of a, b or rgb that is not finite, a negative colour,
 * object < 0, count < 0, count * pieces > 2^21 with the pieces in force (a piece adds to one accumulator word at most 4 times, each add
 * at most 2^40: 2^21 * 4 * 2^40 < 2^64).  rpt_set_segment_options: flags = RPT_SEGMENTS_INVERSE_SQUARE or 0, depth_bias >= 0 in units
 * of dist, pieces one of 1, 2, 4, 8, 16, 32, 64 (defaults 0, 0.0f, 16); RPT_ERR_ARG for anything else and for count * pieces > 2^21
 * with the set held.  rpt_render_segments[_async] refuses what rpt_render_particles refuses (the ray-map camera, an interval other than
 * -1 or 0, a set whose largest object index is not below the object count), with messages that start "rpt_render_segments:"; the
 * context stays usable.  With no set the call launches nothing and reports zeros.  Calling it twice adds the segments twice.
 * rpt_last_segments: of the last FINISHED pass, out[0] = pieces with at least one tap of at least one sample inside the frame that
 * passes the depth test, out[1] = pixels whose bytes changed.
 *
 * Limits: clipping at the pinhole's plane and at a window's edge has the granularity of a piece; between nodes the image is a chord of
 * the true curve; a panorama piece that passes over a pole or spans half the circle is drawn badly; particle temperatures do not apply;
 * the ray-map camera is refused; the number of pieces is fixed per set, not adaptive. */
/* rpt_segment: include/rpt_layout.h (48 B) */
#define RPT_SEGMENTS_INVERSE_SQUARE 1   /* divide the colour by the squared rest-frame distance r^2 */
#define RPT_SEGMENT_MAX_STEPS 1024      /* a piece longer than this on the screen, in pixels along its longer axis, is dropped */
int rpt_set_segments(rpt_ctx *ctx, const rpt_segment *segments_or_null, int count);
int rpt_set_segment_options(rpt_ctx *ctx, int flags, float depth_bias, int pieces);   /* defaults 0, 0.0f, 16 */
int rpt_render_segments(rpt_ctx *ctx);          /* enqueue and wait */
int rpt_render_segments_async(rpt_ctx *ctx);    /* enqueue; rpt_sync waits */
int rpt_last_segments(rpt_ctx *ctx, unsigned long long out[2]);   /* pieces drawn, pixels changed */
/* Measurement only (tools/segments_cost.py): as rpt_set_particles_measurement / rpt_last_particles_ms, for the segment pass's two kernels. */
int rpt_set_segments_measurement(rpt_ctx *ctx, int timed);
int rpt_last_segments_ms(rpt_ctx *ctx, float ms[2]);

/* Lit particles (not in the reference; DESIGN.md §23 "Lit particles" gives every rule operation by operation): dust.  With
 * RPT_PARTICLES_LIT a particle's rgb is an ALBEDO, and its colour at rest is what it scatters from the scene's lights — the light loop
 * the renderer runs for a surface, with the normal taken out (a grain scatters alike in every direction).  Light delay applies on the
 * light -> grain leg as on the grain -> camera leg: with rpt_set_object_windows a lamp switched on shows its front expanding through the
 * dust (a light echo), a moving lamp's beam is aberrated, shifted and beamed, and with RPT_PARTICLES_SHADOWED a body's shadow stands in
 * the dust, tilted by light delay.
 *
 * In short, per particle that has a tap inside the frame passing the depth test (L = Object[object], tau of the particle pass): its
 * event E = (L.stationaryCam.x + tau, pos), hitPos = L.InvLorentz E; sum = rgb * ambient (RPT_PARTICLES_AMBIENT; rpt_set_params) or 0;
 * for every Object[i] with light != 0, in index order, i == object included: P = Lorentz_i hitPos, d3 = (M_i[0].w, M_i[1].w, M_i[2].w)
 * - P.yzw, len = |d3| (the light is skipped unless 0 < len <= FLT_MAX), dLF = (interval * len, d3); with windows set the light is
 * skipped unless P.x + dLF.x lies in its window; lightDir = InvLorentz_i dLF, dObj = L.Lorentz lightDir, l3 = dObj.yzw; with
 * RPT_PARTICLES_SHADOWED the pair is skipped, and counted, if the renderer's own shadow ray from hitPos along lightDir.yzw meets any
 * object but i below |lightDir.yzw| (meshes through the octree walk; occluders held against their windows); k = 1 / (1 + 0.1 |l3| +
 * 0.01 l3.l3); col = color_i, through S_f(dObj.x / dLF.x, .) while rpt_set_doppler is set; sum += (rgb * k) * col.  The particle pass
 * then goes on with sum where it had rgb (the camera factor D = dist / r, / D^2, / r^2, the taps, the resolve).  With interval == 0
 * nothing of this runs and the pass is the plain one, byte for byte: the renderer lights nothing without light propagation.
 *
 * rpt_set_particle_lighting: flags = 0 (default: the particle pass as it was, its kernels 1130 / 1132) or RPT_PARTICLES_LIT, optionally
 * with RPT_PARTICLES_SHADOWED and RPT_PARTICLES_AMBIENT.  RPT_ERR_ARG, message "rpt_set_particle_lighting: ...", the previous value
 * kept: an unknown bit, SHADOWED or AMBIENT without LIT.  Per context, not shared by rpt_share_scene.  While LIT is set
 * rpt_render_particles[_async] also refuses, the context still usable: with RPT_ERR_ARG particle temperatures (a scattered spectrum is
 * not the grain's blackbody) and, with SHADOWED and RPT_ERR_STATE, a scene whose octrees have no derived layout (what rpt_probe_object
 * refuses, with the same code).
 * rpt_last_particle_lighting: of the last FINISHED particle pass, out[0] = (particle, light) pairs that lit, out[1] = pairs a shadow ray
 * found occluded, both over the particles rpt_last_particles counts as seen; zeros for a plain pass and before the first.
 *
 * Limits: single scattering, isotropic, no extinction — grains do not shade one another or the surfaces, and the frame's surfaces do
 * not see the dust; the shadow ray starts AT the grain (there is no normal to step along), so a grain placed on a surface
 * (particles.at_events) is shadowed by that surface or not by rounding; rods (the segment pass) stay self-luminous. */
#define RPT_PARTICLES_LIT       1   /* rgb is an albedo: the grain shows what it scatters from the scene's lights */
#define RPT_PARTICLES_SHADOWED  2   /* needs LIT: a shadow ray per (grain, light), the reference's sample_light */
#define RPT_PARTICLES_AMBIENT   4   /* needs LIT: add rgb * ambient (rpt_set_params), as trace does for a surface */
int rpt_set_particle_lighting(rpt_ctx *ctx, int flags);                       /* default 0: today's pass, today's kernels */
int rpt_last_particle_lighting(rpt_ctx *ctx, unsigned long long out[2]);     /* (grain, light) pairs that lit; pairs shadowed */

/* The ballistic pass (not in the reference; DESIGN.md §24 "Ballistic particles" gives every rule operation by operation): point sources
 * with a velocity of their own — a jet, an exploding shell, debris, a gas — without one Object per velocity.  A record is a straight
 * worldline written in the rest frame of one entry of Object[], and the window of that frame's time in which the source shines; the
 * pass finds the event of the worldline on the camera's past light cone in closed form, and from there on is the particle pass: the same
 * projection, depth test, point-source Doppler law, accumulator and resolve.  A sixth sibling of the overlay, readout, star, particle and
 * segment passes with the same discipline: opt-in, per context, not shared by rpt_share_scene; after a colour frame and an event frame
 * of the same view; in place into the R, G, B bytes.  Ballistic particles light nothing, cast no shadow and hide nothing: they add.
 *
 *   pos     where the particle is at time 0 of the rest-frame clock of Object[object] (the clock of rpt_event.event[0]), in that frame's
 *           coordinates (rpt_event.event[1..3]).
 *   object  the frame the worldline is WRITTEN in.  The particle does not ride the body, and the object's own time window
 *           (rpt_set_object_windows) is NOT applied to it.
 *   rgb     the linear colour at rest in the PARTICLE's own frame, on the scale of object colours.
 *   u       the proper velocity gamma * beta in that object's rest frame: every finite u is a subluminal velocity, and 1 - beta^2 is
 *           never formed.
 *   t0, t1  the particle shines while t0 <= t < t1 on that object's clock; -infinity / +infinity = always.
 *
 * In short (L = Object[object], cam = L.stationaryCam, I = L.InvLorentz): g = sqrt(1 + u.u), beta = u / g; w0 = (pos + beta cam.x) -
 * cam.yzw, a = u.w0, r' = sqrt(w0.w0 + a a) — the camera's distance in the particle's own rest frame, gamma (r + beta.w) — and a record
 * whose r' is not finite or not > 0 is skipped; tau = g (a - r') where a <= 0 and -g (w0.w0) / (a + r') elsewhere (interval == -1: the
 * same root of the light-cone equation, each form without cancellation on its side), or -(I0.yzw.w0) / (I0.x + I0.yzw.beta) (interval ==
 * 0); w = w0 + beta tau, t = cam.x + tau, skipped unless !(t < t0) && !(t >= t1); k = I (tau, w), dist = |k.yzw|, n = k.yzw / dist,
 * skipped as a particle is; then the particle pass's colour rule with r' for r (D = dist / r', S_f or T_f, / D^2 with beaming, / r'^2
 * with RPT_PARTICLES_INVERSE_SQUARE), its projection, taps, depth test, accumulator and resolve.  With u = 0 and the window open the
 * pass is the particle pass, operation for operation.
 *
 * rpt_set_ballistics copies the set and writes it to the device once, in stream order; NULL or count 0 switches the pass off.
 * RPT_ERR_ARG, message "rpt_set_ballistics: ...", the previous set kept: a component of pos, rgb or u that is not finite, |u_k| > 1000,
 * a negative colour, object < 0, a t0 or t1 that is NaN, t0 >= t1, count < 0 or count > 2^22.  rpt_set_ballistic_options: as
 * rpt_set_particle_options, kept apart from the particle pass's (flags = RPT_PARTICLES_INVERSE_SQUARE or 0; depth_bias >= 0).
 * rpt_set_ballistic_temperatures: as rpt_set_particle_temperatures, one temperature per record (the splat is then kernel 1152 for 1150).
 * rpt_render_ballistics[_async] refuses what rpt_render_particles refuses (the ray-map camera, an interval other than -1 or 0, a set
 * whose largest object index is not below the object count, a temperature count that is not the set's), with messages that start
 * "rpt_render_ballistics:"; the context stays usable.  With no set the call launches nothing and reports zeros.  Calling it twice adds
 * the particles twice.  rpt_last_ballistics: of the last FINISHED pass, out[0] = records that were not skipped and have at least one
 * tap inside the frame that passes the depth test, out[1] = pixels whose bytes changed.
 *
 * Limits: straight worldlines only; the sources are not lit by the scene's lights (rpt_set_particle_lighting does not apply); the
 * ray-map camera is refused. */
/* rpt_ballistic: include/rpt_layout.h (48 B) */
int rpt_set_ballistics(rpt_ctx *ctx, const rpt_ballistic *records_or_null, int count);
int rpt_set_ballistic_options(rpt_ctx *ctx, int flags, float depth_bias);   /* defaults 0, 0.0f */
int rpt_set_ballistic_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count);
int rpt_render_ballistics(rpt_ctx *ctx);        /* enqueue and wait */
int rpt_render_ballistics_async(rpt_ctx *ctx);  /* enqueue; rpt_sync waits */
int rpt_last_ballistics(rpt_ctx *ctx, unsigned long long out[2]);   /* records seen, pixels changed */
/* Measurement only (tools/ballistics_cost.py): as rpt_set_particles_measurement / rpt_last_particles_ms, for the ballistic pass's two kernels. */
int rpt_set_ballistics_measurement(rpt_ctx *ctx, int timed);
int rpt_last_ballistics_ms(rpt_ctx *ctx, float ms[2]);

/* The rocket pass (not in the reference; DESIGN.md §25 "Accelerated particles" gives every rule operation by operation): point sources
 * under constant proper acceleration — the relativistic rocket, Bell's spaceships, a Born-rigid fleet, the Rindler horizon.  A record is
 * a hyperbolic worldline written in the rest frame of one entry of Object[], and the window of that frame's time in which the source
 * shines; the pass finds the event of the worldline on the camera's past light cone in closed form (+ - * / and sqrt only), and from
 * there on is the ballistic pass: the same projection, depth test, point-source Doppler law, accumulator and resolve.  A seventh sibling
 * of the overlay, readout, star, particle, segment and ballistic passes with the same discipline: opt-in, per context, not shared by
 * rpt_share_scene; after a colour frame and an event frame of the same view; in place into the R, G, B bytes.  Rockets light nothing,
 * cast no shadow and hide nothing: they add.
 *
 *   pos, object, rgb, u, t0, t1   exactly as in rpt_ballistic: the place at time 0 of the clock of Object[object], the frame the
 *           worldline is written in (its own time window is not applied), the colour at rest in the rocket's own frame, the proper
 *           velocity gamma * beta at that moment, and the window [t0, t1) held against the emission time on that clock.
 *   acc     the proper acceleration 3-vector in the rocket's own instantaneous rest frame at that moment — what the crew feels — in
 *           units where c = 1.  Every finite acc is legal; alpha^2 = acc.acc is formed from it directly, never by cancellation.
 *   reserved  must be 0.
 *
 * In short (L = Object[object], (T, C) = L.stationaryCam, I = L.InvLorentz, al2 = acc.acc): g = sqrt(1 + u.u), a0 = u.acc,
 * a = acc + u (a0 / (g + 1)): the 4-velocity (g, u) and the 4-acceleration (a0, a) at time 0.  With z = (2 / alpha) tanh(alpha s / 2)
 * and d = 1 - al2 z^2 / 4 the worldline is rational in z: X = (0, pos) + (g, u) z / d + (a0, a) z^2 / (2 d).  The state is advanced to
 * the camera's time T (G = sqrt(g^2 + 2 a0 T + al2 T^2) is gamma there), then w0 = p - C, n = u1.w0, m = a1.w0,
 * Aq = (m - 1) - (w0.w0) al2 / 4 and r' = sqrt(n^2 - Aq (w0.w0)) — the discriminant of the light-cone quadratic Aq z^2 + 2 n z + w0.w0
 * = 0 and, exactly, the camera's distance in the rocket's rest frame at emission.  Skipped unless 0 < r' <= FLT_MAX; the past root is
 * z = -(w0.w0) / (n + r') where n > 0, (r' - n) / Aq where n <= 0 and Aq < 0, and none elsewhere; skipped unless d > 0: the camera is
 * beyond the rocket's horizon.  Then tau, w, the window, k = I (tau, w), D = dist / r' and the ballistic pass's rules 5-7.  With
 * acc = 0 the rules are the ballistic pass's up to rounding (another operation order; not bit for bit).
 *
 * rpt_set_rockets copies the set and writes it to the device once, in stream order; NULL or count 0 switches the pass off.
 * RPT_ERR_ARG, message "rpt_set_rockets: entry i: ...", the previous set kept: what rpt_set_ballistics refuses, a component of acc that
 * is not finite, |acc_k| > 1000, reserved != 0.  rpt_set_rocket_options: as rpt_set_ballistic_options, kept apart from it (flags =
 * RPT_PARTICLES_INVERSE_SQUARE or 0; depth_bias >= 0).  rpt_set_rocket_temperatures: one temperature per record (the splat is then
 * kernel 1162 for 1160).  rpt_render_rockets[_async] refuses what rpt_render_ballistics refuses, with messages that start
 * "rpt_render_rockets:"; the context stays usable.  With no set the call launches nothing and reports zeros.  Calling it twice adds the
 * rockets twice.  rpt_last_rockets: of the last FINISHED pass, out[0] = records that were not skipped and have at least one tap inside
 * the frame that passes the depth test, out[1] = pixels whose bytes changed.
 *
 * Limits: constant proper acceleration only (a trip is several records with abutting windows); no rotation; the sources are not lit by
 * the scene's lights; the ray-map camera is refused. */
/* rpt_rocket: include/rpt_layout.h (64 B) */
int rpt_set_rockets(rpt_ctx *ctx, const rpt_rocket *records_or_null, int count);
int rpt_set_rocket_options(rpt_ctx *ctx, int flags, float depth_bias);   /* defaults 0, 0.0f */
int rpt_set_rocket_temperatures(rpt_ctx *ctx, const float *kelvin_or_null, int count);
int rpt_render_rockets(rpt_ctx *ctx);        /* enqueue and wait */
int rpt_render_rockets_async(rpt_ctx *ctx);  /* enqueue; rpt_sync waits */
int rpt_last_rockets(rpt_ctx *ctx, unsigned long long out[2]);   /* records seen, pixels changed */
/* Measurement only (tools/rockets_cost.py): as rpt_set_ballistics_measurement / rpt_last_ballistics_ms, for the rocket pass's two kernels. */
int rpt_set_rockets_measurement(rpt_ctx *ctx, int timed);
int rpt_last_rockets_ms(rpt_ctx *ctx, float ms[2]);

void *rpt_output_ptr(rpt_ctx *ctx);          /* device pointer of the current framebuffer */
size_t rpt_output_bytes(rpt_ctx *ctx);
void *rpt_colour_plane_ptr(rpt_ctx *ctx);    /* device pointer of the compact plane (rpt_set_rows) */
/* Render the compact colour plane into caller-owned device memory (at least
 * local_tiles*RPT_TILE_ROWS*width*4 B), e.g. the send buffer of the gather; NULL = library-owned. */
int rpt_set_plane_output(rpt_ctx *ctx, void *device_ptr_or_null);

int rpt_read_framebuffer(rpt_ctx *ctx, void *host_dst, size_t bytes);
int rpt_read_debug_rgb(rpt_ctx *ctx, void *host_dst, size_t bytes);
int rpt_last_frame_ms(rpt_ctx *ctx, float *ms);     /* device time of the last rendered frame */
/* Render `frames` frames back to back and report the average device time per frame, measured
 * with HIP events on the launch stream. */
int rpt_timed_frames(rpt_ctx *ctx, int frames, float *avg_ms);

/* Per-frame device timing over a region: after rpt_timing_begin every rpt_render[_async] brackets
 * its kernel with its own pair of HIP events on the launch stream (up to `max_frames`);
 * rpt_timing_end waits for them and returns the summed kernel time and the frame count. */
int rpt_timing_begin(rpt_ctx *ctx, int max_frames);
int rpt_timing_end(rpt_ctx *ctx, float *total_ms, int *frames);
/* The same, returning every frame's launch duration (up to `capacity`) instead of their sum. */
int rpt_timing_end_frames(rpt_ctx *ctx, float *per_frame_ms, int capacity, int *frames);
/* The same region as SPANS: when each timed launch began and ended on the device, in ms after the FIRST timed launch of `base`
 * began (base: any context of the same device whose timing region started with this one's — frames in flight run on several
 * contexts, their spans share one clock this way).  Ends the region like rpt_timing_end_frames. */
int rpt_timing_end_spans(rpt_ctx *ctx, const rpt_ctx *base, float *begin_ms, float *end_ms, int capacity, int *frames);

/* Root side of the multi-GPU exchange: expand `n_ranks` gathered colour planes (rank r's plane at
 * planes + r*plane_stride_bytes) into the 16 B/pixel framebuffer `out16` (x, y, packed colour). */
int rpt_scatter_colour_plane(rpt_ctx *ctx, const void *planes, void *out16, int width, int height,
                             int n_ranks, int plane_stride_words, int reserved);
/* The same on an explicit HIP stream (NULL = the context's launch stream): lets the root overlap the
 * reassembly of frame k with the rendering of frame k+1. */
int rpt_scatter_colour_plane_on(rpt_ctx *ctx, void *hip_stream, const void *planes, void *out16, int width, int height,
                                int n_ranks, int plane_stride_words);

/* The exchange at 3 bytes per pixel: the fourth byte of every packed colour is the constant 1 (opencl_kernel.cl:657),
 * so a rank may send 3/4 of its plane.  rpt_pack_colour_plane3_on rewrites `pixels` (a multiple of 4; a plane of
 * whole 8-row tiles always is) packed words at `plane4` as 3*pixels bytes at `plane3`, on `hip_stream` (NULL = the
 * context's launch stream); rpt_scatter_colour_plane3_on is rpt_scatter_colour_plane_on for gathered 3-byte planes
 * that lie `plane_stride_bytes` apart. */
int rpt_pack_colour_plane3_on(rpt_ctx *ctx, void *hip_stream, const void *plane4, void *plane3, size_t pixels);
int rpt_scatter_colour_plane3_on(rpt_ctx *ctx, void *hip_stream, const void *planes3, void *out16, int width, int height,
                                 int n_ranks, size_t plane_stride_bytes);
/* Reassembly for the weighted split: planes3 holds n_ranks gathered 3-byte planes plane_stride_bytes apart (slot 0, the
 * root's, is not read); the helpers' tiles are written into out16, the root's own tiles (already rendered there) are
 * left alone. */
int rpt_scatter_helper_planes3_on(rpt_ctx *ctx, void *hip_stream, const void *planes3, void *out16, int width, int height,
                                  int n_ranks, int root_run, size_t plane_stride_bytes);

/* Diagnostic variant 7 only (librpt_hip_diag.so): loop-iteration counters of the octree walk of the last frame —
 * [0..2] leaf steps / triangle tests / descent steps summed over lanes, [3..5] the same counted
 * once per executing wavefront (lane sum / (64 * wave count) = SIMD utilisation of that loop); [6] longest walk,
 * [7] walks > 32 steps, [8] sum over leaf steps of distinct nodes among the active lanes, [9] sum of active lanes,
 * [10..15] histogram of distinct nodes per step (1, 2, 3-4, 5-8, 9-16, >16). */
int rpt_read_counters(rpt_ctx *ctx, unsigned long long out[16]);

/* Diagnostic variant 11 only (librpt_hip_diag.so): ten words per wavefront of the last frame — {start, end} stamps (100 MHz
 * s_memrealtime) and the cycle / iteration accounting of the walk's loops (tools/timeline.py);
 * wave w = (blockIdx.y*gridDim.x + blockIdx.x)*4 + wave-in-block. */
int rpt_read_wave_times(rpt_ctx *ctx, unsigned long long *out, size_t max_words, size_t *words);

/* Opt-in glare (not in the reference): a linear point-spread function for the point-source passes.  While a descriptor
 * is set, rpt_render_stars, _particles, _segments, _ballistics and _rockets convolve their fixed-point accumulator with it, in exact
 * integer arithmetic, between the splat and the resolve (kernels 1170 and 1171 in place of 1121 / 1131), so that a brighter source
 * looks bigger: more of its tail clears the display's floor.  Up to RPT_GLARE_LAYERS_MAX separable Gaussian layers (weight, sigma);
 * sigma in pixels, in [0.5, 32/3]; every weight > 0; the weights become w_k = floor(weight_k 65536 + 0.5) and the core — the source's own
 * pixel — keeps w_0 = 65536 - sum w_k, which must not be negative.  rpt_set_glare refuses a NaN, a weight <= 0, a sigma out of range, a
 * negative core and a layer count outside 0 .. RPT_GLARE_LAYERS_MAX; a null descriptor or 0 layers switches glare off (the default), and
 * a context without glare launches exactly the kernels it launched before and gives the same bytes.  Glare acts at each pass's own
 * resolve on that pass's sources only, in pixel space (in a panorama it is stretched towards the poles and does not cross them; across
 * the seam of a full circle it wraps), and flux that falls outside the frame is lost.  It adds no refusal at a launch.
 * rpt_glare_taps is host code and touches no device: the 2 radius + 1 integer taps of one layer, radius = min(32, ceil(3 sigma)),
 * t[j] = floor(65536 g_j / sum g + 0.5) off the centre with g_j = exp(-j^2 / (2 sigma^2)) in double, the centre tap what is left of 65536.
 * taps65_out[RPT_GLARE_RADIUS_MAX + j] is t[j] for |j| <= radius, 0 beyond.  RPT_ERR_ARG for a sigma outside [0.5, 32/3] or a null. */
#define RPT_GLARE_LAYERS_MAX 3
#define RPT_GLARE_RADIUS_MAX 32
typedef struct rpt_glare {
    int layers;                                 /* 0 .. RPT_GLARE_LAYERS_MAX; 0 = off */
    double weight[RPT_GLARE_LAYERS_MAX];        /* doubles: the integers of rules G0 and G1 are formed from exactly what the caller wrote */
    double sigma[RPT_GLARE_LAYERS_MAX];
} rpt_glare;
int rpt_set_glare(rpt_ctx *ctx, const rpt_glare *desc_or_null);
int rpt_glare_taps(double sigma, unsigned int taps65_out[2 * RPT_GLARE_RADIUS_MAX + 1], int *radius_out);

/* GPU octree build (replaces Mesh::GenerateOctree, Mesh.cpp:5-28, and Subdivide, Octree.cpp:171-248): builds the
 * octree of the mesh whose triangles start at word `first_triangle_word` of `triangles` (the root lists every
 * triangle imported so far, as the reference's does).  All levels run on the device in one submission on the context's
 * stream (stop rule, split decisions, triangle/box classification, ordered lists); the call waits once, reads the levels
 * back and numbers them as the reference does: node order, lists, neighbour links are byte-identical to the host builder's.
 * (RPT_OCTREE_TIMING=1 in the environment prints the call's phases to stderr.)  Node and list
 * indices in the output are absolute, based at node_index_base / tri_index_base (the current lengths of the
 * host's octree and octreeTris arrays).  The two arrays are malloc()ed; release them with rpt_free_host. */
int rpt_build_octree(rpt_ctx *ctx, const rpt_float3 *vertices, size_t vertex_count, const uint32_t *triangles,
                     size_t triangle_words, size_t first_triangle_word, int node_index_base, int tri_index_base,
                     rpt_octree **nodes_out, size_t *node_count, int32_t **tris_out, size_t *tri_count);
void rpt_free_host(void *p);

/* Known-answer probes of individual device functions (tests): which = 0 intersect_triangle
 * (in 15 floats -> out 4), 1 intersect_AABB (12 -> 5), 2 createCamRay (4 -> 3), 3 hable (3 -> 3), 4 asin / atan2 of the
 * textured-sphere (u,v) (3 -> 2), 5 the walk's pure steps: exit face of a leaf and child selection, general and fast (6 -> 12),
 * 6 the Doppler kernels' colour operator S_f (5 -> 3: {D, r, g, b, flags as a float} -> the operated r, g, b),
 * 7 the sky lookup alone on the context's current environment (3 -> 5: a direction {d.x, d.y, d.z} of the sky's rest frame, normalised
 * by the probe, -> {u, v, r, g, b}; RPT_ERR_STATE without an environment),
 * 8 the thermal point sources' colour operator T_f (6 -> 3: {D, r, g, b, flags as a float, x_G} -> the operated r, g, b). */
int rpt_probe(rpt_ctx *ctx, int which, const void *host_in, void *host_out, int n);
/* Test hook, one object's functions at ray level (the oracle's counterpart: rpt_oracle_object_rays): which = 0 n 4-D rays
 * {origin4, dir4} of object `object_index`'s rest frame through its intersector in the general form of opencl_kernel.cl:312-359 /
 * 200-308 (8 floats in, {hit, dist, normal.xyz, uv.xy, 0} out); 1 n shadow rays {origin4, dir4, lightDist} of the camera frame
 * through sample_light (:488-545) with light `object_index` (9 in; out 2 = occluded as the un-culled kernel decides it, and as the
 * culled kernels do — the same wave-level segment culls as in a frame); 2 the transforms of :75-104 on n vectors (4 in, 16 out:
 * transformPoint(InvM), transformPoint4D(Lorentz), transformDirection(InvM), applyTranspose(InvM)); 3 n primary rays given by
 * their camera direction through the form the default kernels use (3 in, 8 out as in 0). */
int rpt_probe_object(rpt_ctx *ctx, int which, int object_index, const float *host_in, float *host_out, int n);
/* Test hook (csrc/rpt_device_math.hip.h rcp_newton / rcp_exact): every float s with lo <= |s| <= hi (0 < lo <= hi <= 2^127), both signs,
 * through the three reciprocal forms on the device, compared bit for bit with IEEE 1.0f / s.  counts_out = {values compared,
 * mismatches of form 1, 2, 3, mismatching values seen}; the first max_samples mismatches go to samples_out as {s, mask of the forms
 * that missed: 1, 2, 4}. */
int rpt_probe_reciprocal(rpt_ctx *ctx, float lo, float hi, unsigned long long counts_out[5], float *samples_out, int max_samples);
/* Test hook, the octree walk at ray level: n rays {origin.xyz, dir.xyz} in the object space of mesh object `object_index` of the
 * current Object[] go through the three walks of the product library — the reference's layouts (opencl_kernel.cl:200-308 as
 * written), the throughput walk of kernel 41 and the latency walk of kernel 43 — and host_out receives 3 x 8 floats per ray:
 * {hit, dist, normal.xyz, uv.xy, 0} per walk, the distance re-measured from the object's origin as :303-305 does.  The three
 * must agree bit for bit (tests/test_gpu_kat.py). */
int rpt_probe_walk(rpt_ctx *ctx, int object_index, const float *host_rays, float *host_out, int n);
#ifdef __cplusplus
}
#endif
#endif /* RPT_H */
