"""Float64 model of what a pixel goes through besides the octree walk: spheres, cubes, the choice of the nearest object, the boost
into each rest frame, the flash, the time windows, the texture fetch, a mesh hit's normal and (u, v), and the light-delay shading — TEST
INFRASTRUCTURE.

A helper, no tests in it.  Plain numpy, float64 throughout, written from the geometry and from special relativity, as
tests/mesh_truth.py is for meshes.  It shares nothing with oracle/, tests/native/*.c or csrc/ but DATA: the Object records' M, InvM,
Lorentz, InvLorentz, stationaryCam, type, colour, light flag and flash fields (float32 values taken as float64), the per-pixel float32
directions, the windows, `ambient`, `white_point` and `interval`, the texture pool's bytes with each object's textureIndex, textureWidth
and textureHeight, and mesh_truth.arrays' vertices, normals, uvs and triangle words.  It imports none of those restatements and calls
none of their entry points.  tests/test_primitive_ground_truth.py holds the CPU restatements against it, tests/test_gpu_primitive_ground_truth.py the device.

Rules
-----
Frames.  All frames share one origin event; Lorentz_i takes camera-frame coordinates (t, x, y, z) to object i's rest frame, InvLorentz_i
back, and stationaryCam_i is the camera event in object i's rest frame.
 * Ray.  The events seen along unit direction n are cam + s (interval, n), s >= 0, in the camera frame; in object i's rest frame
   stationaryCam_i + s Lorentz_i (interval, n).  s is the same parameter for every object: it is the record's `dist`.
 * Shapes.  The unit sphere and the cube [-1, 1]^3 in object space (InvM applied to the spatial part), by the exact quadratic and the
   exact slab test.  An origin inside a shape sees the far wall.  A sphere root counts when it lies more than EPSILON = 1e-7 object-space
   units ahead of the origin (the sphere's rule), a cube face at s >= 0.  The nearest s over all objects wins; of equal s the first
   object.  Mesh objects take part through mesh_truth.brute_force (first hit's object and distance, and as occluders).
 * Record.  event = stationaryCam + s dir4 in the hit object's rest frame.  Sphere: (u, v) = (0.5 + atan2(z, x) / 2 pi, asin(y) / pi + 0.5)
   of the object-space point.  Cube: (a + 1) / 2 of the two in-face coordinates, in the face order x: (y, z), y: (x, z), z: (x, y).
   The normal is normalize(InvM^T g): g the object-space point for the sphere (OUTWARD also when seen from inside), -sign(d_a) e_a for
   the cube face on axis a (AGAINST the ray, also from inside).  A mesh hit takes both from mesh_truth.hit_attributes: the vertex normals
   interpolated by the barycentrics, through InvM^T, normalised (as the mesh gives them: not turned against the ray), and the corners' uv
   entries interpolated likewise.  A mesh without `vt` lines reads the one padded entry the arrays hold at every corner: data, not a rule.
 * Texture.  Texel (x, y) of a W x H image is its RGB bytes / 255 at byte textureIndex + 3 (W y + x) of the pool.  With U = W u,
   V = H (1 - v) (row 0 is v = 1; no half-texel offset, no wrap), x0 = min(floor U, W - 1), y0 = min(floor V, H - 1), a = U - x0, b = V - y0,
   x1 = min(x0 + 1, W - 1), y1 = min(y0 + 1, H - 1):   sample = (1 - b) [(1 - a) T(x0, y0) + a T(x1, y0)] + b [(1 - a) T(xl, y1) + a T(x1, y1)],
   xl = x0 — but see "Exception, the reference's" below for the last column.  c, the colour the shading starts from, is the sample, or
   the object's `color` without a texture, doubled by the flash.  (u, v) outside [0, 1]^2 is outside the rule (the reference reads
   whatever lies there in the pool): ill-conditioned by name, not modelled.
 * Flash.  The colour doubles where event[0] - period floor(event[0] / period) < duration (period > 0).
 * Windows.  A hit exists iff t0 <= event[0] < t1 on the object's own clock — an object whose candidate hit is outside its window is
   not there for this ray at all (its far wall does not show either).  The same holds for an occluder's crossing event and for a
   light's emission event.
 * Shading (interval != 0), for each light l != hit object: start from the hit event moved 0.001 along the normal in the hit object's
   rest frame, no change of time.  In the LIGHT's rest frame the lamp's centre p_l (M's translation) is at rest, so the emission event on
   the hit event's past light cone is (t_hit + interval |p_l - x_hit|, p_l): the retarded-time condition, solved in that one frame.  The
   displacement D between the two events is carried to the hit object's frame and must be null there (`NullConeError` otherwise: the
   model's own check).  The light counts iff its emission event is inside its window, the normal faces it (n . D_xyz > 0 in the hit
   object's frame) and no object other than the light — the hit object included — crosses the OPEN segment hit -> emission, each occluder
   tested in its own rest frame with the shape rules above (parameter tau in (0, 1) of the segment), crossing event inside its window.
   Weight k = cos(theta) / (1 + 0.1 r + 0.01 r^2), r the spatial length of D in the hit object's frame.
   colour = c (ambient + [hit object is a light]) + sum_l c k c_l;  interval == 0: colour = c (1 + [is a light]);  a miss: (0.15, 0.15, 0.25).
   Then Hable's curve over the white point's, clamped at 1.  For a mesh hit the normal of the 0.001 offset, of the facing test and of cos(theta)
   is the interpolated one, and the hit mesh is an occluder of its own segment through brute_force like any other mesh.

Bounds — derived, not tuned  (u = 2^-24)
----------------------------------------
csrc/rpt_bounds_certify.hpp section 2 (tests/test_float_error_bounds.py): a float sphere hit is an exact hit of the sphere of
R^2 = 1 + 32u (|o|^2 + 1); a float cube hit lies in [-m, m]^3, m = 1 + 4u (1 + |o|max).  Section 1: the object-space direction handed to
the intersectors differs from the exact InvM3 Lorentz (interval, n) by at most ERR_i = 24u sum_k |InvM_ik| sum_j |Lorentz_kj| per
component; over the path to the far side of the shape that moves the ray sideways by at most (|ERR| / |d|) (|o| + 2), which joins the
slack of the radius / the half width.  So the float distance lies between the exact distances to the shape grown and shrunk by that
slack: with s+ and s- those two,
    |dist_f - s|  <=  tol_s  =  max(|s+ - s|, |s- - s|)  +  8u s          (the divide by the scale, the square root, the quadratic's sums)
    |event_f - event|_k  <=  |dir4_k| tol_s  +  8u (|stationaryCam_k| + s sum_j |Lorentz_kj|)      (a 4-term dot, a product, a sum)
    |uv_f - uv|  <=  |uv(s+) - uv(s-)|  +  (tol_p + 8u (1 + |o| + s |d|)) J
with tol_p = |d| tol_s the object-space move of the hit point and J the Jacobian of (u, v): 1 / 2 for the cube, 1 / (pi rho) for the
sphere (v's; u's is half that), rho the distance of the point from the sphere's axis through its poles in object space, plus 8u for the
4 ulp OpenCL leaves asin and atan2.  u of the sphere is compared modulo 1 (the seam at atan2 = pi).  A mesh hit takes mesh_truth's dt
(its docstring) for tol_s, the direction budget joining dQ, and tol_normal and tol_uv from mesh_truth.hit_tolerances with the same
budget as extra_dq and the 4-D ray's direction length as world_dirlen; its (u, v) is compared where mesh_truth.well_conditioned passes the hit.
The colour's chain (two more boosts with cancellation, the weight, the tonemap) is not derived here: tests/test_primitive_ground_truth.py
measures it on the CPU oracle and asserts 8 x that value, as tests/test_events_model.py does for the null-cone residual.  Two terms come on
top of that constant per pixel (`rgb_extra`, absolute, 0 for an untextured sphere or cube), both derived:
 * texture: the sample is continuous and piecewise bilinear in (U, V), so while W tol_u < 1 and H tol_v < 1
       |dc|  <=  W tol_u Gx + H tol_v Gy + 8u,
   Gx / Gy the largest differences between horizontally / vertically adjacent texels of the 3 x 3 neighbourhood of (x0, y0), per channel
   (in the last column Gy + Gx stands for Gy: the exception below).  Otherwise the pixel has no finite texture term: ill-conditioned.
 * normal, mesh hits: tol_normal moves cos(theta) of a lamp by at most tol_normal, its term by the factor 1 -+ tol_normal / cos(theta);
   a lamp with |cos(theta)| <= tol_normal may face either way: ill-conditioned ("light near the horizon of the surface").
   Both are carried through the tonemap by evaluating the shading at c -+ dc and k (1 -+ rho): Hable's curve is increasing for x >= 0, so
   the two ends bound the colour — an interval, not an estimate.  tol_normal charges every barycentric error to the most unequal vertex
   normals (mesh_truth), so the interval is wide on a mesh (median 3 % of a channel on the pear): wrong normals or uv corners are
   still caught (the tests that bite), a slip of a few per mille in a mesh hit's weight is not.
END_MARGIN and SHADOW_SLACK, set for spheres and cubes, sufficed for a mesh hit's own segment too: the 0.001 offset is 50 x the slack, a
start within END_MARGIN of the hit mesh's own triangles is flagged like any crossing at the segment's end, and every committed mesh case keeps the caps
(the concave bunny 94 %).  The offset taken along the FACE normal instead of the interpolated one moves no well-conditioned pixel of any
committed case beyond its bound, so no test claims to catch it.

Conditioning
------------
A float program cannot be held to the exact answer where the answer turns on the last bits.  `frame` returns, per pixel, the figures that
say so (`figures`), each verdict by name (`why`), and two summaries.  `well_rec` (records): the exact, the grown and the shrunk model
name the same object and the same cube face; the second object is more than MIN_GAP (relative) behind; |cos| at the hit >= MIN_COS; the
ray is more than EDGE_MARGIN (object units along it) from where another cube face would decide; no origin is within ORIGIN_MARGIN (object
units) of a shape's surface, the sphere's EPSILON rule included; no event time is within TIME_MARGIN (relative to the magnitudes that
formed it) of a window's end; and the hit HAS a finite bound (a mesh hit edge-on to its triangle has none: ill-conditioned, not
passed).  `well_col` (colours) in addition: the flash phase is more than FLASH_MARGIN off its boundary; for each
light |cos theta| >= MIN_COS_LIGHT, the emission time is clear of the window's ends, no occluder's verdict differs between grown and
shrunk (grown there by SHADOW_SLACK more: the segment starts from a float hit point), no occluder crosses within END_MARGIN of the segment's
ends or through a cube's edge, and the segment's line stays more than mesh_truth.MARGIN (barycentric) from every edge line of a
mesh occluder's triangles that could decide it; a textured sphere's u is more than tol_u from the seam (the fetch does not wrap: columns
0 and W - 1 meet there discontinuously), (u, v) lies in the unit square, the texture term has a finite bound, the sample is clear of the
last texel column's discontinuities (below), and a mesh hit passes mesh_truth.well_conditioned (edge margin, |cos|, second hit, t floor).  A channel at the tonemap's clamp is a figure only: min(x, 1) is continuous.
`candidates` says which objects (or a miss) a float program may name on a pixel that is not well-conditioned: the winners of the three
models, every object within 2 MIN_GAP of the front, and — where an object's verdict itself may go either way (a window's end, an origin
at a surface, a ray through a cube's edge) — everything the ray meets, or nothing.
Exception, the reference's: a ray exactly through a cube's edge is left to neither face (both in-face tests are strict), so a float
program following the reference misses the cube there; the model hits it, marks the pixel, and allows the miss.
Exception, the reference's: the texture fetch steps x -> x + 1 (clamped), y -> y + 1 (clamped), x -> x - 1 (clamped at 0) between its four
taps, so in the LAST column (x0 = W - 1, W >= 2) the lower-left tap is column xl = W - 2, not W - 1: there the sample jumps where U
crosses W - 1 and where V crosses a row boundary 1 .. H - 1, and down the column it changes by a horizontal difference as well as a
vertical one.  Oracle and device follow the reference; the model takes xl = max(x1 - 1, 0) as the rule, widens the bound there and marks
pixels within the (u, v) bound of those lines ("last texel column's boundary").

What the model does not reach: (u, v) outside the unit square; a texture so fine, or a shape so unequal, that the derived (u, v) bound
spans a texel (the needles of scene_fuzz's ellipsoids under an 800 x 400 texture); a mesh hit's weight to better than tol_normal / cos(theta).
"""
from __future__ import annotations

import numpy as np

import mesh_truth

U = 2.0 ** -24
EPSILON = 1e-7
SPHERE, CUBE, MESH = 0, 1, 2
BACKGROUND = (0.15, 0.15, 0.25)
MIN_GAP = 1e-3            # relative gap in s to the second object
MIN_COS = 0.05            # |cos| between the ray and the normal at the hit
ORIGIN_MARGIN = 1e-3      # object units: distance of a ray origin from a surface
TIME_MARGIN = 1e-5        # relative: an event time from a window's end
FLASH_MARGIN = 1e-4       # in units of the period
MIN_COS_LIGHT = 1e-3      # |cos theta| of a light
END_MARGIN = 2e-4         # in tau: an occluder's crossing from the segment's ends
SHADOW_SLACK = 2e-5       # object units: extra growth of occluders for the shadow verdict's conditioning
CLAMP_MARGIN = 1e-5
EDGE_MARGIN = 1e-5        # object units along the ray: a cube hit from where another face would decide
ROUNDINGS = 8.0


class NullConeError(AssertionError):
    pass


def object_types(objs):
    """rpt_layout.h's type codes as this model names them (sphere 0, cube 1, mesh 2)."""
    return objs["type"].astype(np.int64)


# ---- shapes --------------------------------------------------------------------------------------------------------------------------

def _object_ray(obj, o4, d4):
    A = obj["InvM"].astype(np.float64)
    o3 = o4[..., 1:] @ A[:3, :3].T + A[:3, 3]
    d3 = d4[..., 1:] @ A[:3, :3].T
    return o3, d3


def _dir_budget(obj):
    """Section 1's ERR as a length: |24u sum_k |InvM_ik| sum_j |Lorentz_kj||."""
    A = np.abs(obj["InvM"].astype(np.float64)[:3, :3])
    L = np.abs(obj["Lorentz"].astype(np.float64)).sum(axis=1)[1:]
    return float(np.linalg.norm(24.0 * U * (A @ L)))


def _sphere(o, d, grow, extra):
    """s of the unit sphere's first root more than EPSILON ahead (inf: none); aux: both roots times |d| (object units)."""
    a = np.einsum("ij,ij->i", d, d)
    b = np.einsum("ij,ij->i", o, d)
    oo = np.einsum("ij,ij->i", o, o)
    R = np.ones_like(oo)
    if grow:
        R = np.sqrt(np.maximum(1.0 + grow * 32.0 * U * (oo + 1.0), 0.0)) + grow * extra
        R = np.maximum(R, 0.0)
    disc = b * b - a * (oo - R * R)
    with np.errstate(invalid="ignore", divide="ignore"):
        sq = np.sqrt(disc)
        s1, s2 = (-b - sq) / a, (-b + sq) / a
        la = np.sqrt(a)
        s = np.where(s1 * la > EPSILON, s1, np.where(s2 * la > EPSILON, s2, np.inf))
    s = np.where(disc >= 0.0, s, np.inf)
    s = np.where(np.isfinite(s), s, np.inf)
    with np.errstate(invalid="ignore"):
        near = np.where(disc >= 0.0, np.minimum(np.abs(s1 * la - EPSILON), np.abs(s2 * la - EPSILON)), np.inf)
    near = np.minimum(np.where(np.isfinite(near), near, np.inf), np.abs(np.sqrt(oo) - 1.0))
    return s, near


def _cube(o, d, grow, extra):
    """s of the cube's entry face (exit face for an origin inside), face axis, inf / -1: none."""
    m = np.ones(len(o))
    if grow:
        m = np.maximum(1.0 + grow * (4.0 * U * (1.0 + np.abs(o).max(axis=1)) + extra), 0.0)
    m = m[:, None]
    with np.errstate(invalid="ignore", divide="ignore"):
        t1, t2 = (-m - o) / d, (m - o) / d
        tn, tf = np.minimum(t1, t2), np.maximum(t1, t2)
        bad = np.isnan(tn).any(axis=1)
        tnear, tfar = tn.max(axis=1), tf.min(axis=1)
        inside = (np.abs(o) < m).all(axis=1)
        hit = ~bad & (tnear <= tfar) & np.where(inside, tfar >= 0.0, tnear >= 0.0)
    s = np.where(hit, np.where(inside, tfar, tnear), np.inf)
    # the edge margin: how far the second slab is from deciding instead (in s, times |d|: object units along the ray)
    with np.errstate(invalid="ignore"):
        tn2, tf2 = np.sort(np.where(np.isnan(tn), -np.inf, tn), axis=1)[:, 1], np.sort(np.where(np.isnan(tf), np.inf, tf), axis=1)[:, 1]
        edge = np.where(hit, np.where(inside, tf2 - tfar, tnear - tn2), np.inf) * np.linalg.norm(d, axis=1)
        edge = np.where(np.isnan(edge), 0.0, edge)
    axis = np.where(inside, np.argmin(np.where(np.isnan(tf), np.inf, tf), axis=1), np.argmax(np.where(np.isnan(tn), -np.inf, tn), axis=1))
    near = np.abs(np.abs(o) - 1.0).min(axis=1)                 # (distance from a face PLANE: a lower bound of the distance from the surface)
    near = np.where((np.abs(o) < 1.0 + 2 * ORIGIN_MARGIN).all(axis=1), near, np.inf)
    return s, np.where(hit, axis, -1), near, edge


def _shape(ctx, i, o4, d4, grow, extra_slack=0.0):
    """Object i against rays o4 + s d4 of its own rest frame: (s, cube face axis or -1, origin's distance from the surface, distance
    along the ray to where another cube face would decide — inf for the other shapes)."""
    obj = ctx["objs"][i]
    o3, d3 = _object_ray(obj, o4, d4)
    kind = int(ctx["types"][i])
    n = len(o3)
    extra = 0.0
    if grow:
        with np.errstate(invalid="ignore", divide="ignore"):
            extra = ctx["budget"][i] / np.linalg.norm(d3, axis=1) * (np.linalg.norm(o3, axis=1) + 2.0)
        extra = np.where(np.isfinite(extra), extra, 0.0) + extra_slack
    if kind == SPHERE:
        s, near = _sphere(o3, d3, grow, extra)
        return s, np.full(n, -1), near, np.full(n, np.inf)
    if kind == CUBE:
        return _cube(o3, d3, grow, extra)
    ids, tris = ctx["mesh"](i)
    bf = mesh_truth.brute_force(np.hstack([o3, d3]), tris, grow=(grow or None))
    if not grow:
        ctx["last_bf"] = (i, bf, tris, o3, d3)
    return (np.where(bf["hit"], bf["t"], np.inf), np.full(n, -1), np.where(np.isfinite(bf["t_edge"]), bf["t_edge"] * np.linalg.norm(d3, axis=1), np.inf),
            np.full(n, np.inf))


def _mesh_tol(ctx):
    """mesh_truth's dt of the last exact brute force, in s: the float triangle test's error along the ray (its docstring), the
    direction budget joining dQ."""
    i, bf, tris, o3, d3 = ctx["last_bf"]
    j = np.where(bf["hit"], bf["tri"], 0)
    A = tris[j, 0]
    e1, e2 = tris[j, 1] - A, tris[j, 2] - A
    l1, l2 = np.linalg.norm(e1, axis=1), np.linalg.norm(e2, axis=1)
    area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
    tau = np.linalg.norm(o3 - A, axis=1)
    dlen = np.linalg.norm(d3, axis=1)
    t_len = np.where(bf["hit"], bf["t"], 0.0) * dlen
    with np.errstate(invalid="ignore", divide="ignore"):
        extra = ctx["budget"][i] / dlen * (np.linalg.norm(o3, axis=1) + t_len)
        dq = 27.2 * U * tau * l1 * l2 / (area2 * bf["cos"]) + U * (tau + 2.1 * t_len + 2.1 * np.maximum(l1, l2)) + extra
        dt = dq / bf["cos"] / dlen
    return np.where(bf["hit"] & np.isfinite(dt), dt, np.inf)


def _window_in(windows, i, t):
    if windows is None:
        return np.ones(t.shape, dtype=bool)
    return (t >= windows[i, 0]) & (t < windows[i, 1])


def _window_dist(windows, i, t, scale):
    """Relative distance of t from the nearer FINITE end of window i (inf without one)."""
    if windows is None:
        return np.full(t.shape, np.inf)
    out = np.full(t.shape, np.inf)
    for end in windows[i]:
        if np.isfinite(end):
            out = np.minimum(out, np.abs(t - end) / np.maximum(scale, 1e-300))
    return out


# ---- the frame -----------------------------------------------------------------------------------------------------------------------

def context(objs, windows=None, mesh_arrays=None, textures=None):
    """What the model reads of a scene: `objs` the Object records (scene.OBJECT_DTYPE; a corrupted copy is as good), `windows` (n, 2) or
    None, `mesh_arrays` mesh_truth.arrays(scene) when the scene has mesh objects, `textures` the pool's bytes when an object is textured
    (default: the arrays' own)."""
    objs = np.asarray(objs).reshape(-1)
    cache = {}
    if textures is None and mesh_arrays is not None:
        textures = mesh_arrays.get("textures")
    arrays = None
    if mesh_arrays is not None:
        arrays = dict(mesh_arrays)
        arrays["objects"] = objs

    def mesh(i):
        if i not in cache:
            a = dict(mesh_arrays)
            a["objects"] = objs
            cache[i] = mesh_truth.mesh_triangles(a, i)
        return cache[i]
    w = None if windows is None else np.asarray(windows, dtype=np.float64)
    return {"objs": objs, "types": object_types(objs), "windows": w, "mesh": mesh, "budget": [_dir_budget(o) for o in objs], "arrays": arrays,
            "textures": None if textures is None else np.asarray(textures, dtype=np.uint8).reshape(-1),
            "L": objs["Lorentz"].astype(np.float64), "IL": objs["InvLorentz"].astype(np.float64), "sc": objs["stationaryCam"].astype(np.float64)}


def _first_hit(ctx, ray4, grow):
    """Per object the candidate s along camera-frame rays (interval, n), windowed: S (n_obj, N), faces, near, event times."""
    n_obj, N = len(ctx["objs"]), len(ray4)
    S = np.full((n_obj, N), np.inf)
    F = np.full((n_obj, N), -1)
    near = np.full((n_obj, N), np.inf)
    wdist = np.full((n_obj, N), np.inf)
    raw = np.full((n_obj, N), np.inf)
    edge = np.full((n_obj, N), np.inf)
    mesh_tol = {}
    for i in range(n_obj):
        d4 = ray4 @ ctx["L"][i].T
        o4 = np.broadcast_to(ctx["sc"][i], d4.shape)
        s, f, nr, eg = _shape(ctx, i, o4, d4, grow)
        if not grow and int(ctx["types"][i]) == MESH:
            mesh_tol[i] = _mesh_tol(ctx)
            ctx.setdefault("mesh_hits", {})[i] = ctx["last_bf"]
        with np.errstate(invalid="ignore"):
            te = o4[:, 0] + np.where(np.isfinite(s), s, 0.0) * d4[:, 0]
        scale = np.abs(o4[:, 0]) + np.where(np.isfinite(s), s, 0.0) * np.abs(ctx["L"][i][0]).sum()
        wd = np.where(np.isfinite(s), _window_dist(ctx["windows"], i, te, scale), np.inf)
        ok = _window_in(ctx["windows"], i, te)
        S[i], F[i], near[i], wdist[i], raw[i], edge[i] = np.where(ok, s, np.inf), f, nr, wd, s, eg
    return S, F, near, wdist, raw, edge, mesh_tol


def _attributes(ctx, i, o4, d4, s, face):
    """(event, uv, normal in the rest frame, |cos|, J of the uv) of hits of object i (a sphere or a cube) at parameter s."""
    obj = ctx["objs"][i]
    A = obj["InvM"].astype(np.float64)[:3, :3]
    o3, d3 = _object_ray(obj, o4, d4)
    p = o3 + s[:, None] * d3
    event = o4 + s[:, None] * d4
    if int(ctx["types"][i]) == SPHERE:
        g = p
        y = np.clip(p[:, 1], -1.0, 1.0)
        uv = np.stack([0.5 + np.arctan2(p[:, 2], p[:, 0]) / (2 * np.pi), np.arcsin(y) / np.pi + 0.5], axis=1)
        rho = np.sqrt(np.maximum(p[:, 0] ** 2 + p[:, 2] ** 2, 1e-300))
        J = 1.0 / (np.pi * rho)
    else:
        rows = np.arange(len(p))
        g = np.zeros_like(p)
        ax = np.maximum(face, 0)
        g[rows, ax] = -np.sign(d3[rows, ax])
        first = np.where(ax == 0, 1, 0)
        second = np.where(ax == 2, 1, 2)
        uv = np.stack([(p[rows, first] + 1.0) / 2.0, (p[rows, second] + 1.0) / 2.0], axis=1)
        J = np.full(len(p), 0.5)
    nrm = g @ A                                                   # InvM3^T g, row-wise
    with np.errstate(invalid="ignore", divide="ignore"):
        nrm = nrm / np.linalg.norm(nrm, axis=1, keepdims=True)
        dn = d4[:, 1:] / np.linalg.norm(d4[:, 1:], axis=1, keepdims=True)
        cos = np.abs(np.einsum("ij,ij->i", nrm, dn))
    return event, uv, nrm, cos, J, np.linalg.norm(o3, axis=1), np.linalg.norm(d3, axis=1)


def hable(x):
    A, B, C, D, E, F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
    x = np.asarray(x, dtype=np.float64)
    return (x * (A * x + C * B) + D * E) / (x * (A * x + B) + D * F) - E / F


def weight(cos, r_hit_frame, r_light_frame):
    """cos(theta) / (1 + 0.1 r + 0.01 r^2), r the spatial length of the hit -> emission displacement in the HIT object's rest frame
    (its length in the lamp's frame is handed over too, and not used)."""
    return cos / (1.0 + 0.1 * r_hit_frame + 0.01 * r_hit_frame ** 2)


def tonemap(colour, white_point):
    return np.minimum(hable(colour) / hable(np.asarray(white_point, dtype=np.float64)), 1.0)


# ---- the texture fetch ---------------------------------------------------------------------------------------------------------------

def texel_coords(u, v, W, H):
    """Texel coordinates of (u, v) in a W x H image: (W u, H (1 - v)) — row 0 is v = 1, and there is no half-texel offset."""
    return W * u, H * (1.0 - v)


def texels(pool, index, W, x, y):
    """RGB / 255 of the texels (x, y) (integer arrays) of the W-wide image whose first byte is byte `index` of the pool: (n, 3).  (An
    address outside the pool is clamped into it, which only keeps numpy quiet: it happens on no pixel inside the rules.)"""
    addr = np.asarray(index + 3 * (W * y + x), dtype=np.int64)
    return pool[np.clip(addr[..., None] + np.arange(3), 0, len(pool) - 1)].astype(np.float64) / 255.0


def sample_texture(pool, index, W, H, uv):
    """The bilinear sample at uv (n, 2) and what its bound needs: (colour (n, 3), Gx (n, 3), Gy (n, 3), x0, y0, U, V) — Gx / Gy the
    largest differences between horizontally / vertically adjacent texels of the 3 x 3 neighbourhood of (x0, y0), per channel."""
    Uc, Vc = texel_coords(uv[:, 0], uv[:, 1], W, H)
    x0 = np.clip(np.floor(Uc), 0, W - 1).astype(np.int64)
    y0 = np.clip(np.floor(Vc), 0, H - 1).astype(np.int64)
    a, b = (Uc - x0)[:, None], (Vc - y0)[:, None]
    x1, y1 = np.minimum(x0 + 1, W - 1), np.minimum(y0 + 1, H - 1)
    xl = np.maximum(x1 - 1, 0)                                    # "Exception, the reference's": x0, but W - 2 in the last column
    t = lambda x, y: texels(pool, index, W, x, y)                 # noqa: E731
    colour = (1.0 - b) * ((1.0 - a) * t(x0, y0) + a * t(x1, y0)) + b * ((1.0 - a) * t(xl, y1) + a * t(x1, y1))
    xs = np.clip(x0[:, None] + np.arange(-1, 2), 0, W - 1)
    ys = np.clip(y0[:, None] + np.arange(-1, 2), 0, H - 1)
    block = texels(pool, index, W, xs[:, None, :], ys[:, :, None])                 # (n, 3 rows, 3 columns, 3 channels)
    Gx = np.abs(np.diff(block, axis=2)).max(axis=(1, 2))
    Gy = np.abs(np.diff(block, axis=1)).max(axis=(1, 2))
    return colour, Gx, Gy, x0, y0, Uc, Vc


def frame(objs, dirs, interval, ambient=0.0, white_point=(1.0, 1.0, 1.0), windows=None, mesh_arrays=None, colour=True, textures=None):
    """The model's frame for per-pixel directions `dirs` (N, 3; float32 values, not necessarily unit).  Returns a dict of (N, ...) arrays:
      object (-1: miss), dist, event (4), uv (2), normal (3), face;  tol_dist, tol_event (4), tol_uv (2);
      well_rec, well_col, candidates (n_obj + 1, N) bool — which objects (last row: a miss) a float program may name where ~well_rec;
      tol_normal (mesh hits; 0 elsewhere), mesh_well (mesh_truth's own filter; True off meshes), face_side (-1 / +1: which cube face of the axis);
      rgb (3) after the tonemap, rgb_extra (3): the derived texture and normal terms through the tonemap, absolute, on top of the
      measured constant; texel (x0, y0) and clamped_tap (x0 = W - 1 or y0 = H - 1) of textured hits; lit (n_obj, N) bool per light, shadowed (n_obj, N) per light,
      shadow_by (n_obj, N): pixels some light of which occluder i blocks, self_shadow, flashing, windowed_out (a nearer candidate fell
      outside its window), inside (the hit is a far wall seen from inside), `figures`, the conditioning figures by name, and `why`, the
      verdicts drawn from them by name (True: the pixel is ill-conditioned for that reason)."""
    ctx = context(objs, windows, mesh_arrays, textures)
    objs = ctx["objs"]
    n_obj = len(objs)
    dirs = np.asarray(dirs, dtype=np.float64).reshape(-1, 3)
    N = len(dirs)
    nrm_dir = dirs / np.linalg.norm(dirs, axis=1, keepdims=True)
    ray4 = np.hstack([np.full((N, 1), float(interval)), nrm_dir])
    runs = {g: _first_hit(ctx, ray4, g) for g in (0, +1, -1)}
    S, F, near, wdist, _, edge_fig, mesh_tol = runs[0]
    win = np.argmin(S, axis=0)
    cols = np.arange(N)
    s = S[win, cols]
    hit = np.isfinite(s)
    obj_idx = np.where(hit, win, -1)
    out = {"object": obj_idx, "dist": np.where(hit, s, 0.0), "event": np.zeros((N, 4)), "uv": np.zeros((N, 2)), "normal": np.zeros((N, 3)),
           "face": np.where(hit, F[win, cols], -1), "tol_dist": np.full(N, np.nan), "tol_event": np.full((N, 4), np.nan), "tol_uv": np.full((N, 2), np.nan)}
    # the conditioning of the record
    S2 = S.copy()
    S2[win, cols] = np.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        gap = np.where(hit, (S2.min(axis=0) - s) / np.maximum(s, 1e-300), np.inf)
    same = np.ones(N, dtype=bool)
    cand = np.zeros((n_obj + 1, N), dtype=bool)
    cand[np.where(hit, win, n_obj), cols] = True
    s_pm = {}
    for g in (+1, -1):
        Sg, Fg = runs[g][0], runs[g][1]
        wg = np.argmin(Sg, axis=0)
        hg = np.isfinite(Sg[wg, cols])
        same &= (hg == hit) & (~hit | ((wg == win) & (Fg[wg, cols] == F[win, cols])))
        cand[np.where(hg, wg, n_obj), cols] = True
        s_pm[g] = Sg[win, cols]
        # every object that comes within MIN_GAP of the front in this run may be named
        front = Sg.min(axis=0)
        with np.errstate(invalid="ignore"):
            cand[:n_obj] |= np.isfinite(Sg) & (Sg <= front * (1.0 + 2 * MIN_GAP))
    # a window's end, an origin at a surface, a ray within the slack of a cube's edge (the strict in-face tests leave the edge itself to
    # neither face: "Exception, the reference's"): that object's verdict may go either way, so the float program may name it, anything
    # else the ray meets, or nothing
    faces_differ = np.zeros(N, dtype=bool)
    for g in (+1, -1):
        wg = np.argmin(runs[g][0], axis=0)
        faces_differ |= hit & np.isfinite(runs[g][0][wg, cols]) & (wg == win) & (runs[g][1][wg, cols] != F[win, cols])
    on_edge = hit & ((edge_fig[win, cols] <= EDGE_MARGIN) | faces_differ)
    edge_obj = (wdist <= TIME_MARGIN) | (near <= ORIGIN_MARGIN)
    edge_obj[win, cols] |= on_edge
    edge = edge_obj.any(axis=0)
    cand[:n_obj] |= edge[None, :] & (np.isfinite(runs[0][4]) | np.isfinite(runs[+1][4]))
    cand[n_obj] |= edge
    figures = {"gap": gap, "same_grown_shrunk": same, "origin_near": near.min(axis=0), "window_dist": wdist.min(axis=0),
               "cube_edge": np.where(hit, edge_fig[win, cols], np.inf)}
    cosv = np.full(N, np.nan)
    out["tol_normal"] = np.zeros(N)
    out["face_side"] = np.zeros(N, dtype=np.int64)
    mesh_well = np.ones(N, dtype=bool)
    inside = np.zeros(N, dtype=bool)
    flashing = np.zeros(N, dtype=bool)
    flash_dist = np.full(N, np.inf)
    for i in range(n_obj):
        idx = np.flatnonzero(obj_idx == i)
        if not idx.size:
            continue
        d4 = ray4[idx] @ ctx["L"][i].T
        o4 = np.broadcast_to(ctx["sc"][i], d4.shape)
        kind = int(ctx["types"][i])
        si = s[idx]
        out["event"][idx] = o4 + si[:, None] * d4
        with np.errstate(invalid="ignore"):
            tol_s = np.maximum(np.abs(s_pm[+1][idx] - si), np.abs(s_pm[-1][idx] - si)) + ROUNDINGS * U * si
            if kind == MESH:
                tol_s = mesh_tol[i][idx] + ROUNDINGS * U * si
        tol_s = np.where(np.isfinite(tol_s), tol_s, np.inf)
        out["tol_dist"][idx] = tol_s
        Lrow = np.abs(ctx["L"][i]).sum(axis=1)
        with np.errstate(invalid="ignore"):
            tol_e = np.abs(d4) * tol_s[:, None] + ROUNDINGS * U * (np.abs(o4) + si[:, None] * Lrow[None, :])
        out["tol_event"][idx] = np.where(np.isnan(tol_e), np.inf, tol_e)
        period, duration = float(objs[i]["flashPeriod"]), float(objs[i]["flashDuration"])
        if period > 0:
            e0 = out["event"][idx, 0]
            phase = e0 - period * np.floor(e0 / period)
            flashing[idx] = phase < duration
            scale = np.maximum(1.0, np.abs(e0) / period)          # the float phase loses the bits of e0 / period
            flash_dist[idx] = np.minimum(np.minimum(np.abs(phase - duration), phase), period - phase) / period / scale
        if kind == MESH:
            cosv[idx] = 1.0
            _, bf, tris, o3, d3 = ctx["mesh_hits"][i]
            ids = ctx["mesh"](i)[0]
            sub = {k: v[idx] for k, v in bf.items()}
            dlen = np.linalg.norm(d3[idx], axis=1)
            rays = np.hstack([o3[idx], d3[idx]])
            extra = ctx["budget"][i] / dlen * (np.linalg.norm(o3[idx], axis=1) + si * dlen)
            wlen = np.linalg.norm(d4[:, 1:], axis=1)
            _, nrm, uv = mesh_truth.hit_attributes(ctx["arrays"], i, rays, ids, sub, world_dirlen=wlen)
            _, tol_n, tol_t = mesh_truth.hit_tolerances(ctx["arrays"], i, rays, ids, tris, sub, extra_dq=extra, world_dirlen=wlen)
            out["normal"][idx], out["uv"][idx] = nrm, uv
            out["tol_normal"][idx] = np.where(np.isfinite(tol_n), tol_n, np.inf)
            out["tol_uv"][idx] = np.where(np.isfinite(tol_t), tol_t, np.inf)[:, None]
            lo, hi = mesh_truth.root_box(ctx["arrays"], i)
            sub["t_edge"] = sub["t_edge"] * dlen                   # (brute_force's t is the ray's parameter; the floor is a length)
            mesh_well[idx] = mesh_truth.well_conditioned(sub, 1e-3 * float(np.linalg.norm(hi - lo)))
            continue
        event, uv, nrm, cos, J, olen, dlen = _attributes(ctx, i, o4, d4, si, out["face"][idx])
        out["uv"][idx], out["normal"][idx], cosv[idx] = uv, nrm, cos
        o3 = _object_ray(objs[i], o4, d4)[0]
        inside[idx] = (np.linalg.norm(o3, axis=1) < 1.0) if kind == SPHERE else (np.abs(o3) < 1.0).all(axis=1)
        if kind == CUBE:                                           # which of the two faces on that axis: the sign of the hit point's coordinate
            ax = np.maximum(out["face"][idx], 0)
            d3 = _object_ray(objs[i], o4, d4)[1]
            out["face_side"][idx] = np.sign((o3 + si[:, None] * d3)[np.arange(len(idx)), ax]).astype(np.int64)
        spread = np.zeros_like(uv)
        ok = np.isfinite(s_pm[+1][idx]) & np.isfinite(s_pm[-1][idx])
        if ok.any():
            up = _attributes(ctx, i, o4[ok], d4[ok], s_pm[+1][idx][ok], out["face"][idx][ok])[1]
            um = _attributes(ctx, i, o4[ok], d4[ok], s_pm[-1][idx][ok], out["face"][idx][ok])[1]
            dd = np.abs(up - um)
            if kind == SPHERE:
                dd[:, 0] = np.minimum(dd[:, 0], 1.0 - dd[:, 0])
            spread[ok] = dd
        spread[~ok] = np.inf
        out["tol_uv"][idx] = spread + ((dlen * tol_s + ROUNDINGS * U * (1.0 + olen + si * dlen)) * J)[:, None] + ROUNDINGS * U
    figures["cos"] = cosv
    figures["flash_dist"] = flash_dist
    with np.errstate(invalid="ignore"):
        well = same & (gap > MIN_GAP) & (~hit | (cosv >= MIN_COS)) & ~edge
    # a hit whose bound is not finite (a mesh hit edge-on to its triangle, a grown or shrunk shape the ray no longer meets) is not held
    # to a bound at all: ill-conditioned, by name
    with np.errstate(invalid="ignore"):
        no_bound = hit & ~(np.isfinite(out["tol_dist"]) & np.isfinite(out["tol_event"]).all(axis=1))
    well = well & ~no_bound
    out["well_rec"] = well
    with np.errstate(invalid="ignore"):
        out["why"] = {"grown / shrunk disagree": ~same, "second object within MIN_GAP": ~(gap > MIN_GAP), "grazing hit": hit & ~(cosv >= MIN_COS),
                      "origin at a surface": (near <= ORIGIN_MARGIN).any(axis=0), "ray through a cube's edge": on_edge, "event time at a window's end": (wdist <= TIME_MARGIN).any(axis=0),
                      "no finite bound": no_bound}
    out["candidates"] = cand
    out["mesh_well"] = mesh_well
    out["why"]["mesh hit that mesh_truth calls ill-conditioned"] = ~mesh_well
    out["inside"] = inside & hit
    out["flashing"] = flashing
    out["windowed_out"] = np.zeros(N, dtype=bool)
    if ctx["windows"] is not None:
        bare = _first_hit(dict(ctx, windows=None), ray4, 0)[0]
        out["windowed_out"] = bare.min(axis=0) < np.where(hit, s, np.inf)
    out["figures"] = figures
    if colour:
        _shade(ctx, out, ray4, interval, ambient, white_point)
    return out


def _shade(ctx, out, ray4, interval, ambient, white_point):
    objs, n_obj, N = ctx["objs"], len(ctx["objs"]), len(ray4)
    obj_idx = out["object"]
    rgb_lin = np.tile(np.asarray(BACKGROUND, dtype=np.float64), (N, 1))
    well = out["well_rec"] & (out["figures"]["flash_dist"] > FLASH_MARGIN)
    why = out["why"]
    why["flash phase at its boundary"] = ~(out["figures"]["flash_dist"] > FLASH_MARGIN)
    for key in ("light near the horizon of the surface", "emission time at a window's end", "occluder verdict turns on the slack", "occluder crossing at the segment's end",
                "sphere u at the seam", "uv outside the unit square", "texture term without a finite bound", "last texel column's boundary"):
        why[key] = np.zeros(N, dtype=bool)
    lin_lo, lin_hi = rgb_lin.copy(), rgb_lin.copy()
    out["texel"] = np.full((N, 2), -1, dtype=np.int64)
    out["clamped_tap"] = np.zeros(N, dtype=bool)
    lit = np.zeros((n_obj, N), dtype=bool)
    shadowed = np.zeros((n_obj, N), dtype=bool)
    shadow_by = np.zeros((n_obj, N), dtype=bool)
    self_shadow = np.zeros(N, dtype=bool)
    light_cos = np.full(N, np.inf)
    null_res = 0.0
    lights = [l for l in range(n_obj) if objs[l]["light"]]
    for h in range(n_obj):
        idx = np.flatnonzero(obj_idx == h)
        if not idx.size:
            continue
        c = np.tile(objs[h]["color"].astype(np.float64)[:3], (len(idx), 1))
        dc = np.zeros_like(c)
        ok_px = np.ones(len(idx), dtype=bool)
        if int(objs[h]["textureIndex"]) != -1:
            Wt, Ht = int(objs[h]["textureWidth"]), int(objs[h]["textureHeight"])
            uv, tol = out["uv"][idx], out["tol_uv"][idx]
            c, Gx, Gy, x0, y0, Uc, Vc = sample_texture(ctx["textures"], int(objs[h]["textureIndex"]), Wt, Ht, uv)
            with np.errstate(invalid="ignore"):
                finite = (Wt * tol[:, 0] < 1.0) & (Ht * tol[:, 1] < 1.0)
                # in the last column the lower row blends columns W - 2 and W - 1 while the upper row is column W - 1 alone ("Exception,
                # the reference's"): down a column the sample changes by a vertical AND a horizontal difference
                in_last = (Wt >= 2) & (x0 == Wt - 1)
                dc = np.where(finite[:, None], Wt * tol[:, :1] * Gx + Ht * tol[:, 1:] * (Gy + np.where(in_last[:, None], Gx, 0.0)), 0.0) + ROUNDINGS * U
                outside = ~((uv >= 0.0) & (uv <= 1.0)).all(axis=1)
                seam = (int(ctx["types"][h]) == SPHERE) & (np.minimum(uv[:, 0], 1.0 - uv[:, 0]) <= tol[:, 0])
                row = np.rint(Vc)
                last = (Wt >= 2) & ((np.abs(Uc - (Wt - 1)) <= Wt * tol[:, 0]) | (in_last & (np.abs(Vc - row) <= Ht * tol[:, 1]) & (row >= 1) & (row <= Ht - 1)))
            why["uv outside the unit square"][idx], why["texture term without a finite bound"][idx] = outside, ~finite
            why["sphere u at the seam"][idx], why["last texel column's boundary"][idx] = seam, last
            ok_px &= finite & ~outside & ~seam & ~last
            out["texel"][idx] = np.stack([x0, y0], axis=1)
            out["clamped_tap"][idx] = (x0 == Wt - 1) | (y0 == Ht - 1)
        flash = np.where(out["flashing"][idx], 2.0, 1.0)[:, None]
        c, dc = c * flash, dc * flash
        c_lo, c_hi = np.maximum(c - dc, 0.0), c + dc
        is_light = 1.0 if objs[h]["light"] else 0.0
        if interval == 0:
            rgb_lin[idx], lin_lo[idx], lin_hi[idx] = c * (1.0 + is_light), c_lo * (1.0 + is_light), c_hi * (1.0 + is_light)
            well[idx] &= ok_px
            continue
        col = c * (float(ambient) + is_light)
        col_lo, col_hi = c_lo * (float(ambient) + is_light), c_hi * (float(ambient) + is_light)
        nrm = out["normal"][idx]
        tol_n = out["tol_normal"][idx]
        P = out["event"][idx] + np.hstack([np.zeros((len(idx), 1)), 0.001 * nrm])
        X = P @ ctx["IL"][h].T                                    # the start of the segment, camera frame
        for l in lights:
            if l == h:
                continue
            Y = X @ ctx["L"][l].T
            p_l = objs[l]["M"].astype(np.float64)[:3, 3]
            dv = p_l[None, :] - Y[:, 1:]
            rL = np.linalg.norm(dv, axis=1)
            D_L = np.hstack([(interval * rL)[:, None], dv])
            te = Y[:, 0] + interval * rL
            on = _window_in(ctx["windows"], l, te)
            wd = _window_dist(ctx["windows"], l, te, np.abs(Y[:, 0]) + rL)
            D_cam = D_L @ ctx["IL"][l].T
            D_h = D_cam @ ctx["L"][h].T
            r = np.linalg.norm(D_h[:, 1:], axis=1)
            res = np.abs(np.abs(D_h[:, 0]) - r) / np.maximum(r, 1e-300)
            bound = 64.0 * U * np.linalg.norm(ctx["L"][h], 2) * np.linalg.norm(ctx["IL"][l], 2) * np.linalg.norm(ctx["L"][l], 2) * np.linalg.norm(ctx["IL"][h], 2)
            if res.size and float(res.max()) > bound:
                raise NullConeError(f"object {h}, light {l}: the hit -> emission displacement is not null in the hit object's frame: "
                                    f"relative residual {float(res.max()):.3e} > {bound:.3e}")
            null_res = max(null_res, float(res.max()) if res.size else 0.0)
            cos = np.einsum("ij,ij->i", nrm, D_h[:, 1:]) / np.maximum(r, 1e-300)
            facing_sure = (np.abs(cos) >= MIN_COS_LIGHT) & (np.abs(cos) > tol_n)      # (tol_normal: 0 but for mesh hits)
            ok_px &= (wd > TIME_MARGIN) & facing_sure
            why["light near the horizon of the surface"][idx] |= ~facing_sure
            why["emission time at a window's end"][idx] |= ~(wd > TIME_MARGIN)
            light_cos[idx] = np.minimum(light_cos[idx], np.abs(cos))
            todo = np.flatnonzero(on & (cos > 0.0))
            if not todo.size:
                continue
            blocked = np.zeros(len(todo), dtype=bool)
            unsure = np.zeros(len(todo), dtype=bool)
            for i in range(n_obj):
                if i == l:
                    continue
                o4 = X[todo] @ ctx["L"][i].T
                d4 = D_cam[todo] @ ctx["L"][i].T
                verdicts = []
                for g in (0, +1, -1):
                    tau, _, _, eg = _shape(ctx, i, o4, d4, g, SHADOW_SLACK if g else 0.0)
                    with np.errstate(invalid="ignore"):
                        tc = o4[:, 0] + np.where(np.isfinite(tau), tau, 0.0) * d4[:, 0]
                    v = (tau < 1.0) & _window_in(ctx["windows"], i, tc)
                    verdicts.append(v)
                    if not g and int(ctx["types"][i]) == MESH:
                        # a mesh occluder's silhouette: mesh_truth's barycentric margin of the segment's line (its grow knows only the
                        # triangle test's own slack, not the float hit point the segment starts from)
                        graze = ctx["last_bf"][1]["margin"] <= mesh_truth.MARGIN
                        unsure |= graze
                        why["occluder verdict turns on the slack"][idx[todo]] |= graze
                    if g >= 0:
                        near_end = np.isfinite(tau) & ((np.abs(tau - 1.0) < END_MARGIN) | (tau < END_MARGIN) | ((tau < 1.0 + END_MARGIN) & (eg <= EDGE_MARGIN)))
                        near_win = np.isfinite(tau) & (tau < 1.0 + END_MARGIN) & \
                            (_window_dist(ctx["windows"], i, tc, np.abs(o4[:, 0]) + np.abs(d4[:, 0])) <= TIME_MARGIN)
                        unsure |= near_end | near_win
                        why["occluder crossing at the segment's end"][idx[todo]] |= near_end | near_win
                turns = (verdicts[1] != verdicts[2]) | (verdicts[0] != verdicts[1])
                why["occluder verdict turns on the slack"][idx[todo]] |= turns
                unsure |= turns
                blocked |= verdicts[0]
                shadow_by[i, idx[todo]] |= verdicts[0]
                if i == h:
                    self_shadow[idx[todo]] |= verdicts[0]
            ok_px[todo] &= ~unsure
            k = weight(cos[todo], r[todo], rL[todo])
            kc = np.where(blocked, 0.0, k)[:, None] * objs[l]["color"].astype(np.float64)[:3][None, :]
            with np.errstate(invalid="ignore", divide="ignore"):
                rho = np.where(tol_n[todo] > 0.0, tol_n[todo] / cos[todo], 0.0)[:, None]      # cos theta moves by tol_normal at the most
            col[todo] += c[todo] * kc
            col_lo[todo] += c_lo[todo] * kc * np.maximum(1.0 - rho, 0.0)
            col_hi[todo] += c_hi[todo] * kc * (1.0 + rho)
            lit[l, idx[todo]] = ~blocked
            shadowed[l, idx[todo]] = blocked
        rgb_lin[idx], lin_lo[idx], lin_hi[idx] = col, col_lo, col_hi
        well[idx] &= ok_px
    rgb = tonemap(rgb_lin, white_point)
    # the texture's and the normal's terms through the tonemap: Hable's curve is increasing for x >= 0, so [lo, hi] maps to an interval
    with np.errstate(invalid="ignore"):
        extra = np.maximum(tonemap(lin_hi, white_point) - rgb, rgb - tonemap(lin_lo, white_point))
    out["rgb_extra"] = np.where(np.isnan(extra), np.inf, np.maximum(extra, 0.0))
    with np.errstate(invalid="ignore"):
        raw = hable(rgb_lin) / hable(np.asarray(white_point, dtype=np.float64))
        at_clamp = (np.abs(raw - 1.0) < CLAMP_MARGIN).any(axis=1)
    out["rgb"] = rgb
    out["well_col"] = well & np.isfinite(rgb).all(axis=1) & (obj_idx >= 0) & out["mesh_well"] & np.isfinite(out["rgb_extra"]).all(axis=1)
    out["lit"], out["shadowed"], out["shadow_by"], out["self_shadow"] = lit, shadowed, shadow_by, self_shadow
    out["figures"]["light_cos"] = light_cos
    out["figures"]["at_clamp"] = at_clamp
    out["null_residual"] = null_res


def subset(model, mask):
    """The model's frame on the pixels of `mask` alone (a ray map's pixels that have a ray)."""
    mask = np.asarray(mask, dtype=bool).reshape(-1)
    N = len(mask)

    def cut(v):
        if isinstance(v, dict):
            return {k: cut(x) for k, x in v.items()}
        if isinstance(v, np.ndarray) and v.ndim >= 1 and v.shape[0] == N:
            return v[mask]
        if isinstance(v, np.ndarray) and v.ndim == 2 and v.shape[1] == N:
            return v[:, mask]
        return v
    return {k: cut(v) for k, v in model.items()}


# ---- the comparison ------------------------------------------------------------------------------------------------------------------

def compare_records(model, rec, objs):
    """Records `rec` (EVENT_DTYPE, any shape of N) of a float program against `model` (frame's dict).  Returns a dict:
      index_bad    well-conditioned pixels whose object index differs                                      [must be empty]
      attr_bad     well-conditioned hits whose dist, event or (u, v) is beyond its bound                   [must be empty]
      unexplained  ill-conditioned pixels whose object is none of the model's candidates                   [must be empty]
      ill_diff     ill-conditioned pixels whose object differs;  well_share: well-conditioned share of the model's hit pixels
      ratio_dist / ratio_event / ratio_uv: largest observed error / bound;  rel_dist: largest relative distance error (well hits)"""
    rec = np.asarray(rec).reshape(-1)
    N = len(rec)
    got = rec["object"].astype(np.int64)
    want = model["object"]
    well = model["well_rec"]
    n_obj = len(np.asarray(objs).reshape(-1))
    diff = got != want
    rows = np.where((got >= 0) & (got < n_obj), got, n_obj)
    allowed = model["candidates"][rows, np.arange(N)]
    both = well & (want >= 0) & ~diff
    types = object_types(np.asarray(objs).reshape(-1))
    is_sphere = np.zeros(N, dtype=bool)
    is_sphere[want >= 0] = types[want[want >= 0]] == SPHERE
    uv_held = model["mesh_well"]                 # a mesh hit's (u, v) is held to its bound where mesh_truth's own filter passes it
    e_d = np.abs(rec["dist"].astype(np.float64) - model["dist"])
    e_e = np.abs(rec["event"].astype(np.float64) - model["event"])
    e_uv = np.abs(rec["uv"].astype(np.float64) - model["uv"])
    e_uv[:, 0] = np.where(is_sphere, np.minimum(e_uv[:, 0], np.abs(1.0 - e_uv[:, 0])), e_uv[:, 0])
    with np.errstate(invalid="ignore", divide="ignore"):
        r_d = np.where(both, e_d / model["tol_dist"], 0.0)
        r_e = np.where(both[:, None], e_e / model["tol_event"], 0.0)
        # (an exact (u, v) under a bound of 0 — every corner of a vt-less mesh carries the one padded entry — is within it)
        r_uv = np.where((both & uv_held)[:, None] & (e_uv > 0.0), e_uv / model["tol_uv"], 0.0)
        rel = np.where(both, e_d / np.maximum(model["dist"], 1e-300), 0.0)
    r_d, r_e, r_uv = (np.where(np.isnan(x), np.inf, x) for x in (r_d, r_e, r_uv))
    attr_bad = both & ((r_d > 1.0) | (r_e > 1.0).any(axis=1) | (r_uv > 1.0).any(axis=1))
    hits = want >= 0
    return {"index_bad": np.flatnonzero(well & diff), "attr_bad": np.flatnonzero(attr_bad), "ill_diff": np.flatnonzero(~well & diff),
            "unexplained": np.flatnonzero(~well & diff & ~allowed), "well_share": float(well[hits].mean()) if hits.any() else 1.0,
            "hits": int(hits.sum()), "ratio_dist": float(r_d.max(initial=0.0)), "ratio_event": float(r_e.max(initial=0.0)),
            "ratio_uv": float(r_uv.max(initial=0.0)), "rel_dist": float(rel.max(initial=0.0))}


def compare_colours(model, rgb, floor=1e-3):
    """Tonemapped float RGB (N, 3 in any shape) against the model's: the largest error relative to max(model, floor) over the
    well-conditioned pixels (`rel`), its pixel, the well-conditioned share of the model's hit pixels that carry a colour, and the
    miss pixels' largest error (`miss`: a constant through the tonemap)."""
    rgb = np.asarray(rgb, dtype=np.float64).reshape(-1, 3)
    well = model["well_col"]
    with np.errstate(invalid="ignore"):
        # the per-pixel derived allowance (texture and normal terms, absolute, through the tonemap; 0 where neither applies) comes off
        # first: what is left is held to the one constant
        err = np.maximum(np.abs(rgb - model["rgb"]) - np.where(well[:, None], model["rgb_extra"], 0.0), 0.0) / np.maximum(model["rgb"], floor)
    e = np.where(well[:, None], err, 0.0).max(axis=1)
    coloured = (model["object"] >= 0) & np.isfinite(model["rgb"]).all(axis=1)
    miss = (model["object"] < 0) & model["well_rec"]
    return {"rel": float(e.max(initial=0.0)), "worst": int(np.argmax(e)) if e.size else -1, "median": float(np.median(e[well])) if well.any() else 0.0,
            "well_share": float(well[coloured].mean()) if coloured.any() else 1.0, "coloured": int(coloured.sum()),
            "miss": float(err[miss].max(initial=0.0)) if miss.any() else 0.0, "err": e}


# ---- the front end's matrices ----------------------------------------------------------------------------------------------------------

def boost(v):
    """The 4 x 4 Lorentz boost to the frame moving at velocity v (c = 1), rows and columns (t, x, y, z), float64."""
    v = np.asarray(v, dtype=np.float64)[:3]
    b2 = float(v @ v)
    B = np.eye(4)
    if b2 == 0.0:
        return B
    g = 1.0 / np.sqrt(1.0 - b2)
    B[0, 0] = g
    B[0, 1:] = B[1:, 0] = -g * v
    B[1:, 1:] += (g - 1.0) * np.outer(v, v) / b2
    return B
