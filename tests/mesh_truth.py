"""Float64 model of "intersect this ray with this mesh" and of "does this triangle lie in this box" — TEST INFRASTRUCTURE.

A helper, no tests in it.  Plain numpy, float64 throughout, written from the geometry: Moeller-Trumbore over EVERY triangle
of the mesh, no octree, no early exit, no epsilon.  It shares nothing with the walk (oracle/rpt_oracle.c, csrc/) but the
vertex data.  tests/test_mesh_ground_truth.py holds the oracle and the host octree builder against it,
tests/test_gpu_mesh_ground_truth.py the device.

Tolerances (`hit_tolerances`) — derived, not tuned
--------------------------------------------------
u = 2^-24.  The float triangle test is Cramer's rule in fp32; csrc/rpt_kernels.hip.h (comment of mesh_segment_apart, item (i);
DESIGN.md section 4) carries its error through the float operations: with tau = |o - A|, e1 = B - A, e2 = C - A, the float point
Q_f = o + g dist_f and the point T_f = A + u_f e1 + v_f e2 of the triangle's plane obey

    |Q_f - T_f|  <=  dQ  =  27.2 u tau |e1| |e2| / |det|  +  u (tau + 2.1 t + 2.1 max(|e1|, |e2|)),     det = g . (e1 x e2).

(The source then bounds |e1||e2| / |det| by K / 1e-7, which gives its `16.2 tau K`; here the ray's own determinant is known,
|det| = |e1 x e2| |cos|, so the bound is taken before that last step: 27.2 u tau / (sin(angle at A) |cos|).)
 * distance along the ray: Q_f is on the ray and within dQ of the plane, so |t_f - t| <= dt = dQ / |cos|;
 * reported distance |M Q| (rpt_oracle_octree_rays: zero world origin, unit direction length):
       |dist_f - dist| <= ||M3||_2 dt + 8u (||M3||_2 |Q| + |M.t|)      (transformPoint and length in float: a handful of roundings);
 * barycentrics: T_f lies within dQ + dt <= 2 dt of the exact hit point, and u, v change by one over an altitude of the
   triangle:  |u_f - u|, |v_f - v| <= Eb = 2 dt / h_min,  h_min = |e1 x e2| / (longest side);
 * interpolated normal n = normalize(InvM3^T (w nA + u nB + v nC)): the raw sum moves by at most Eb (2|nA| + |nB| + |nC|), and
   normalising after a linear map multiplies a relative error by at most 2 cond(InvM3):
       |n_f - n| <= 2 cond(InvM3) Eb (2|nA| + |nB| + |nC|) / |w nA + u nB + v nC| + 16u;
 * texture coordinates:  |uv_f - uv| <= Eb (2|uvA| + |uvB| + |uvC|) + 8u max|uv|.
These are worst-case bounds; the observed errors are far smaller (DESIGN.md section 3 puts both side by side).

Conditioning
------------
A float test cannot be held to the exact answer where the exact answer turns on the last bits.  `brute_force` returns the
figures that say so, per ray: the barycentric margin (distance, in barycentric units, of a plane hit from the nearest edge line
of its triangle, over every triangle that could decide the ray), |cos| between the ray and the hit triangle's normal, the relative
gap in t to the second-nearest hit, and `t_edge`: the smallest |t| of a plane hit that lies in or next to its triangle — the
`0 <= dist` edge of the test, which an origin IN a triangle's plane sits on (Models/cube.obj and Models/triangle.obj have
every triangle in a face of their root box).
"""
from __future__ import annotations

import numpy as np

U = 2.0 ** -24
MARGIN = 1e-3          # a plane hit nearer than this (barycentric) to an edge line of its triangle is ill-conditioned
MIN_COS = 0.05         # as is a hit at less than this |cos| to the triangle's normal
MIN_GAP = 1e-3         # and a second hit less than this (relative, in t) behind the first
PAIRS_PER_CHUNK = 3_000_000      # ray x triangle pairs per numpy chunk: 24 MB per float64 temporary


# ---- the scene's arrays ------------------------------------------------------------------------------------------------------------

def arrays(scene):
    """The scene as float64 / int arrays.  `scene` is a relativitypathtracer_amd.Scene, or a dict as this function returns it
    (so that a test can hand over a corrupted COPY)."""
    if isinstance(scene, dict):
        return scene
    from relativitypathtracer_amd.scene import OBJECT_DTYPE, OCTREE_DTYPE
    b = scene.buffers()
    return {
        "objects": b["objects"].view(OBJECT_DTYPE).copy(),
        "vertices": b["vertices"], "normals": b["normals"], "uvs": b["uvs"],
        "triangles": b["triangles"], "octrees": b["octrees"].view(OCTREE_DTYPE).copy(), "octreeTris": b["octreeTris"],
        "textures": b["textures"],
    }


def mesh_triangles(scene, object_index):
    """The triangle set mesh object `object_index` stands for: the de-duplicated list of its root node, vertices through
    triangles[9 t + 0 / 3 / 6].  (The root list is the definition: the reference lets a second mesh's root list the first mesh's
    triangles too.)  Returns (ids (T,), corners (T, 3, 3) float64)."""
    a = arrays(scene)
    root = a["octrees"][int(a["objects"][object_index]["meshIndex"])]
    lst = a["octreeTris"][int(root["trisIndex"]): int(root["trisIndex"]) + int(root["trisCount"])]
    ids = np.unique(lst).astype(np.int64)
    words = a["triangles"].astype(np.int64)
    v = a["vertices"][:, :3].astype(np.float64)
    corners = np.stack([v[words[9 * ids + 0]], v[words[9 * ids + 3]], v[words[9 * ids + 6]]], axis=1)
    return ids, corners


def root_box(scene, object_index):
    a = arrays(scene)
    root = a["octrees"][int(a["objects"][object_index]["meshIndex"])]
    return root["min"][:3].astype(np.float64), root["max"][:3].astype(np.float64)


# ---- brute force -------------------------------------------------------------------------------------------------------------------

def _pairs(rays, tris):
    """det, u, v, t of every (ray, triangle) pair, (R, T) each: Moeller-Trumbore written as scalar triple products so that each
    is a matrix product.  det = d . (e1 x e2) (sign: positive when the ray runs along the normal); degenerate triangles and
    rays in a triangle's plane give inf / nan, which every comparison below treats as "no"."""
    o, d = rays[:, :3], rays[:, 3:6]
    A, e1, e2 = tris[:, 0], tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    n = np.cross(e1, e2)
    m = np.cross(o, d)                                       # (R, 3)
    det = -(d @ n.T)                                         # e1 . (d x e2)
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (m @ e2.T - d @ np.cross(e2, A).T) / det
        v = (-(m @ e1.T) - d @ np.cross(A, e1).T) / det
        t = (o @ n.T - np.einsum("ij,ij->i", A, n)[None, :]) / det
    return det, u, v, t


def brute_force(rays, tris, chunk_pairs=PAIRS_PER_CHUNK, grow=None):
    """Nearest hit with t >= 0 of `rays` (n, 6: origin, direction; the direction need not be unit) over all `tris` (T, 3, 3).

    Returns a dict of (n,) arrays: hit, t, tri (index into tris, -1), u, v, and the conditioning figures margin, cos, gap, t_edge
    (module docstring).  `grow`: None for the exact test; +1 / -1 for the test with every triangle grown / shrunk by the float
    test's own slack (`_pair_slack`), the t >= 0 edge and, when shrinking, the determinant cut moved likewise."""
    rays = np.asarray(rays, dtype=np.float64)
    tris = np.asarray(tris, dtype=np.float64)
    n, T = len(rays), len(tris)
    out = {k: np.full(n, f, dtype=np.float64) for k, f in
           (("t", np.inf), ("u", np.nan), ("v", np.nan), ("margin", np.inf), ("cos", np.nan), ("gap", np.inf), ("t_edge", np.inf))}
    out["hit"] = np.zeros(n, dtype=bool)
    out["tri"] = np.full(n, -1, dtype=np.int64)
    e1, e2 = tris[:, 1] - tris[:, 0], tris[:, 2] - tris[:, 0]
    nrm = np.cross(e1, e2)
    nlen = np.linalg.norm(nrm, axis=1)
    step = max(1, chunk_pairs // max(T, 1))
    for r0 in range(0, n, step):
        rr = rays[r0:r0 + step]
        det, u, v, t = _pairs(rr, tris)
        with np.errstate(invalid="ignore"):
            w = 1.0 - u - v
            bary = np.minimum(np.minimum(u, v), w)
            if grow is None:
                inside = (bary >= 0.0) & (t >= 0.0)
            else:
                s_b, s_t, det_floor = _pair_slack(rr, tris, det, t)
                inside = (bary >= -grow * s_b) & (t >= -grow * s_t)
                if grow < 0:
                    inside &= np.abs(det) >= det_floor
        inside &= np.isfinite(t) & np.isfinite(bary)
        tt = np.where(inside, t, np.inf)
        k = np.argmin(tt, axis=1)
        rows = np.arange(len(rr))
        tn = tt[rows, k]
        hit = np.isfinite(tn)
        sl = slice(r0, r0 + len(rr))
        out["hit"][sl] = hit
        out["t"][sl] = tn
        out["tri"][sl] = np.where(hit, k, -1)
        out["u"][sl] = np.where(hit, u[rows, k], np.nan)
        out["v"][sl] = np.where(hit, v[rows, k], np.nan)
        dlen = np.linalg.norm(rr[:, 3:6], axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            out["cos"][sl] = np.where(hit, np.abs(det[rows, k]) / (nlen[k] * dlen), np.nan)
            # second-nearest hit, relative
            tt[rows, k] = np.inf
            t2 = tt.min(axis=1)
            out["gap"][sl] = np.where(hit & np.isfinite(t2), (t2 - tn) / np.maximum(np.abs(tn), 1e-300), np.inf)
            # barycentric margin over every triangle that could decide the ray
            front = np.isfinite(t) & np.isfinite(bary) & (t >= 0.0) & (t <= np.where(hit, 1.001 * tn, np.inf)[:, None])
            out["margin"][sl] = np.where(front, np.abs(bary), np.inf).min(axis=1)
            # the t = 0 edge: plane hits in or next to their triangle, either side of the origin
            near = np.isfinite(t) & np.isfinite(bary) & (bary > -MARGIN)
            out["t_edge"][sl] = np.where(near, np.abs(t), np.inf).min(axis=1)
    return out


def _pair_slack(rays, tris, det, t):
    """Per (ray, triangle) pair: the slack of the float triangle test in barycentric units (Eb of the module docstring), in t
    (dt), and the determinant below which the float test's `|det| < 1e-7` cut may strike (1e-7 plus the 6.8u |e1||e2| a float
    3-term dot of a cross product can be off by, for a unit direction)."""
    o, d = rays[:, :3], rays[:, 3:6]
    dlen = np.linalg.norm(d, axis=1)[:, None]
    A = tris[:, 0]
    e1, e2, e3 = tris[:, 1] - A, tris[:, 2] - A, tris[:, 2] - tris[:, 1]
    l1, l2, l3 = (np.linalg.norm(e, axis=1) for e in (e1, e2, e3))
    area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
    tau = np.linalg.norm(o[:, None, :] - A[None, :, :], axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        adet = np.abs(det) / dlen                                     # of the unit direction
        cos = adet / area2[None, :]
        dq = 27.2 * U * tau * (l1 * l2)[None, :] / adet + U * (tau + 2.1 * np.abs(t) * dlen + 2.1 * np.maximum(l1, l2)[None, :])
        dt = dq / cos
        h_min = area2 / np.maximum(np.maximum(l1, l2), l3)
        eb = 2.0 * dt / h_min[None, :]
    eb = np.where(np.isfinite(eb), eb, np.inf)
    dt = np.where(np.isfinite(dt), dt, np.inf) / dlen
    det_floor = (1e-7 + 6.8 * U * (l1 * l2)[None, :]) * dlen
    return eb, dt, det_floor


def well_conditioned(bf, t_floor):
    """The rays of a brute_force result on which a float test can be held to the exact answer: barycentric margin above MARGIN;
    for hits |cos| >= MIN_COS and no second hit within MIN_GAP (relative); and no plane hit in or next to its triangle at
    |t| <= t_floor (callers pass 1e-3 of the root box's diagonal: far above any dt, far below the spacing of random origins)."""
    ok = (bf["margin"] > MARGIN) & (bf["t_edge"] > t_floor)
    with np.errstate(invalid="ignore"):
        ok &= ~bf["hit"] | ((bf["cos"] >= MIN_COS) & (bf["gap"] > MIN_GAP))
    return ok


# ---- what the walk reports for a hit ---------------------------------------------------------------------------------------------------

def hit_attributes(scene, object_index, rays, ids, bf, world_origin=None, world_dirlen=None):
    """Float64 distance, normal and (u, v) as rpt_probe_walk / rpt_oracle_octree_rays report them, for the hits of `bf`:
    the normal interpolated from triangles[9 t + 2 / 5 / 8] through InvM transposed and normalised, (u, v) from
    triangles[9 t + 1 / 4 / 7], the distance as the length of M * hitpoint.  M and InvM are the object's float32 matrices taken
    as float64.  `world_origin` (n, 3) / `world_dirlen` (n,): the ray's origin and direction length in the object's rest frame, from
    which the 4-D entry points re-measure the distance (rpt_probe_object; default: zero and one).  Rows of misses are nan.  Returns (dist (n,), normal (n, 3), uv (n, 2))."""
    a = arrays(scene)
    obj = a["objects"][object_index]
    M, InvM = obj["M"].astype(np.float64), obj["InvM"].astype(np.float64)
    rays = np.asarray(rays, dtype=np.float64)
    hit = bf["hit"]
    k = ids[np.where(hit, bf["tri"], 0)]
    words = a["triangles"].astype(np.int64)
    nrm, uvs = a["normals"][:, :3].astype(np.float64), a["uvs"].astype(np.float64)
    u, v = bf["u"][:, None], bf["v"][:, None]
    w = 1.0 - u - v
    raw = w * nrm[words[9 * k + 2]] + u * nrm[words[9 * k + 5]] + v * nrm[words[9 * k + 8]]
    n = raw @ InvM[:3, :3]                                   # InvM3^T raw, row-wise
    with np.errstate(invalid="ignore", divide="ignore"):
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
    uv = w * uvs[words[9 * k + 1]] + u * uvs[words[9 * k + 4]] + v * uvs[words[9 * k + 7]]
    q = rays[:, :3] + rays[:, 3:6] * np.where(hit, bf["t"], np.nan)[:, None]
    wp = q @ M[:3, :3].T + M[:3, 3]
    dist = np.linalg.norm(wp if world_origin is None else wp - world_origin, axis=1) / (1.0 if world_dirlen is None else world_dirlen)
    n[~hit], uv[~hit] = np.nan, np.nan
    return dist, n, uv


def hit_tolerances(scene, object_index, rays, ids, tris, bf, extra_dq=0.0, world_dirlen=None):
    """The bounds of the module docstring for the hits of `bf`: (tol_dist (n,), tol_normal (n,), tol_uv (n,)); nan for misses.
    `extra_dq`: how far the float walk's object-space ray may lie from `rays` at the hit point (callers that map rays with InvM
    themselves); it joins dQ.  `world_dirlen` scales the distance bound as it scales the distance."""
    a = arrays(scene)
    obj = a["objects"][object_index]
    M, InvM = obj["M"].astype(np.float64), obj["InvM"].astype(np.float64)
    rays = np.asarray(rays, dtype=np.float64)
    hit = bf["hit"]
    j = np.where(hit, bf["tri"], 0)
    k = ids[j]
    o, d = rays[:, :3], rays[:, 3:6]
    dlen = np.linalg.norm(d, axis=1)
    A = tris[j, 0]
    e1, e2, e3 = tris[j, 1] - A, tris[j, 2] - A, tris[j, 2] - tris[j, 1]
    l1, l2, l3 = (np.linalg.norm(e, axis=1) for e in (e1, e2, e3))
    area2 = np.linalg.norm(np.cross(e1, e2), axis=1)
    tau = np.linalg.norm(o - A, axis=1)
    t_len = np.where(hit, bf["t"], 0.0) * dlen
    with np.errstate(invalid="ignore", divide="ignore"):
        cos = bf["cos"]
        dq = 27.2 * U * tau * l1 * l2 / (area2 * cos) + U * (tau + 2.1 * t_len + 2.1 * np.maximum(l1, l2)) + extra_dq
        dt = dq / cos
        eb = 2.0 * dt * np.maximum(np.maximum(l1, l2), l3) / area2
    q = o + d * np.where(hit, bf["t"], 0.0)[:, None]
    m_norm = np.linalg.norm(M[:3, :3], 2)
    tol_dist = (m_norm * dt + 8 * U * (m_norm * np.linalg.norm(q, axis=1) + np.linalg.norm(M[:3, 3]))) / (1.0 if world_dirlen is None else world_dirlen)
    words = a["triangles"].astype(np.int64)
    nrm, uvs = a["normals"][:, :3].astype(np.float64), a["uvs"].astype(np.float64)
    nA, nB, nC = nrm[words[9 * k + 2]], nrm[words[9 * k + 5]], nrm[words[9 * k + 8]]
    u, v = np.where(hit, bf["u"], 0.0)[:, None], np.where(hit, bf["v"], 0.0)[:, None]
    raw = (1.0 - u - v) * nA + u * nB + v * nC
    ln = lambda x: np.linalg.norm(x, axis=1)                 # noqa: E731
    with np.errstate(invalid="ignore", divide="ignore"):
        tol_n = 2.0 * np.linalg.cond(InvM[:3, :3]) * eb * (2 * ln(nA) + ln(nB) + ln(nC)) / ln(raw) + 16 * U
    tA, tB, tC = uvs[words[9 * k + 1]], uvs[words[9 * k + 4]], uvs[words[9 * k + 7]]
    tol_uv = eb * (2 * ln(tA) + ln(tB) + ln(tC)) + 8 * U * np.maximum(np.maximum(ln(tA), ln(tB)), ln(tC))
    for x in (tol_dist, tol_n, tol_uv):
        x[~hit] = np.nan
    return tol_dist, tol_n, tol_uv


def compare_walk(scene, object_index, rays, got, t_floor=None, bf=None, world_origin=None, world_dirlen=None, extra_dq=0.0):
    """`got` (n, 8) = {hit, dist, normal.xyz, uv.xy, 0} of a walk (oracle or device) on object-space `rays` (n, 6) against the
    brute force.  Returns a dict:
      well          (n,) bool: the well-conditioned rays
      flag_bad      indices of well-conditioned rays whose hit flag differs from the brute force's        [must be empty]
      attr_bad      indices of well-conditioned hits whose distance, normal or (u, v) is beyond its bound [must be empty]
      ill_flag      indices of ill-conditioned rays whose hit flag differs
      ill_unexplained   those of ill_flag that the grown and the shrunk brute force do NOT answer differently [must be empty]
      err_dist / err_normal / err_uv, tol_dist / tol_normal / tol_uv   (n,) observed errors and bounds (nan off the well hits)
      bf            the brute force's result"""
    rays = np.asarray(rays, dtype=np.float64)
    got = np.asarray(got, dtype=np.float64)
    ids, tris = mesh_triangles(scene, object_index)
    lo, hi = root_box(scene, object_index)
    if t_floor is None:
        t_floor = 1e-3 * float(np.linalg.norm(hi - lo))
    if bf is None:
        bf = brute_force(rays, tris)
    well = well_conditioned(bf, t_floor)
    got_hit = got[:, 0] != 0.0
    flag_diff = got_hit != bf["hit"]
    dist, nrm, uv = hit_attributes(scene, object_index, rays, ids, bf, world_origin, world_dirlen)
    tol_d, tol_n, tol_uv = hit_tolerances(scene, object_index, rays, ids, tris, bf, extra_dq, world_dirlen)
    both = well & bf["hit"] & got_hit
    with np.errstate(invalid="ignore"):
        err_d = np.where(both, np.abs(got[:, 1] - dist), np.nan)
        err_n = np.where(both, np.linalg.norm(got[:, 2:5] - nrm, axis=1), np.nan)
        err_uv = np.where(both, np.linalg.norm(got[:, 5:7] - uv, axis=1), np.nan)
        attr_bad = both & ~((err_d <= tol_d) & (err_n <= tol_n) & (err_uv <= tol_uv))
    ill_flag = np.flatnonzero(~well & flag_diff)
    unexplained = []
    if ill_flag.size:
        grown = brute_force(rays[ill_flag], tris, grow=+1)["hit"]
        shrunk = brute_force(rays[ill_flag], tris, grow=-1)["hit"]
        unexplained = ill_flag[~(grown & ~shrunk)]
    return {
        "well": well, "flag_bad": np.flatnonzero(well & flag_diff), "attr_bad": np.flatnonzero(attr_bad),
        "ill_flag": ill_flag, "ill_unexplained": np.asarray(unexplained, dtype=np.int64),
        "err_dist": err_d, "err_normal": err_n, "err_uv": err_uv, "tol_dist": tol_d, "tol_normal": tol_n, "tol_uv": tol_uv,
        "dist": dist, "bf": bf, "err_dist_any": np.where(bf["hit"] & got_hit, np.abs(got[:, 1] - dist), np.nan),
    }


# ---- ray families ------------------------------------------------------------------------------------------------------------------

FAMILIES = ("outside->box", "inside", "->triangle interior", "->vertex/edge", "axis-parallel", "on the box", "from 50 diagonals")
ILL_FAMILY = 3            # the vertex / edge-midpoint family: ill-conditioned by construction, kept to a sixth of the rays


def ray_families(lo, hi, tris, rng, per_family, origins_off_the_box=0.0):
    """Object-space rays (float32 values, returned as float32 (n, 6)) and their family index (n,), for a mesh with root box
    [lo, hi] and corners `tris`: FAMILIES, `per_family` rays each, the vertex / edge family included (one of seven: under a sixth).

    A flat root box (Models/triangle.obj) gets a thickness of 1 % of its diagonal for DRAWING points, and
    `origins_off_the_box` (a fraction of the diagonal) moves the "inside" and "on the box" origins onto a box grown by that much:
    for meshes whose triangles lie IN the faces of their root box (cube.obj, triangle.obj) an origin on the box is an origin in a
    triangle's plane, which no float test can be held to."""
    lo, hi = np.asarray(lo, dtype=np.float64), np.asarray(hi, dtype=np.float64)
    diag = float(np.linalg.norm(hi - lo))
    flat = (hi - lo) < 1e-2 * diag
    dlo, dhi = np.where(flat, lo - 5e-3 * diag, lo), np.where(flat, hi + 5e-3 * diag, hi)
    c = 0.5 * (lo + hi)
    k = per_family
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)      # noqa: E731
    shell = lambda r0, r1: c + unit(rng.normal(size=(k, 3))) * rng.uniform(r0, r1, size=(k, 1)) * diag     # noqa: E731
    T = len(tris)
    fam = []
    # 0: from outside towards uniformly drawn points of the root box
    o = shell(1.5, 6.0)
    fam.append(np.hstack([o, unit(rng.uniform(dlo, dhi, size=(k, 3)) - o)]))
    # 1: from inside the box, any direction
    g = origins_off_the_box * diag
    fam.append(np.hstack([rng.uniform(dlo - g, dhi + g, size=(k, 3)), unit(rng.normal(size=(k, 3)))]))
    # 2: from outside towards a uniformly drawn interior point of a uniformly drawn triangle (must hit; not edge-on: the origin is
    #    drawn again until the ray makes |cos| >= 0.1 with the triangle's normal — grazing directions are family-0 business)
    tri = tris[rng.integers(0, T, size=k)]
    r1, r2 = np.sqrt(rng.random((k, 1))), rng.random((k, 1))
    p = (1 - r1) * tri[:, 0] + r1 * (1 - r2) * tri[:, 1] + r1 * r2 * tri[:, 2]
    nt = np.cross(tri[:, 1] - tri[:, 0], tri[:, 2] - tri[:, 0])
    nt = nt / np.maximum(np.linalg.norm(nt, axis=1, keepdims=True), 1e-300)
    o = shell(2.0, 4.0)
    for _ in range(8):
        again = np.abs(np.einsum("ij,ij->i", unit(p - o), nt)) < 0.1
        o = np.where(again[:, None], shell(2.0, 4.0), o)
    fam.append(np.hstack([o, unit(p - o)]))
    # 3: towards vertices and edge midpoints
    tri = tris[rng.integers(0, T, size=k)]
    a, b = rng.integers(0, 3, size=k), rng.integers(0, 3, size=k)
    p = 0.5 * (tri[np.arange(k), a] + tri[np.arange(k), b])             # a == b: the vertex itself
    o = shell(2.0, 4.0)
    fam.append(np.hstack([o, unit(p - o)]))
    # 4: axis-parallel, one and two zero components
    d = np.zeros((k, 3))
    ax = rng.integers(0, 3, size=k)
    d[np.arange(k), ax] = rng.choice([-1.0, 1.0], size=k)
    two = rng.random(k) < 0.5
    d[two, (ax[two] + 1) % 3] = rng.normal(size=int(two.sum()))
    ext = np.maximum(dhi - dlo, 1e-2 * diag)
    o = rng.uniform(dlo, dhi, size=(k, 3))
    o[np.arange(k), ax] = (c - d * 2.0 * ext)[np.arange(k), ax]          # outside, looking in along the axis
    fam.append(np.hstack([o, unit(d)]))
    # 5: origins on faces, edges and corners of the root box
    o = rng.uniform(lo, hi, size=(k, 3))
    snap = rng.random((k, 3)) < 0.4
    snap[np.arange(k), rng.integers(0, 3, size=k)] = True
    snap[:, flat] = True                                                 # (a flat box: always off its plane, or every ray would graze)
    side = rng.random((k, 3)) < 0.5
    o = np.where(snap, np.where(side, lo - g, hi + g), o)
    fam.append(np.hstack([o, unit(c + rng.uniform(-0.5, 0.5, size=(k, 3)) * (dhi - dlo) - o)]))
    # 6: long rays from 50 box diagonals away
    #    (aimed at the box grown by half its extent on every side, so that a mesh that fills its box — cube.obj — is missed too)
    o = shell(50.0, 50.0)
    fam.append(np.hstack([o, unit(rng.uniform(dlo - 0.5 * (dhi - dlo), dhi + 0.5 * (dhi - dlo), size=(k, 3)) - o)]))
    rays = np.vstack(fam).astype(np.float32)
    return rays, np.repeat(np.arange(len(fam)), k)


# ---- triangle against box ----------------------------------------------------------------------------------------------------------

def triangle_box_separation(tri, lo, hi):
    """Signed separation of triangles `tri` (N, 3, 3) from boxes [lo, hi] ((N, 3) each or broadcastable) by the separating-axis
    theorem in float64: over the 13 axes (3 box normals, the triangle's normal, 9 edge x box-axis products, each normalised; zero
    axes skipped) the largest gap between the two projections.  > 0: disjoint, that far apart along some axis; < 0: they overlap,
    and no single axis translation shorter than that separates them."""
    tri = np.asarray(tri, dtype=np.float64)
    lo, hi = np.broadcast_to(np.asarray(lo, dtype=np.float64), tri[:, 0].shape), np.broadcast_to(np.asarray(hi, dtype=np.float64), tri[:, 0].shape)
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    p = tri - c[:, None, :]
    e = np.stack([p[:, 1] - p[:, 0], p[:, 2] - p[:, 1], p[:, 0] - p[:, 2]], axis=1)
    eye = np.eye(3)
    axes = [np.broadcast_to(eye[i], c.shape) for i in range(3)]
    axes.append(np.cross(e[:, 0], e[:, 1]))
    for i in range(3):
        for j in range(3):
            axes.append(np.cross(e[:, i], np.broadcast_to(eye[j], c.shape)))
    sep = np.full(len(tri), -np.inf)
    for ax in axes:
        ln = np.linalg.norm(ax, axis=1)
        ok = ln > 0
        a = ax / np.where(ok, ln, 1.0)[:, None]
        proj = np.einsum("nkj,nj->nk", p, a)
        r = np.einsum("nj,nj->n", h, np.abs(a))
        gap = np.maximum(proj.min(axis=1) - r, -r - proj.max(axis=1))
        sep = np.where(ok, np.maximum(sep, gap), sep)
    return sep


def triangle_overlaps_box(tri, lo, hi, slack=0.0):
    """True where triangle and box overlap by more than `slack` (slack > 0), or come within |slack| of each other (slack < 0:
    so `~triangle_overlaps_box(..., slack=-s)` is "clear by more than s")."""
    return triangle_box_separation(tri, lo, hi) < -slack


# ---- octree against geometry -------------------------------------------------------------------------------------------------------

def mesh_nodes(scene, root_index):
    """Indices of the nodes of the octree rooted at `root_index` (breadth first) and their depth."""
    oc = arrays(scene)["octrees"]
    order, depth, level, dcur = [], [], [root_index], 0
    while level:
        order += level
        depth += [dcur] * len(level)
        nxt = []
        for i in level:
            ch = oc[i]["children"]
            if ch[0] != -1:
                nxt += [int(x) for x in ch]
        level, dcur = nxt, dcur + 1
    return np.array(order), np.array(depth)


def check_octree(scene, root_index, slack):
    """The octree rooted at node `root_index` against the geometry.  Returns a dict of violation lists (all must be empty):
      incomplete  (leaf, triangle): overlaps the leaf's box by more than `slack` and is missing from its list
      unsound     (leaf, triangle): listed, and clear of the leaf's box by more than `slack`
      tiling      inner nodes whose eight children do not tile them float for float (see the code: the far faces by the reference's rule)
      far_face_drift   (node, ulp): inner nodes whose far faces miss the parent's by rounding — the reference's property, bounded by the caller
      links       (node, side): the neighbour link is not the cell beyond that face (see below)
    Links (side ids 0/1 = -z/+z, 2/3 = -x/+x, 4/5 = -y/+y): -1 exactly where the node's face lies on the root box's boundary;
    otherwise the linked box is at least as large as the node and contains the centre of the node's face pushed outward by half
    the node's extent."""
    a = arrays(scene)
    oc = a["octrees"]
    nodes, _ = mesh_nodes(a, root_index)
    root = oc[root_index]
    lst = a["octreeTris"]
    root_ids = np.unique(lst[int(root["trisIndex"]): int(root["trisIndex"]) + int(root["trisCount"])]).astype(np.int64)
    words = a["triangles"].astype(np.int64)
    v = a["vertices"][:, :3].astype(np.float64)
    corners = np.stack([v[words[9 * root_ids + 0]], v[words[9 * root_ids + 3]], v[words[9 * root_ids + 6]]], axis=1)
    pos = {int(t): i for i, t in enumerate(root_ids)}
    tmin, tmax = corners.min(axis=1), corners.max(axis=1)
    mn = oc["min"][:, :3].astype(np.float64)
    mx = oc["max"][:, :3].astype(np.float64)
    is_leaf = oc["children"][:, 0] == -1
    leaves = nodes[is_leaf[nodes]]
    res = {"incomplete": [], "unsound": [], "tiling": [], "far_face_drift": [], "links": [], "leaves": int(leaves.size), "nodes": int(nodes.size)}
    # completeness and soundness: candidate pairs by bounding boxes (grown by the slack), then the 13 axes
    T = len(root_ids)
    step = max(1, PAIRS_PER_CHUNK // max(T, 1))
    cand_leaf, cand_tri = [], []
    for l0 in range(0, leaves.size, step):
        ll = leaves[l0:l0 + step]
        near = np.all((tmin[None, :, :] <= mx[ll][:, None, :] + slack) & (tmax[None, :, :] >= mn[ll][:, None, :] - slack), axis=2)
        i, j = np.nonzero(near)
        cand_leaf.append(ll[i])
        cand_tri.append(j)
    cand_leaf, cand_tri = np.concatenate(cand_leaf), np.concatenate(cand_tri)
    sep = triangle_box_separation(corners[cand_tri], mn[cand_leaf], mx[cand_leaf]) if cand_leaf.size else np.zeros(0)
    listed = set()
    for leaf in leaves:
        n0, cnt = int(oc[leaf]["trisIndex"]), int(oc[leaf]["trisCount"])
        for t in lst[n0:n0 + cnt]:
            listed.add((int(leaf), pos.get(int(t), -1 - int(t))))
    for leaf, j in zip(cand_leaf[sep < -slack], cand_tri[sep < -slack]):
        if (int(leaf), int(j)) not in listed:
            res["incomplete"].append((int(leaf), int(root_ids[j])))
    overlapping = {(int(leaf), int(j)) for leaf, j in zip(cand_leaf[sep <= slack], cand_tri[sep <= slack])}
    for leaf, j in listed:
        if (leaf, j) not in overlapping:         # not even a candidate, or clear by more than the slack; j < 0: not of this mesh's root list
            res["unsound"].append((leaf, int(root_ids[j]) if j >= 0 else -1 - j))
    # tiling.  Siblings meet float for float and the low faces are the parent's: no gap, no overlap inside a node.  The FAR faces
    # follow the reference's rule child.max = child.min + half_extents (Octree.cpp:195-196), float for float; that sum need not
    # land on the parent's max: where it does not, the node goes to `far_face_drift` with the drift in ulp of the parent's corner.
    f32 = np.float32
    for i in nodes[~is_leaf[nodes]]:
        lo32, hi32 = oc[i]["min"][:3].astype(f32), oc[i]["max"][:3].astype(f32)
        half = (hi32 - lo32) / f32(2)
        ch = oc[i]["children"]
        ok, drift = True, 0.0
        for ci in range(8):
            cl, chh = oc[ch[ci]]["min"][:3].astype(f32), oc[ch[ci]]["max"][:3].astype(f32)
            ok &= bool(np.all(chh == cl + half))
            for k, sh in enumerate((4, 2, 1)):                            # x, y, z
                if ci & sh == 0:
                    ok &= bool(cl[k] == lo32[k])
                else:
                    ok &= bool(cl[k] == oc[ch[ci & ~sh]]["max"][k])
                    if chh[k] != hi32[k]:
                        drift = max(drift, abs(float(chh[k]) - float(hi32[k])) / float(np.spacing(max(abs(lo32[k]), abs(hi32[k])))))
        if not ok:
            res["tiling"].append(int(i))
        if drift:
            res["far_face_drift"].append((int(i), drift))
    # neighbour links (tolerance: the slack — far faces drift by an ulp or two per level, cells are thousands of ulp wide)
    rlo, rhi = mn[root_index], mx[root_index]
    axis_of_side = {0: 2, 1: 2, 2: 0, 3: 0, 4: 1, 5: 1}
    for i in nodes:
        ext = mx[i] - mn[i]
        for side in range(6):
            ax, up = axis_of_side[side], side % 2
            nb = int(oc[i]["neighbors"][side])
            if nb != -1 and not (0 <= nb < len(oc)):
                res["links"].append((int(i), side))
                continue
            if rhi[ax] - rlo[ax] > 4 * slack:            # (a root box flat along this axis has every cell on both of its faces: no verdict)
                on_boundary = abs(mx[i][ax] - rhi[ax]) <= slack if up else abs(mn[i][ax] - rlo[ax]) <= slack
                if (nb == -1) != bool(on_boundary):
                    res["links"].append((int(i), side))
                    continue
            if nb == -1:
                continue
            p = 0.5 * (mn[i] + mx[i])
            p[ax] = (mx[i][ax] + 0.5 * ext[ax]) if up else (mn[i][ax] - 0.5 * ext[ax])
            inside = np.all((mn[nb] - slack <= p) & (p <= mx[nb] + slack))
            larger = np.all(mx[nb] - mn[nb] >= ext - 2 * slack)
            if not (inside and larger):
                res["links"].append((int(i), side))
    return res


def octree_slack(scene, root_index):
    """The slack of the completeness / soundness tests: the builder forms box corners, centres, half extents and centre-relative
    vertices in float (a rounding each, 2^-24 relative to the largest coordinate in play), and its 13 axis tests compare sums of
    three products of them; 16 ulp of the largest coordinate magnitude of root box and vertices covers those with room."""
    a = arrays(scene)
    root = a["octrees"][root_index]
    big = max(float(np.abs(root["min"][:3]).max()), float(np.abs(root["max"][:3]).max()))
    return 16.0 * U * big


# ---- the meshes both test files run on ---------------------------------------------------------------------------------------------

MESH_CASES = ("bunny", "pear", "kat-pear", "kat-bunny", "cube", "triangle", "dense")
RAYS_PER_FAMILY = {"dense": 400}          # 19 872 triangles: fewer rays keep the brute force's share of the run small
DEFAULT_RAYS_PER_FAMILY = 860             # 7 x 860 = 6 020 rays per mesh


def load_case(name, tmp_dir, kat_state=((0.2, -0.1, 0.4), 3.0)):
    """(scene, object index of the mesh, origins_off_the_box) of one of MESH_CASES: Scenes/bunny.txt; the pear of
    Scenes/shadows.txt; the pear as SECOND mesh and the scaled, turned, moving bunny of tests/test_gpu_kat.py's KAT_SCENE;
    Models/cube.obj and Models/triangle.obj in a one-object scene; Models/bunny.obj subdivided once by tools/dense_mesh.py."""
    import os
    import sys
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.scene import ASSET_ROOT
    off = 0.0
    if name in ("bunny", "pear"):
        scene = Scene.from_file("bunny" if name == "bunny" else "shadows")
        scene.update_objects()
        obj = int(np.flatnonzero(scene.objects()["type"] == 2)[0])
    elif name in ("kat-pear", "kat-bunny"):
        from test_gpu_kat import KAT_SCENE
        scene = Scene()
        scene.inputScene(KAT_SCENE)
        scene.set_camera(*kat_state)
        scene.update_objects()
        obj = 4 if name == "kat-pear" else 5
    else:
        if name == "dense":
            sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
            from dense_mesh import subdivide_obj
            os.makedirs(os.path.join(str(tmp_dir), "Models"), exist_ok=True)
            subdivide_obj(os.path.join(ASSET_ROOT, "Models", "bunny.obj"), os.path.join(str(tmp_dir), "Models", "bunny_x4.obj"), 1)
            scene = Scene(asset_root=str(tmp_dir))
            model = "Models/bunny_x4.obj"
        else:
            scene = Scene()
            model = f"Models/{name}.obj"
            # every triangle of cube.obj / triangle.obj lies in a face of the root box (ray_families); the flat triangle.obj needs its
            # origins well off its plane, or the "inside" and "on the box" families are grazing rays only
            off = 0.01 if name == "cube" else 0.25
        scene.inputScene(f"M{model}\nOm0\n p0.5,-1,6,0.6,0.2,1,0.1,2,1.5,2.5\n c0.8,0.5,0.3\nA0.2\nR\n")
        scene.update_objects()
        obj = 0
    return scene, obj, off


def case_rays(name, scene, obj, off):
    """The fixed-seed rays of one mesh case: (rays float32 (n, 6), family (n,))."""
    import zlib
    _, tris = mesh_triangles(scene, obj)
    lo, hi = root_box(scene, obj)
    rng = np.random.default_rng(zlib.crc32(name.encode()) + 20261016)
    return ray_families(lo, hi, tris, rng, RAYS_PER_FAMILY.get(name, DEFAULT_RAYS_PER_FAMILY), origins_off_the_box=off)


def check_walk(label, scene, obj, rays, fam, got, bf=None, **kw):
    """Print the figures of one walk against the brute force and assert the conditions the comparison stands on: flags equal on
    EVERY well-conditioned ray, distance / normal / (u, v) of every well-conditioned hit within its derived bound, the filters
    not hiding the sample (per family but the vertex / edge one >= 90 % well-conditioned, >= 80 % over all, of the
    well-conditioned >= 25 % hits and >= 10 % misses, the aimed family all hits), and every ill-conditioned flag disagreement
    answered both ways by the grown / shrunk brute force.  Returns compare_walk's dict."""
    c = compare_walk(scene, obj, rays, got, bf=bf, **kw)
    b, well = c["bf"], c["well"]
    n_well = int(well.sum())
    hits, misses = int((well & b["hit"]).sum()), int((well & ~b["hit"]).sum())
    shares = [float(well[fam == f].mean()) for f in range(len(FAMILIES))]
    print(f"\n{label}: {len(rays)} rays, {len(mesh_triangles(scene, obj)[0])} triangles; well-conditioned {n_well} ({n_well / len(rays):.1%}): "
          f"{hits} hits, {misses} misses; ill-conditioned flag disagreements {len(c['ill_flag'])} (unexplained {len(c['ill_unexplained'])})")
    print("   well-conditioned share per family: " + ", ".join(f"{FAMILIES[f]} {shares[f]:.1%}" for f in range(len(FAMILIES))))
    for k, rel in (("dist", True), ("normal", False), ("uv", False)):
        e, t = c["err_" + k], c["tol_" + k]
        ok = np.isfinite(e) & np.isfinite(t)
        if ok.any():
            scale = np.maximum(c["dist"][ok], 1e-300) if rel else 1.0
            print(f"   {k:6s} error{' (relative)' if rel else ''}: median {np.median(e[ok] / scale):.2e}, max {np.max(e[ok] / scale):.2e};  "
                  f"derived bound: median {np.median(t[ok] / scale):.2e};  largest error / bound {np.max(e[ok] / np.maximum(t[ok], 1e-300)):.3f}")
    with np.errstate(invalid="ignore"):
        rel_any = c["err_dist_any"] / np.maximum(c["dist"], 1e-300)
        only_margin = (b["margin"] > MARGIN) & ~well & np.isfinite(rel_any)
        if only_margin.any():
            i = int(np.flatnonzero(only_margin)[np.argmax(rel_any[only_margin])])
            print(f"   largest relative distance error with the edge margin alone: {rel_any[i]:.2e} (|cos| {b['cos'][i]:.3f}, gap {b['gap'][i]:.1e})")
    assert c["flag_bad"].size == 0, (label, "hit flag differs on well-conditioned rays", c["flag_bad"][:8], np.asarray(rays)[c["flag_bad"][:3]])
    assert c["attr_bad"].size == 0, (label, "another triangle, or beyond the bound", c["attr_bad"][:8], np.asarray(rays)[c["attr_bad"][:3]])
    assert c["ill_unexplained"].size == 0, (label, "ill-conditioned disagreement the slack does not explain", c["ill_unexplained"][:8])
    for f in range(len(FAMILIES)):
        assert f == ILL_FAMILY or shares[f] >= 0.90, (label, FAMILIES[f], shares[f])
    assert n_well >= 0.80 * len(rays), (label, n_well)
    assert hits >= 0.25 * n_well and misses >= 0.10 * n_well, (label, hits, misses, n_well)
    assert b["hit"][fam == 2].all(), (label, "a ray aimed at the interior of a triangle misses the mesh in float64")
    return c
