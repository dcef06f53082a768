"""The mesh path against a float64 brute force over all triangles, and the octree against the geometry (tests/mesh_truth.py).

Every other test of the mesh path compares two implementations of one reading of the reference (kernel and oracle, device
builder and host builder).  These ask the question from outside: does the walk return the triangle a ray really hits, does a
leaf list the triangles that really lie in it, does a link lead to the cell that really lies beyond that face.  Here: the CPU
oracle and the host builder, on every machine; tests/test_gpu_mesh_ground_truth.py: the device in their place.

Figures of the oracle's walk at the commit that added this file (6 020 rays per mesh, 2 800 on the dense one): relative distance
error median 3e-8 .. 6e-8, largest 1.5e-5 (derived bound: median 1e-5 .. 1e-4; largest error / bound 0.20); normal error
largest 7.4e-4 (bound median 1e-2); no flag disagreement on 35 000 well-conditioned rays."""
import ctypes as C

import numpy as np
import pytest

import mesh_truth as mt
import oracle_ffi
from mesh_soups import SOUP_SEEDS, write_soup

_cases = {}


def _case(name, tmp_path_factory):
    if name not in _cases:
        scene, obj, off = mt.load_case(name, tmp_path_factory.mktemp(name.replace(" ", "_")))
        rays, fam = mt.case_rays(name, scene, obj, off)
        _cases[name] = (scene, obj, rays, fam)
    return _cases[name]


def oracle_walk(a, object_index, rays):
    """rpt_oracle_octree_rays on the arrays of mesh_truth.arrays() — the scene's own or a corrupted copy."""
    args = oracle_ffi.OracleArgs()
    keep = {k: np.ascontiguousarray(a[k]) for k in ("objects", "vertices", "normals", "uvs", "triangles", "octrees", "octreeTris")}
    args.objects, args.object_count = keep["objects"].ctypes.data, len(keep["objects"])
    for k in ("vertices", "normals", "uvs", "triangles", "octrees", "octreeTris"):
        setattr(args, k, keep[k].ctypes.data)
    rays = np.ascontiguousarray(rays, dtype=np.float32)
    out = np.empty((len(rays), 8), dtype=np.float32)
    rc = oracle_ffi.lib().rpt_oracle_octree_rays(C.byref(args), int(object_index), rays.ctypes.data, out.ctypes.data, len(rays))
    assert rc == 0
    return out


@pytest.mark.parametrize("name", mt.MESH_CASES)
def test_oracle_walk_returns_the_nearest_triangle(name, tmp_path_factory):
    """intersect_octree of the oracle, ray by ray against Moeller-Trumbore in float64 over every triangle of the mesh: the same
    hit flag on EVERY well-conditioned ray, and on hits the same triangle — distance, interpolated normal and (u, v) within the
    bounds derived in mesh_truth's docstring."""
    scene, obj, rays, fam = _case(name, tmp_path_factory)
    got = oracle_ffi.octree_rays(scene, obj, rays)
    mt.check_walk(f"oracle, {name}", scene, obj, rays, fam, got)


def _octree_report(label, res):
    print(f"\n{label}: {res['nodes']} nodes, {res['leaves']} leaves; incomplete {len(res['incomplete'])}, unsound {len(res['unsound'])}, "
          f"tiling {len(res['tiling'])}, links {len(res['links'])}")
    drift = res["far_face_drift"]
    print(f"   far faces off the parent's by rounding (Octree.cpp:196): {len(drift)} inner nodes, at most {max([d for _, d in drift], default=0):.1f} ulp")
    for k in ("incomplete", "unsound", "tiling", "links"):
        assert not res[k], (label, k, len(res[k]), res[k][:6])
    # child.max = fl(fl(min + half) + half) against the parent's max: half carries the rounding of (max - min) (0.5 ulp of the extent),
    # each sum one of its own (0.5 ulp of a corner): at most 2 ulp of the parent's larger corner
    assert all(d <= 2.0 for _, d in drift), (label, max(d for _, d in drift))
    return len(drift)


@pytest.mark.parametrize("name", mt.MESH_CASES)
def test_host_octree_against_the_geometry(name, tmp_path_factory):
    """The host builder's octree of every mesh case: each leaf lists every triangle of the root list that overlaps its box by
    more than the slack (completeness) and none that is clear of it by more than the slack (soundness; the builder's rule is
    the exact 13-axis overlap test in float, Octree.cpp:6-169, so soundness holds as strictly as completeness); the children of
    every inner node tile it float for float; every link leads to the cell beyond that face.  Slack: mesh_truth.octree_slack."""
    scene, obj, _, _ = _case(name, tmp_path_factory)
    a = mt.arrays(scene)
    root = int(a["objects"][obj]["meshIndex"])
    _octree_report(f"host octree, {name}", mt.check_octree(a, root, mt.octree_slack(a, root)))


@pytest.mark.parametrize("seed", SOUP_SEEDS)
def test_host_octree_of_random_soups_against_the_geometry(seed, tmp_path):
    from relativitypathtracer_amd import Scene
    scene = Scene(asset_root="/")
    scene.ReadOBJ(write_soup(tmp_path, seed))
    a = mt.arrays(scene)
    root = int(scene.mesh_roots()[0])
    _octree_report(f"host octree, soup {seed}", mt.check_octree(a, root, mt.octree_slack(a, root)))


# ---- the check has teeth: corrupt a COPY of the scene's arrays (never the library, never anything sent to a GPU) -------------------

def _lonely_leaf(a, root):
    """A leaf with exactly one entry that is also the only leaf holding that triangle's centroid; of those, the one whose
    triangle the fewest other leaves list.  Returns (leaf, triangle, centroid)."""
    oc, lst = a["octrees"], a["octreeTris"]
    nodes, _ = mt.mesh_nodes(a, root)
    leaves = nodes[oc["children"][nodes, 0] == -1]
    words = a["triangles"].astype(np.int64)
    v = a["vertices"][:, :3].astype(np.float64)
    count = np.bincount(np.concatenate([lst[int(oc[l]["trisIndex"]): int(oc[l]["trisIndex"]) + int(oc[l]["trisCount"])] for l in leaves]))
    lmin, lmax = oc["min"][leaves][:, :3].astype(np.float64), oc["max"][leaves][:, :3].astype(np.float64)
    best = None
    for l in leaves[oc["trisCount"][leaves] == 1]:
        t = int(lst[int(oc[l]["trisIndex"])])
        cen = (v[words[9 * t]] + v[words[9 * t + 3]] + v[words[9 * t + 6]]) / 3.0
        holding = leaves[np.all((lmin <= cen) & (cen <= lmax), axis=1)]
        if holding.tolist() == [int(l)] and (best is None or count[t] < best[3]):
            best = (int(l), t, cen, int(count[t]))
    assert best is not None
    return best[:3]


def test_a_triangle_missing_from_a_leaf_is_reported(tmp_path_factory):
    """Teeth: take one triangle out of one leaf's list (a copy of bunny's arrays), walk rays aimed at its centroid through the
    oracle: the comparison with the brute force reports hit-flag or wrong-triangle disagreements on well-conditioned rays, and
    the octree check reports the leaf as incomplete."""
    scene, obj, _, _ = _case("bunny", tmp_path_factory)
    a = {k: v.copy() for k, v in mt.arrays(scene).items()}
    root = int(a["objects"][obj]["meshIndex"])
    leaf, tri, cen = _lonely_leaf(a, root)
    a["octrees"]["trisCount"][leaf] -= 1
    # rays that start INSIDE that leaf, a little in front of the triangle, within 60 degrees of its normal: the walk meets the
    # triangle's own leaf first (a ray from far away finds the triangle in the lists of the leaves it crosses before)
    words, v = a["triangles"].astype(np.int64), a["vertices"][:, :3].astype(np.float64)
    A, B, Cc = v[words[9 * tri]], v[words[9 * tri + 3]], v[words[9 * tri + 6]]
    nrm = np.cross(B - A, Cc - A)
    nrm /= np.linalg.norm(nrm)
    rng = np.random.default_rng(7)
    d = rng.normal(size=(4096, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    d = d[np.abs(d @ nrm) > 0.5][:256]
    bmin, bmax = a["octrees"][leaf]["min"][:3].astype(np.float64), a["octrees"][leaf]["max"][:3].astype(np.float64)
    with np.errstate(divide="ignore"):
        room = np.min(np.where(d > 0, (cen - bmin) / np.abs(d), (bmax - cen) / np.abs(d)), axis=1)      # back along -d to the leaf's wall
    org = cen - d * 0.8 * room[:, None]
    rays = np.hstack([org, d]).astype(np.float32)
    intact = mt.compare_walk(scene, obj, rays, oracle_ffi.octree_rays(scene, obj, rays))
    assert intact["flag_bad"].size == 0 and intact["attr_bad"].size == 0 and intact["well"].sum() > 50
    broken = mt.compare_walk(a, obj, rays, oracle_walk(a, obj, rays))
    reported = broken["flag_bad"].size + broken["attr_bad"].size
    print(f"\nleaf {leaf} without triangle {tri}: {reported} of {int(broken['well'].sum())} well-conditioned rays reported")
    assert reported > 0
    res = mt.check_octree(a, root, mt.octree_slack(a, root))
    assert (leaf, tri) in res["incomplete"] and not res["unsound"] and not res["links"]


def test_a_cut_neighbour_link_is_reported(tmp_path_factory):
    """Teeth: one link of an interior leaf redirected to -1 (a copy): the link test names that node and side."""
    scene, obj, _, _ = _case("bunny", tmp_path_factory)
    a = {k: v.copy() for k, v in mt.arrays(scene).items()}
    root = int(a["objects"][obj]["meshIndex"])
    oc = a["octrees"]
    nodes, _ = mt.mesh_nodes(a, root)
    interior = [int(i) for i in nodes if oc[i]["children"][0] == -1 and np.all(oc[i]["neighbors"] != -1)]
    leaf, side = interior[len(interior) // 2], 3
    oc["neighbors"][leaf, side] = -1
    res = mt.check_octree(a, root, mt.octree_slack(a, root))
    assert res["links"] == [(leaf, side)], res["links"][:6]
