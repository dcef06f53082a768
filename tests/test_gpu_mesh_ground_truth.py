"""The DEVICE's mesh path against the float64 brute force and the geometry (tests/mesh_truth.py): the comparisons of
tests/test_mesh_ground_truth.py with rpt_probe_walk, rpt_probe_object and rpt_build_octree in the oracle's and the host builder's
place — so that they keep holding if a later change moves kernel and oracle together.  Same rays, same filters, same derived
tolerances, same conditions."""
import numpy as np
import pytest

import mesh_truth as mt
from mesh_soups import SOUP_SEEDS, write_soup

pytestmark = pytest.mark.gpu

WALKS = ("reference layouts", "throughput walk (kernel 41)", "latency walk (kernel 43)")
_cases = {}


@pytest.fixture(scope="module")
def renderer():
    from relativitypathtracer_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


def _case(name, tmp_path_factory, **kw):
    key = (name, tuple(sorted(kw.items())))
    if key not in _cases:
        scene, obj, off = mt.load_case(name, tmp_path_factory.mktemp(name), **kw)
        rays, fam = mt.case_rays(name, scene, obj, off)
        _cases[key] = (scene, obj, rays, fam, mt.brute_force(rays, mt.mesh_triangles(scene, obj)[1]))
    return _cases[key]


def _exact_rcp_of_a_frame(r, scene):
    r.set_scene_params(scene, 64, 36)
    r.set_output(None)
    r.set_variant(41)
    r.render()
    exact = r.last_exact_rcp()
    r.set_variant(0)
    return exact


@pytest.mark.parametrize("name", mt.MESH_CASES)
def test_device_walks_return_the_nearest_triangle(renderer, name, tmp_path_factory):
    """rpt_probe_walk — the reference-layout walk, the throughput walk and the latency walk, with the exact reciprocal of the
    triangle test — ray by ray against Moeller-Trumbore in float64 over every triangle."""
    scene, obj, rays, fam, bf = _case(name, tmp_path_factory)
    renderer.upload_scene(scene)
    assert _exact_rcp_of_a_frame(renderer, scene)
    got = renderer.probe_walk(obj, rays)
    for w, walk in enumerate(WALKS):
        mt.check_walk(f"device {walk}, {name}", scene, obj, rays, fam, got[:, w, :], bf=bf)


def test_device_walks_with_the_ieee_division(renderer, tmp_path_factory, tmp_path):
    """The same on a scene outside the exact reciprocal's domain (a second mesh with |e1| |e2| > 2^60 in the pool, named by no
    object): the walks' IEEE-division twins face the ground truth too."""
    from relativitypathtracer_amd import Scene
    _, obj, rays, fam, bf = _case("bunny", tmp_path_factory)
    huge = tmp_path / "huge.obj"
    huge.write_text("v -2147483648 -2147483648 8589934592\nv 2147483648 -2147483648 8589934592\nv 0 2147483648 8589934592\n"
                    "vt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")
    scene = Scene.from_file("bunny")
    scene.ReadOBJ(str(huge))
    scene.update_objects()
    renderer.upload_scene(scene)
    assert not _exact_rcp_of_a_frame(renderer, scene)
    got = renderer.probe_walk(obj, rays)
    for w, walk in enumerate(WALKS):
        mt.check_walk(f"device {walk}, IEEE division, bunny", scene, obj, rays, fam, got[:, w, :], bf=bf)


KAT_STATES = [((0.0, 0.0, 0.0), 0.0), ((0.2, -0.1, 0.4), 3.0), ((0.0, 0.0, 0.95), 7.0)]       # test_gpu_kat.test_sample_light_at_ray_level's


def _object_space(o, org4, dir4):
    """A 4-D rest-frame ray into the object's space with its own InvM AS FLOAT64, and how far the float walk's ray may lie from
    that at a point `reach` along it: transformPoint / transformDirection in float are 4-term dots, 4u of their operands each."""
    InvM = o["InvM"].astype(np.float64)
    wo, wd = org4[:, 1:4], dir4[:, 1:4]
    rays = np.hstack([wo @ InvM[:3, :3].T + InvM[:3, 3], wd @ InvM[:3, :3].T])
    n3 = np.linalg.norm(InvM[:3, :3], 2)
    eps_o = 4 * mt.U * (n3 * np.linalg.norm(wo, axis=1) + np.linalg.norm(InvM[:3, 3]))
    return rays, eps_o


def _check_object_form(label, scene, obj, fam, org4, dir4, got):
    o = scene.objects()[obj]
    rays, eps_o = _object_space(o, org4, dir4)
    _, tris = mt.mesh_triangles(scene, obj)
    bf = mt.brute_force(rays, tris)
    reach = np.where(bf["hit"], bf["t"], 0.0) * np.linalg.norm(rays[:, 3:6], axis=1)
    extra = eps_o + 8 * mt.U * reach           # the direction: 4u from the transform, its normalisation and the scale a few more
    mt.check_walk(label, scene, obj, rays, fam, got, bf=bf, world_origin=org4[:, 1:4], world_dirlen=np.linalg.norm(dir4[:, 1:4], axis=1),
                  extra_dq=extra)


@pytest.mark.parametrize("state", KAT_STATES)
@pytest.mark.parametrize("obj", [4, 5])
def test_device_mesh_intersector_general_form(renderer, state, obj, tmp_path_factory):
    """rpt_probe_object which = 0, the general 4-D form, on the two mesh objects of KAT_SCENE — the pear as second mesh and the
    scaled, turned, MOVING bunny — at three camera states.  Each rest-frame ray is mapped into object space in float64 with the
    object's own InvM taken as float64 and brute-forced there; flag, distance, normal and (u, v) are compared.  (The float64
    transform of float32 matrices is no independent model of the relativity: the matrices themselves are
    tests/test_scene_frontend.py's business.  What this pins is the mesh intersection of a moving, scaled, turned mesh.)"""
    name = "kat-pear" if obj == 4 else "kat-bunny"
    scene, obj_, orays, fam, _ = _case(name, tmp_path_factory, kat_state=state)
    assert obj_ == obj
    M = scene.objects()[obj]["M"].astype(np.float64)
    rng = np.random.default_rng(31 + obj)
    n = len(orays)
    scale = np.exp(rng.uniform(-1, 1, size=(n, 1)))
    rays8 = np.zeros((n, 8), dtype=np.float32)
    rays8[:, 0] = rng.uniform(-5, 5, size=n)
    rays8[:, 1:4] = orays[:, :3].astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    rays8[:, 4] = rng.choice([-1.0, 0.0, -2.5], size=n)
    rays8[:, 5:8] = (orays[:, 3:6].astype(np.float64) @ M[:3, :3].T) * scale
    renderer.upload_scene(scene)
    renderer.set_scene_params(scene, 64, 64)
    got = renderer.probe_object(0, obj, rays8)
    r64 = rays8.astype(np.float64)
    _check_object_form(f"device general form, object {obj}, camera {state}", scene, obj, fam, r64[:, 0:4], r64[:, 4:8], got)


@pytest.mark.parametrize("state", KAT_STATES)
@pytest.mark.parametrize("obj", [4, 5])
def test_device_mesh_intersector_primary_ray_form(renderer, state, obj, tmp_path_factory):
    """rpt_probe_object which = 3, the default kernels' primary-ray form: camera directions aimed so that their rest-frame rays
    (origin stationaryCam, direction Lorentz * (interval, nd), both as float64 of the object's float32 record) are the family rays;
    brute force in object space as above."""
    name = "kat-pear" if obj == 4 else "kat-bunny"
    scene, _, orays, fam, _ = _case(name, tmp_path_factory, kat_state=state)
    o = scene.objects()[obj]
    M, L, InvL = (o[k].astype(np.float64) for k in ("M", "Lorentz", "InvLorentz"))
    cam4 = o["stationaryCam"].astype(np.float64)
    interval = float(scene.params["interval"])
    # targets: a point on each family ray (its first hit where it has one, else the point nearest the box centre), in the rest frame
    lo, hi = mt.root_box(scene, obj)
    _, tris = mt.mesh_triangles(scene, obj)
    r0 = orays.astype(np.float64)
    bf0 = mt.brute_force(r0, tris)
    s = np.where(bf0["hit"], bf0["t"], np.einsum("ij,ij->i", 0.5 * (lo + hi) - r0[:, :3], r0[:, 3:6]))
    target = (r0[:, :3] + r0[:, 3:6] * s[:, None]) @ M[:3, :3].T + M[:3, 3]
    w = target - cam4[1:4]
    if interval == 0.0:
        t0 = -(w @ InvL[0, 1:4]) / InvL[0, 0]
    else:
        t0 = -np.linalg.norm(w, axis=1)              # light-like, into the past
    b = np.hstack([t0[:, None], w]) @ InvL.T
    cam = (b[:, 1:4] / np.linalg.norm(b[:, 1:4], axis=1, keepdims=True)).astype(np.float32)
    renderer.upload_scene(scene)
    renderer.set_scene_params(scene, 64, 64)
    got = renderer.probe_object(3, obj, cam)
    nd = cam.astype(np.float64)
    nd /= np.linalg.norm(nd, axis=1, keepdims=True)
    dir4 = np.hstack([np.full((len(nd), 1), interval), nd]) @ L.T
    org4 = np.tile(cam4, (len(nd), 1))
    # one family for the conditions that make sense here: these rays all start at the camera
    o_rays, eps_o = _object_space(o, org4, dir4)
    bf = mt.brute_force(o_rays, tris)
    reach = np.where(bf["hit"], bf["t"], 0.0) * np.linalg.norm(o_rays[:, 3:6], axis=1)
    c = mt.compare_walk(scene, obj, o_rays, got, bf=bf, world_origin=org4[:, 1:4], world_dirlen=np.linalg.norm(dir4[:, 1:4], axis=1),
                        extra_dq=eps_o + 16 * mt.U * reach)
    well, hits = c["well"], c["well"] & bf["hit"]
    print(f"\ndevice primary-ray form, object {obj}, camera {state}: {len(cam)} rays, well-conditioned {int(well.sum())}, hits {int(hits.sum())}, "
          f"ill-conditioned flag disagreements {len(c['ill_flag'])} (unexplained {len(c['ill_unexplained'])})")
    assert c["flag_bad"].size == 0 and c["attr_bad"].size == 0 and c["ill_unexplained"].size == 0, (c["flag_bad"][:5], c["attr_bad"][:5])
    assert well.sum() >= 0.8 * len(cam) and hits.sum() >= 0.25 * well.sum() and (well & ~bf["hit"]).sum() >= 0.10 * well.sum()


def _device_octree(renderer, paths, asset_root=None):
    from relativitypathtracer_amd import Scene
    scene = Scene(**({} if asset_root is None else {"asset_root": asset_root}))
    for p in paths:
        renderer.build_octree(scene, scene.ReadOBJ(p, octree=False))
    return scene


def _octree_check(label, scene, root):
    a = mt.arrays(scene)
    res = mt.check_octree(a, root, mt.octree_slack(a, root))
    drift = res["far_face_drift"]
    print(f"\n{label}: {res['nodes']} nodes, {res['leaves']} leaves; incomplete {len(res['incomplete'])}, unsound {len(res['unsound'])}, "
          f"tiling {len(res['tiling'])}, links {len(res['links'])}; far faces off by rounding: {len(drift)} nodes")
    for k in ("incomplete", "unsound", "tiling", "links"):
        assert not res[k], (label, k, len(res[k]), res[k][:6])
    assert all(d <= 2.0 for _, d in drift)          # as in tests/test_mesh_ground_truth.py


@pytest.mark.parametrize("paths", [["Models/bunny.obj"], ["Models/cube.obj"], ["Models/triangle.obj"], ["Models/bunny.obj", "Models/pear.obj"], ["dense"]])
def test_device_octree_against_the_geometry(renderer, paths, tmp_path):
    """rpt_build_octree's own output (not the host builder's) through the completeness, soundness, tiling and link tests: the
    shipped models (the pear also as second mesh, whose root lists the bunny's triangles too) and the dense mesh."""
    root_dir = None
    if paths == ["dense"]:
        import os
        import sys
        sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
        from dense_mesh import subdivide_obj
        from relativitypathtracer_amd.scene import ASSET_ROOT
        os.makedirs(tmp_path / "Models")
        subdivide_obj(os.path.join(ASSET_ROOT, "Models", "bunny.obj"), str(tmp_path / "Models" / "bunny_x4.obj"), 1)
        paths, root_dir = [str(tmp_path / "Models" / "bunny_x4.obj")], "/"
    scene = _device_octree(renderer, paths, root_dir)
    for root in scene.mesh_roots():
        _octree_check(f"device octree, {paths}, root {root}", scene, int(root))


@pytest.mark.parametrize("seed", SOUP_SEEDS)
def test_device_octree_of_random_soups_against_the_geometry(renderer, seed, tmp_path):
    scene = _device_octree(renderer, [write_soup(tmp_path, seed)], "/")
    _octree_check(f"device octree, soup {seed}", scene, int(scene.mesh_roots()[0]))
