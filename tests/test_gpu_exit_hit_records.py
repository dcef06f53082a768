"""The walk through exit records and hit records (csrc/rpt_kernels.hip.h: DExit, DHit) on the device: rpt_probe_walk against the
oracle's intersect_octree ray by ray, bit for bit, on the meshes where the records take every form — a flat root split once (no exit to an inner
node, most of them "none"), a shallow tree, cells of unequal depth side by side, and a list of 255 triangles and more, whose full count is read
through an exit record — and the frames of kernels 41, 43 and 1 against the golden frames of the oracle."""
import os

import numpy as np
import pytest

import derived_layout_helpers as dl
import mesh_truth as mt
import oracle_ffi

pytestmark = pytest.mark.gpu

N_RAYS = 4096
W, H = 128, 72
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def renderer():
    from relativitypathtracer_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


def kat_rays(lo, hi, verts, n, seed):
    """The ray families of tests/test_gpu_kat.py::test_octree_walk_at_ray_level, n rays: from outside towards the box, from inside
    it, aimed at mesh vertices, parallel to one and two axes, origins ON faces, edges and corners of the root box, grazing and missing."""
    rng = np.random.default_rng(seed)
    ext = np.where(hi > lo, hi - lo, np.linalg.norm(hi - lo))          # (a flat root box has a zero extent)
    diag = np.linalg.norm(hi - lo)
    rays = np.empty((n, 6), dtype=np.float64)
    unit = lambda v: v / np.linalg.norm(v, axis=-1, keepdims=True)     # noqa: E731
    k = n // 6
    far = unit(rng.normal(size=(k, 3))) * rng.uniform(1.5, 6.0, size=(k, 1)) * diag + 0.5 * (lo + hi)
    rays[:k, :3] = far
    rays[:k, 3:] = unit(rng.uniform(lo - 0.1 * ext, hi + 0.1 * ext, size=(k, 3)) - far)
    rays[k:2 * k, :3] = rng.uniform(lo, hi, size=(k, 3))
    rays[k:2 * k, 3:] = unit(rng.normal(size=(k, 3)))
    o2 = unit(rng.normal(size=(k, 3))) * 3.0 * diag + 0.5 * (lo + hi)
    rays[2 * k:3 * k, :3] = o2
    rays[2 * k:3 * k, 3:] = unit(verts[rng.integers(0, len(verts), size=k)] - o2)
    d3 = np.zeros((k, 3))
    ax = rng.integers(0, 3, size=k)
    d3[np.arange(k), ax] = rng.choice([-1.0, 1.0], size=k)
    two = rng.random(k) < 0.5
    d3[two, (ax[two] + 1) % 3] = rng.normal(size=int(two.sum()))
    rays[3 * k:4 * k, 3:] = unit(d3)
    rays[3 * k:4 * k, :3] = rng.uniform(lo - 0.5 * ext, hi + 0.5 * ext, size=(k, 3))
    ob = rng.uniform(lo, hi, size=(k, 3))
    snap = rng.random((k, 3)) < 0.5
    snap[np.arange(k), rng.integers(0, 3, size=k)] = True
    side = rng.random((k, 3)) < 0.5
    ob = np.where(snap, np.where(side, lo, hi), ob)
    rays[4 * k:5 * k, :3] = ob
    rays[4 * k:5 * k, 3:] = unit(rng.normal(size=(k, 3)))
    rest = n - 5 * k
    og = rng.uniform(lo - 1.0 * ext, hi + 1.0 * ext, size=(rest, 3))
    axis = rng.integers(0, 3, size=rest)
    og[np.arange(rest), axis] = np.where(rng.random(rest) < 0.5, lo[axis], hi[axis]) * (1.0 + rng.choice([-1e-6, 0.0, 1e-6], size=rest))
    dg = rng.normal(size=(rest, 3))
    dg[np.arange(rest), axis] *= rng.choice([0.0, 1e-4, 1.0], size=rest)
    rays[5 * k:, :3] = og
    rays[5 * k:, 3:] = unit(dg)
    return rays.astype(np.float32)


@pytest.mark.parametrize("name", ["triangle", "cube", "pear", "soup"])
def test_walk_through_exit_and_hit_records_equals_the_oracle(renderer, name, tmp_path):
    if name == "soup":
        scene, obj = dl.soup_scene(tmp_path), 0
        assert dl.exits_into_long_lists(dl.layout(scene, dl.NODES), dl.layout(scene, dl.EXITS)) > 0
    else:
        scene, obj, _ = mt.load_case(name, tmp_path)
    lo, hi = mt.root_box(scene, obj)
    ids, corners = mt.mesh_triangles(scene, obj)
    rays = kat_rays(lo, hi, corners.reshape(-1, 3), N_RAYS, 20261018 + len(name))
    want = oracle_ffi.octree_rays(scene, obj, rays)
    renderer.upload_scene(scene)
    got = renderer.probe_walk(obj, rays)
    hits = int(want[:, 0].sum())
    print(f"\n{name}: {len(ids)} triangles, {hits} of {N_RAYS} rays hit")
    assert 0 < hits < N_RAYS
    for w, walk in enumerate(("reference layouts", "throughput walk", "latency walk")):
        g = got[:, w, :]
        same = (g.view(np.uint32) == want.view(np.uint32)) | (np.isnan(g) & np.isnan(want))
        bad = np.flatnonzero(~same.all(axis=1))
        assert bad.size == 0, (name, walk, bad.size, bad[:5], rays[bad[:2]], g[bad[:2]], want[bad[:2]])


@pytest.mark.parametrize("name", ["bunny", "shadows"])
def test_frames_of_41_43_and_1_equal_the_golden_frames(renderer, name):
    from conftest import load_config
    g = np.load(os.path.join(GOLDEN, f"oracle_{name}_128x72.npz"))
    scene = load_config(name)
    assert np.array_equal(scene.buffers()["objects"], g["objects"]), "Object[] bytes drifted"
    renderer.upload_scene(scene)
    try:
        for variant in (41, 43, 1):
            renderer.set_scene_params(scene, W, H)
            renderer.set_output(None)
            renderer.set_debug_rgb(True)
            renderer.set_variant(variant)
            renderer.render()
            assert renderer.last_variant() == variant
            px, rgb = renderer.read_framebuffer(), renderer.read_debug_rgb()
            assert np.array_equal(px["rgba"].reshape(H, W, 4), g["rgba"]), (name, variant)
            assert np.array_equal(np.ascontiguousarray(rgb).view(np.uint32).reshape(g["rgb"].shape), g["rgb"].view(np.uint32)), (name, variant)
    finally:
        renderer.set_variant(0)
        renderer.set_debug_rgb(False)
