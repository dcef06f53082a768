"""Kernel 41 at six waves per SIMD (csrc/rpt_kernels.hip.h: KernelPolicy::park_bystanders): the shading state waits in
LDS across the shadow walks, slot k of lane l at park_lds[k][l], and the exit plan forms its face ids where it picks them.  Every case
names variant 41 itself — the default rule gives frames this small to kernel 43 — and asks for the same bytes as before:

  * partial tiles: lanes outside the frame leave before anything is parked, tiles are cut on both edges;
  * the light loop and the occluder loop against the committed oracle frames, packed bytes and float RGB bit for bit;
  * the camera inside the mesh's root box: walks start in a leaf, the face ids are picked on the first step;
  * four contexts rendering at once on their own streams with the sky fill beside them: one wave's slots are its own;
  * a short sweep over generated scenes with meshes and lights."""
import math
import os
import sys

import numpy as np
import pytest

import oracle_ffi
from conftest import load_config
from relativitypathtracer_amd import Scene

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KERNEL = 41


@pytest.fixture(scope="module")
def renderer():
    from relativitypathtracer_amd.renderer import Renderer
    r = Renderer(0)
    yield r
    r.close()


def _setup(r, scene, W, H, variant=KERNEL, debug_rgb=False):
    r.set_variant(variant)
    r.upload_scene(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_output(None)
    r.set_debug_rgb(debug_rgb)


@pytest.mark.parametrize("name", ["bunny", "shadows"])
def test_partial_tiles_are_the_unculled_frame(renderer, name):
    scene = load_config(name)
    for W, H in ((9, 9), (70, 45), (129, 73)):
        _setup(renderer, scene, W, H)
        n = renderer.verify_frame()
        assert renderer.last_variant() == KERNEL
        assert n == 0, f"{name} {W}x{H}: kernel {KERNEL} differs from the un-culled kernel on {n} pixels"
    renderer.set_variant(0)


@pytest.mark.parametrize("name", ["shadows", "bunny"])
def test_light_and_occluder_loops_match_the_golden_frames(renderer, name):
    g = np.load(os.path.join(GOLDEN, f"oracle_{name}_128x72.npz"))
    scene = load_config(name)
    _setup(renderer, scene, 128, 72, debug_rgb=True)
    for blocking in (True, False):
        if blocking:
            renderer.render()
        else:
            renderer.render_async()
            renderer.sync()
        assert renderer.last_variant() == KERNEL
        px, rgb = renderer.read_framebuffer(), renderer.read_debug_rgb()
        assert np.array_equal(px["rgba"].reshape(72, 128, 4), g["rgba"]), f"{name}: packed bytes differ"
        assert np.array_equal(rgb.view(np.uint32), g["rgb"].view(np.uint32)), f"{name}: float RGB not bit-identical"
    renderer.set_debug_rgb(False)
    renderer.set_variant(0)


def test_camera_inside_the_mesh_root_box(renderer):
    """tests/test_gpu_parity.py::test_camera_inside_the_mesh_root_box's three camera states at 64x64 through kernel 41"""
    scene = Scene.from_file("bunny")
    objs = scene.objects()
    mesh = int(np.flatnonzero(np.asarray(objs["type"]) == 2)[0])
    node = scene.octrees()[int(objs["meshIndex"][mesh])]
    M = np.array(objs[mesh]["M"], dtype=np.float64).reshape(4, 4)
    centre = M[:3, :3] @ (0.5 * (np.array(node["min"][:3], dtype=np.float64) + np.array(node["max"][:3], dtype=np.float64))) + M[:3, 3]
    W, H = 64, 64
    inside_seen = 0
    for frac, speed in ((1.0, 0.5), (0.8, 0.3), (1.15, 0.7)):
        target = centre * frac
        d = target / np.linalg.norm(target)
        gamma = 1.0 / math.sqrt(1.0 - speed * speed)
        scene.set_camera(tuple(float(x) for x in d * speed), float(np.linalg.norm(target) / (gamma * speed)))
        scene.update_objects()
        opx, orgb, st = oracle_ffi.render(scene, W, H, want_stats=True)
        inside_seen += int(st["inside_starts"] > 0.5 * W * H)
        _setup(renderer, scene, W, H, debug_rgb=True)
        renderer.render()
        assert renderer.last_variant() == KERNEL
        px, rgb = renderer.read_framebuffer(), renderer.read_debug_rgb()
        assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32)), f"frac {frac}: float RGB not bit-identical"
        assert np.array_equal(px["rgba"], opx["rgba"]), f"frac {frac}: packed bytes differ"
        assert renderer.verify_frame() == 0
    assert inside_seen >= 1
    renderer.set_debug_rgb(False)
    renderer.set_variant(0)


def test_four_contexts_side_by_side_with_the_sky_fill():
    """Four contexts share one scene and keep three 256x144 frames each in flight on their own streams, split (RPT_SKY_SPLIT_MIN_PIXELS=0
    when the contexts are created), so that walking waves of different launches and the fill's waves share the SIMDs and the LDS: every
    framebuffer is the blocking un-culled frame, all 16 bytes of every pixel."""
    import torch
    from relativitypathtracer_amd.renderer import Renderer
    W, H, N = 256, 144, 4
    scene = load_config("bunny")
    saved = os.environ.get("RPT_SKY_SPLIT_MIN_PIXELS")
    os.environ["RPT_SKY_SPLIT_MIN_PIXELS"] = "0"
    try:
        ctxs = [Renderer(0) for _ in range(N)]
    finally:
        if saved is None:
            os.environ.pop("RPT_SKY_SPLIT_MIN_PIXELS", None)
        else:
            os.environ["RPT_SKY_SPLIT_MIN_PIXELS"] = saved
    streams = [torch.cuda.Stream(device="cuda:0") for _ in range(N)]
    try:
        ctxs[0].upload_scene(scene)
        for r in ctxs[1:]:
            r.share_scene(ctxs[0])
        for r in ctxs:
            r.set_scene_params(scene, W, H)
            r.set_objects(scene)
        want = torch.full((H * W * 16,), 0xAB, dtype=torch.uint8, device="cuda:0")
        bufs = [torch.full((H * W * 16,), 0xAB, dtype=torch.uint8, device="cuda:0") for _ in range(N)]
        torch.cuda.synchronize()
        ctxs[0].set_output(want.data_ptr())
        ctxs[0].set_variant(3)
        ctxs[0].render()
        assert ctxs[0].last_variant() == 3
        for r, s, b in zip(ctxs, streams, bufs):
            r.set_stream(s.cuda_stream)
            r.set_output(b.data_ptr())
            r.set_variant(KERNEL)
        for _ in range(3):
            for r in ctxs:
                r.render_async()
        for r in ctxs:
            r.sync()
        want = want.cpu().numpy().reshape(H, W, 16)
        for k, (r, b) in enumerate(zip(ctxs, bufs)):
            assert r.last_variant() == KERNEL
            assert r.last_sky_split() is not None, "the bunny's box is a small part of the frame: the fill ran beside the walks"
            got = b.cpu().numpy().reshape(H, W, 16)
            differing = np.argwhere((got != want).any(axis=2))
            assert differing.size == 0, f"context {k}: {len(differing)} pixels differ, the first at (y, x) = {tuple(differing[0])}"
    finally:
        for r in ctxs:
            r.set_output(None)
            r.set_stream(None)
            r.close()


def test_a_short_verify_sweep_over_generated_scenes_with_meshes(renderer):
    """tools/verify_fuzz.py's generators at 160x90, kernel 41 against the un-culled kernel on the device: the first ten accepted scenes of
    `meshwalls` (always a mesh) and the first ten of `random` that hold a mesh"""
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import verify_fuzz
    W, H = 160, 90
    for kind in ("meshwalls", "random"):
        verified = 0
        for seed in range(200):
            if verified == 10:
                break
            try:
                scene, text = verify_fuzz.build(kind, seed)
            except RuntimeError:         # the front end's rejection of a generated scene
                continue
            if not (np.asarray(scene.objects()["type"]) == 2).any():
                continue
            _setup(renderer, scene, W, H)
            n = renderer.verify_frame()
            assert renderer.last_variant() == KERNEL
            assert n == 0, f"{kind} seed {seed}: kernel {KERNEL} differs from the un-culled kernel on {n} pixels\n{text}"
            verified += 1
        assert verified == 10, f"{kind}: only {verified} scenes with a mesh among seeds 0..199"
    renderer.set_variant(0)
