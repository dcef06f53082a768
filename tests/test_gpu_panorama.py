"""rpt_set_projection on the MI355X: the equirectangular camera's frames bit for bit against the CPU oracle fed the same rays
(tests/native/panorama_oracle.c), aberration where special relativity puts it, the shadow culls, Doppler in panorama, and the plumbing
(DESIGN.md "Panorama camera")."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_ffi
from conftest import CONFIGS, load_config
from relativitypathtracer_amd import Scene
from relativitypathtracer_amd.renderer import RenderError, Renderer, projection_tables
from scene_fuzz import close_scene_text, extreme_scene_text, meshwalls_scene_text, random_scene_text, walls_scene_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "panorama_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's
THREADS = min(16, os.cpu_count() or 1)


@pytest.fixture(scope="module")
def pano_oracle(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build tests/native/panorama_oracle.c")
    so = str(tmp_path_factory.mktemp("pano") / "libpanorama_oracle.so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_panorama_oracle_render.restype = C.c_int
    lib.rpt_panorama_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def pano_dirs(W, H, **kw):
    """(H * W, 3) float32 p of include/rpt.h from the library's own tables, as float32 products."""
    cols, rows = projection_tables(W, H, **kw)
    sl, cl = cols[None, :, 0], cols[None, :, 1]
    sp, cp = rows[:, None, 0], rows[:, None, 1]
    p = np.stack([cp * sl, np.broadcast_to(sp, (H, W)), cp * cl], -1).astype(np.float32)
    return np.ascontiguousarray(p.reshape(-1, 3))


def oracle_render(lib, scene, W, H, dirs):
    d, prm = scene.desc(), scene.params
    a = oracle_ffi.OracleArgs()
    a.objects, a.object_count = d.objects, d.object_count
    a.vertices, a.normals, a.uvs = d.vertices, d.normals, d.uvs
    a.triangles, a.octrees, a.octreeTris = d.triangles, d.octrees, d.octreeTris
    a.textures, a.texture_bytes = d.textures, d.texture_bytes
    a.white_point = (C.c_float * 3)(*prm["white_point"])
    a.ambient, a.width, a.height, a.interval, a.msaa = prm["ambient"], W, H, prm["interval"], 1
    px = np.zeros(W * H, dtype=oracle_ffi.PIXEL_DTYPE)
    rgb = np.zeros((H, W, 3), dtype=np.float32)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    assert lib.rpt_panorama_oracle_render(C.byref(a), dirs.ctypes.data, 0, H, THREADS) == 0
    return px, rgb


def _scene(text, v=(0.0, 0.0, 0.0), t=0.0, interval=None):
    s = Scene()
    s.inputScene(text)
    if interval is not None:
        s.set_interval(interval)
    s.set_camera(v, t)
    s.update_objects()
    return s


def _setup(r, scene, W, H, variant=0, doppler=(False, False), **proj):
    r.set_variant(variant)
    r.set_msaa(1)
    r.set_projection("equirect", **proj)
    r.upload_scene(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_debug_rgb(True)
    r.set_debug_doppler(False)
    r.set_doppler(*doppler)


def _assert_frame(r, lib, scene, W, H, what, **proj):
    px, rgb = r.read_framebuffer(), r.read_debug_rgb()
    opx, orgb = oracle_render(lib, scene, W, H, pano_dirs(W, H, **proj))
    assert np.array_equal(px.view(np.uint8), opx.view(np.uint8)), f"{what}: {np.sum(px['rgba'] != opx['rgba'])} bytes differ"
    assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32)), what


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


# ---- 0. the helper itself (no GPU): with the pinhole's directions it is the oracle ------------------------------------------------
@pytest.mark.parametrize("name", ["shadows", "bunny", "cubes"])
def test_helper_with_pinhole_rays_is_the_oracle(pano_oracle, name):
    W, H = 96, 54
    scene = load_config(name)
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    fx = (x / np.float32(W) - np.float32(0.5)) * (np.float32(W) / np.float32(H))
    fy = y / np.float32(H) - np.float32(0.5)
    dirs = np.ascontiguousarray(np.stack([fx, fy, np.full_like(fx, 0.5)], -1).reshape(-1, 3).astype(np.float32))
    px, rgb = oracle_render(pano_oracle, scene, W, H, dirs)
    opx, orgb, _ = oracle_ffi.render(scene, W, H)
    assert np.array_equal(px.view(np.uint8), opx.view(np.uint8))
    assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32))


# ---- 1. bit-exact against the oracle, ray by ray ------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_configs_equal_the_oracle(renderer, pano_oracle, name):
    W, H = 512, 256
    scene = load_config(name)
    _setup(renderer, scene, W, H)
    renderer.render()
    assert renderer.last_variant() in (341, 344)
    _assert_frame(renderer, pano_oracle, scene, W, H, name)
    renderer.set_variant(3)
    renderer.render()
    assert renderer.last_variant() == 303
    _assert_frame(renderer, pano_oracle, scene, W, H, name + " (303)")


GENERATORS = {"random": lambda rng: random_scene_text(rng)[0], "extreme": extreme_scene_text, "close": close_scene_text,
              "walls": walls_scene_text, "meshwalls": meshwalls_scene_text}


@pytest.mark.gpu
@pytest.mark.parametrize("gen", list(GENERATORS))
def test_fuzzed_scenes_equal_the_oracle(renderer, pano_oracle, gen):
    rng = np.random.default_rng(4242 + len(gen))
    W, H = 256, 128
    for i in range(8):
        scene = _scene(GENERATORS[gen](rng))
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * rng.choice([0.0, 0.5, 0.95])
        scene.set_camera(tuple(float(c) for c in v), float(rng.uniform(-3, 20)))
        scene.update_objects()
        _setup(renderer, scene, W, H)
        renderer.render_async()
        renderer.sync()
        _assert_frame(renderer, pano_oracle, scene, W, H, f"{gen} scene {i}")


@pytest.mark.gpu
@pytest.mark.parametrize("name,proj", [("bunny", dict(h_fov=2.0, v_fov=1.2, yaw=0.0)), ("cubes", dict(h_fov=3.0, v_fov=1.5, yaw=0.7)),
                                       ("shadows", dict(yaw=-2.5)), ("arch", dict(h_fov=1.0, v_fov=0.5, yaw=3.0))])
def test_reduced_field_of_view_and_yaw(renderer, pano_oracle, name, proj):
    W, H = 384, 200
    scene = load_config(name)
    _setup(renderer, scene, W, H, **proj)
    renderer.render()
    _assert_frame(renderer, pano_oracle, scene, W, H, name, **proj)


# ---- 2. aberration ------------------------------------------------------------------------------------------------------------
def _hit_mask(r, scene, W, H):
    px = r.read_framebuffer()["rgba"].reshape(H, W, 4)
    bg = px[0, 0].copy()               # (the scenes below leave the bottom-left corner to the background)
    return np.any(px != bg, axis=-1)


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 0.5, 0.9])
def test_aberration_moves_a_side_source_forward(renderer, beta):
    """The camera passes the origin at beta c along +z; a light sphere at rest at (10, 0, 0) is seen at longitude arccos(beta)."""
    W, H = 2048, 1024
    scene = _scene("Os\n p10,0,0,0,0,1,0,0.3,0.3,0.3\n c1,0.8,0.6\n l1\n v0,0,0\nA0.2\nR\n", v=(0.0, 0.0, beta), t=0.0, interval=-1)
    _setup(renderer, scene, W, H)
    renderer.render()
    hit = _hit_mask(renderer, scene, W, H)
    assert hit.sum() > 20
    lam = np.degrees(2 * math.pi * ((np.arange(W) + 0.5) / W - 0.5))
    ys, xs = np.nonzero(hit)
    got = lam[xs].mean()
    assert abs(got - math.degrees(math.acos(beta))) <= 0.5, (beta, got)
    assert abs(((ys + 0.5) / H - 0.5).mean() * 180) <= 0.5            # on the equator


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.0, 0.9])
def test_a_source_straight_behind_stays_on_the_seam(renderer, beta):
    W, H = 2048, 1024
    scene = _scene("Os\n p0,0,-10,0,0,1,0,0.3,0.3,0.3\n c1,0.8,0.6\n l1\n v0,0,0\nA0.2\nR\n", v=(0.0, 0.0, beta), t=0.0, interval=-1)
    _setup(renderer, scene, W, H)
    renderer.render()
    hit = _hit_mask(renderer, scene, W, H)
    ys, xs = np.nonzero(hit)
    assert hit[:, 0].any() and hit[:, W - 1].any()                   # both sides of the seam
    lam = np.degrees(2 * math.pi * ((xs + 0.5) / W - 0.5))
    # (the rear is magnified by sqrt((1 + beta) / (1 - beta)), small angles about the axis)
    assert np.abs(lam).min() >= 180 - 1.1 * math.degrees(math.asin(0.3 / 10)) * math.sqrt((1 + beta) / (1 - beta)) - 0.5


# ---- 3. the shadow culls --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("gen", list(GENERATORS))
@pytest.mark.parametrize("doppler", [False, True])
def test_verify_frame_in_panorama(renderer, gen, doppler):
    rng = np.random.default_rng(777 + len(gen) + 10 * doppler)
    seen = set()
    for i in range(6):
        scene = _scene(GENERATORS[gen](rng))
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * rng.choice([0.0, 0.5, 0.95])
        scene.set_camera(tuple(float(c) for c in v), float(rng.uniform(-3, 20)))
        scene.update_objects()
        _setup(renderer, scene, 320, 160, doppler=(doppler, doppler))
        assert renderer.verify_frame() == 0, f"{gen} scene {i}"
        seen.add(renderer.last_variant())
    assert seen and seen <= ({541, 544} if doppler else {341, 344})


# ---- 4. Doppler -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["arch", "cubes"])
def test_camera_factor_per_pixel(renderer, name):
    W, H = 256, 128
    scene = load_config(name)
    _setup(renderer, scene, W, H, doppler=(True, True))
    renderer.set_debug_doppler(True)
    renderer.render()
    assert renderer.last_variant() == 540
    rec = renderer.read_debug_doppler()
    hit = rec[..., 0] != 0
    assert hit.sum() > 1000
    p = pano_dirs(W, H).astype(np.float64).reshape(H, W, 3)
    n = p / np.linalg.norm(p, axis=-1, keepdims=True)
    assert (n[..., 2] < 0).any()                                      # backward rays included
    ray = np.concatenate([np.full((H, W, 1), float(scene.params["interval"])), n], axis=-1)
    L0 = scene.objects()["Lorentz"][:, 0, :].astype(np.float64)
    cands = scene.params["interval"] / np.einsum("hwk,ok->hwo", ray, L0)
    rel = np.min(np.abs(cands - rec[..., 0:1].astype(np.float64)) / np.abs(cands), axis=-1)
    assert rel[hit].max() <= 1e-5, rel[hit].max()
    assert np.ptp(rec[..., 0][hit]) > 0.1


@pytest.mark.gpu
@pytest.mark.parametrize("name,interval", [("cubes", 0), ("arch", 0), ("bunny", None), ("cube", None)])
def test_neutral_doppler_equals_the_panorama_frame(renderer, name, interval):
    W, H = 320, 160
    scene = load_config(name)
    if interval is not None:
        scene.set_interval(interval)
        scene.update_objects()
    _setup(renderer, scene, W, H)
    renderer.render()
    plain = renderer.read_framebuffer()
    renderer.set_doppler(True, True)
    renderer.render()
    assert renderer.last_variant() in (541, 544)
    assert np.array_equal(renderer.read_framebuffer().view(np.uint8), plain.view(np.uint8))


# ---- 5. plumbing --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,doppler", [("cubes", False), ("bunny", False), ("cubes", True)])
def test_row_tiles_equal_the_whole_frame(renderer, name, doppler):
    W, H = 320, 184
    scene = load_config(name)
    scene.set_camera((0.3, 0.0, 0.1), 3.0)
    scene.update_objects()
    _setup(renderer, scene, W, H, doppler=(doppler, doppler), yaw=1.0)
    renderer.set_debug_rgb(False)
    renderer.render()
    whole32 = renderer.read_framebuffer()["rgba"].reshape(H, W, 4).copy().view(np.uint32).reshape(H, W)
    tiles = (H + 7) // 8
    for first, step, run in ((0, 3, 1), (1, 3, 1), (2, 3, 1), (0, 5, 2), (1, 4, 4)):
        if run == 1:
            renderer.set_rows(first, step, True)
        else:
            renderer.set_tile_pattern(first, step, run, True)
        renderer.render()
        plane = renderer.read_colour_plane()
        local = [t for t in range(tiles) if (t - first) % step < run and t >= first]
        for k, t in enumerate(local):
            rows = slice(t * 8, min(H, t * 8 + 8))
            assert np.array_equal(plane[k * 8:k * 8 + (rows.stop - rows.start)], whole32[rows]), (first, step, t)


@pytest.mark.gpu
def test_frames_in_flight_equal_blocking_frames():
    W, H = 1024, 512
    scene = load_config("bunny")
    slots = [Renderer(0) for _ in range(3)]
    try:
        slots[0].upload_scene(scene)
        for s in slots[1:]:
            s.share_scene(slots[0])
        for k, s in enumerate(slots):
            s.set_scene_params(scene, W, H)
            s.set_output(None)
            s.set_projection("equirect", yaw=0.1 * k)
        frames = []
        for f in range(3):
            scene.set_camera((0.3, 0.0, 0.1), 3.0 + 0.1 * f)
            scene.update_objects()
            slots[f].set_objects(scene)
            slots[f].render_async()
            assert slots[f].last_variant() == 341
        for s in slots:
            s.sync()
            frames.append(s.read_framebuffer())
        for f in range(3):
            scene.set_camera((0.3, 0.0, 0.1), 3.0 + 0.1 * f)
            scene.update_objects()
            slots[0].set_projection("equirect", yaw=0.1 * f)
            slots[0].set_objects(scene)
            slots[0].render()
            assert slots[0].last_variant() == 341
            assert np.array_equal(slots[0].read_framebuffer().view(np.uint8), frames[f].view(np.uint8)), f
    finally:
        for s in slots:
            s.close()


@pytest.mark.gpu
def test_tables_follow_the_frame_size_and_parameters(renderer, pano_oracle):
    scene = load_config("shadows")
    _setup(renderer, scene, 256, 128)
    renderer.render()
    _assert_frame(renderer, pano_oracle, scene, 256, 128, "first size")
    for W, H, proj in ((384, 160, {}), (200, 100, {}), (200, 100, dict(h_fov=2.5, v_fov=1.0, yaw=-0.5))):
        if proj:
            renderer.set_projection("equirect", **proj)
        renderer.set_params(scene.params["white_point"], scene.params["ambient"], W, H, scene.params["interval"])
        renderer.render_async()          # (queued behind the previous frame, which still reads the old tables)
        renderer.sync()
        _assert_frame(renderer, pano_oracle, scene, W, H, f"{W}x{H} {proj}", **proj)


@pytest.mark.gpu
def test_back_to_pinhole_is_the_reference(renderer):
    W, H = 256, 144
    scene = load_config("bunny")
    _setup(renderer, scene, W, H)
    renderer.render()
    assert renderer.last_variant() == 341
    renderer.set_projection("pinhole")
    renderer.render()
    assert renderer.last_variant() == 43
    px, rgb = renderer.read_framebuffer(), renderer.read_debug_rgb()
    opx, orgb, _ = oracle_ffi.render(scene, W, H)
    assert np.array_equal(px.view(np.uint8), opx.view(np.uint8))
    assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32))
    other = Renderer(0)
    try:
        renderer.set_projection("equirect")
        other.share_scene(renderer)                  # not shared by rpt_share_scene
        other.set_scene_params(scene, W, H)
        other.set_output(None)
        other.render()
        assert other.last_variant() == 43
    finally:
        other.close()


@pytest.mark.gpu
def test_variants_and_refusals(renderer):
    W, H = 256, 128
    bunny, arch = load_config("bunny"), load_config("arch")
    for scene, variant, want, twin in ((bunny, 0, 341, 541), (arch, 0, 344, 544), (bunny, 3, 303, 503), (arch, 3, 303, 503)):
        _setup(renderer, scene, W, H, variant)
        renderer.render()
        assert renderer.last_variant() == want
        assert renderer.last_exact_rcp() == (want == 341)
        renderer.set_doppler(True, True)
        renderer.render_async()
        renderer.sync()
        assert renderer.last_variant() == twin
    for variant in (1, 41, 43, 44, 48, 49, 50, 51):
        _setup(renderer, bunny, W, H, variant)
        with pytest.raises(RenderError, match=r"\(1\).*variant"):
            renderer.render()
        with pytest.raises(RenderError, match=r"\(1\)"):
            renderer.verify_frame()
    _setup(renderer, bunny, W, H)
    renderer.set_msaa(2)
    with pytest.raises(RenderError, match=r"\(1\).*MSAA"):
        renderer.render()
    renderer.set_msaa(1)
    # an octree whose children are not consecutive (test_gpu_properties' construction): no derived layout, no panorama kernel
    from relativitypathtracer_amd import _ffi
    shadows = load_config("shadows")
    oc = shadows.buffers()["octrees"].copy().view(np.int32).reshape(-1, 24)
    root = shadows.mesh_roots()[0]
    new = np.vstack([oc, oc[oc[root, 10]][None]])
    new[root, 10] = len(oc)
    d2 = _ffi.SceneDesc.from_buffer_copy(shadows.desc())
    raw = np.ascontiguousarray(new).view(np.uint8).reshape(-1)
    d2.octrees, d2.octree_count = raw.ctypes.data, len(new)
    renderer.upload_desc(d2)
    renderer.set_scene_params(shadows, W, H)
    with pytest.raises(RenderError, match=r"\(1\).*octree"):
        renderer.render()
    renderer.set_projection("pinhole")
    renderer.render()
    assert renderer.last_variant() == 1
    # the setting itself
    lib, h = renderer._lib, renderer._h
    f3 = lambda *v: (C.c_float * 3)(*v)
    assert lib.rpt_set_projection(h, 0, f3(1, 1, 0)) == 1                  # the pinhole takes no parameters
    assert lib.rpt_set_projection(h, 2, None) == 1
    assert lib.rpt_set_projection(h, 1, f3(7.0, 1.0, 0.0)) == 1
    assert lib.rpt_set_projection(h, 1, f3(1.0, 3.5, 0.0)) == 1
    assert lib.rpt_set_projection(h, 1, f3(1.0, 1.0, math.inf)) == 1
    assert lib.rpt_set_projection(h, 1, None) == 0
    with pytest.raises(ValueError):
        renderer.set_projection("cubemap")
    renderer.set_projection("pinhole")
