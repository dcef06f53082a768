"""rpt_set_environment on the MI355X: the sky lookup and whole frames bit for bit against a C restatement on the CPU oracle
(tests/native/environment_oracle.c), off-means-off, aberration and beaming of the sky where special relativity puts them, the culls,
the plumbing and the refusals (DESIGN.md "Environment map")."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import doppler_model as dm
import oracle_ffi
from conftest import CONFIGS, load_config
from relativitypathtracer_amd import Scene
from relativitypathtracer_amd.renderer import RenderError, Renderer, projection_tables
from scene_fuzz import close_scene_text, extreme_scene_text, meshwalls_scene_text, random_scene_text, walls_scene_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "environment_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's
THREADS = min(16, os.cpu_count() or 1)
OBLIQUE = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
CAMERAS = {"rest": (0.0, 0.0, 0.0), "0.5c+z": (0.0, 0.0, 0.5), "0.95c+z": (0.0, 0.0, 0.95),
           "0.95c-oblique": tuple(float(c) for c in 0.95 * OBLIQUE)}
REDUCED = dict(h_fov=2.0, v_fov=1.2, yaw=0.0)


@pytest.fixture(scope="module")
def env_oracle(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build tests/native/environment_oracle.c")
    so = str(tmp_path_factory.mktemp("env") / "libenvironment_oracle.so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_environment_oracle_render.restype = C.c_int
    lib.rpt_environment_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                  C.c_int, C.c_void_p, C.c_int]
    lib.rpt_environment_oracle_lookup.restype = C.c_int
    lib.rpt_environment_oracle_lookup.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    return lib


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


def sky_image(W, H, seed=1):
    """A smooth gradient plus a few one-texel markers (one of them on the wrap column, one in each pole row)."""
    y, x = np.mgrid[0:H, 0:W]
    img = np.stack([(40 + 180 * x / max(W - 1, 1)), (30 + 200 * y / max(H - 1, 1)), (220 - 150 * ((x + y) % max(W, 2)) / max(W, 2))], -1)
    img = img.astype(np.uint8)
    rng = np.random.default_rng(seed)
    for k in range(6):
        img[rng.integers(0, H), rng.integers(0, W)] = (255, 255 * (k & 1), 0)
    img[H // 2, 0] = (0, 255, 255)
    img[H // 3, W - 1] = (255, 0, 255)
    img[0, W // 2] = (255, 255, 255)
    img[H - 1, W // 4] = (0, 0, 0)
    return np.ascontiguousarray(img)


def pinhole_dirs(W, H):
    """The plane point createCamRay normalises, in its float32 operations."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    fx = (x / np.float32(W) - np.float32(0.5)) * (np.float32(W) / np.float32(H))
    fy = y / np.float32(H) - np.float32(0.5)
    return np.ascontiguousarray(np.stack([fx, fy, np.full_like(fx, 0.5)], -1).reshape(-1, 3).astype(np.float32))


def pano_dirs(W, H, **kw):
    cols, rows = projection_tables(W, H, **kw)
    sl, cl = cols[None, :, 0], cols[None, :, 1]
    sp, cp = rows[:, None, 0], rows[:, None, 1]
    p = np.stack([cp * sl, np.broadcast_to(sp, (H, W)), cp * cl], -1).astype(np.float32)
    return np.ascontiguousarray(p.reshape(-1, 3))


def oracle_frame(lib, scene, W, H, dirs, E, img, flags):
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
    hit = np.zeros(W * H, dtype=np.uint8)
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    E = np.ascontiguousarray(E, dtype=np.float32)
    img = np.ascontiguousarray(img)
    assert lib.rpt_environment_oracle_render(C.byref(a), dirs.ctypes.data, E.ctypes.data, img.ctypes.data, img.shape[1], img.shape[0],
                                             int(flags), hit.ctypes.data, THREADS) == 0
    return px, rgb, hit.astype(bool)


def _scene(text, v=(0.0, 0.0, 0.0), t=0.0, interval=None):
    s = Scene()
    s.inputScene(text)
    if interval is not None:
        s.set_interval(interval)
    s.set_camera(v, t)
    s.update_objects()
    return s


def _setup(r, scene, W, H, variant=0, flags=0, proj=None, upload=True):
    r.set_variant(variant)
    r.set_msaa(1)
    if proj is None:
        r.set_projection("pinhole")
    else:
        r.set_projection("equirect", **proj)
    if upload:
        r.upload_scene(scene)
    else:
        r.set_objects(scene)
    r.set_scene_params(scene, W, H)
    r.set_rows(0, 1, False)
    r.set_plane_output(None)
    r.set_output(None)
    r.set_debug_rgb(True)
    r.set_debug_doppler(False)
    r.set_doppler(bool(flags & 1), bool(flags & 2))


def _frame(r):
    r.render()
    return r.read_framebuffer().copy(), r.read_debug_rgb().copy()


def _check_frame(r, lib, scene, W, H, img, flags, proj, what):
    """One frame with the sky against the oracle: every sky pixel bit for bit (floats and packed); every hit pixel equal to the frame
    WITHOUT the sky (the same Doppler flags); and the whole frame, hit pixels included, with Doppler off and on (with Doppler on the
    reference's hit pixels are tests/native/doppler_oracle.c's trace_doppler)."""
    E = scene.camera_lorentz()[1]
    dirs = pinhole_dirs(W, H) if proj is None else pano_dirs(W, H, **proj)
    r.set_environment(None)
    px0, rgb0 = _frame(r)
    plain_variant = r.last_variant()
    r.set_environment(img)
    r.set_environment_frame(E)
    px, rgb = _frame(r)
    assert r.last_variant() in (603, 641, 643, 644, 703, 741, 744), what
    opx, orgb, hit = oracle_frame(lib, scene, W, H, dirs, E, img, flags)
    sky = ~hit
    h2 = hit.reshape(H, W)
    assert np.array_equal(rgb.view(np.uint32)[~h2], orgb.view(np.uint32)[~h2]), f"{what}: sky floats differ"
    assert np.array_equal(px.view(np.uint8).reshape(-1, 16)[sky], opx.view(np.uint8).reshape(-1, 16)[sky]), f"{what}: sky pixels differ"
    assert np.array_equal(rgb.view(np.uint32)[h2], rgb0.view(np.uint32)[h2]), f"{what}: a hit pixel changed with the sky"
    assert np.array_equal(px.view(np.uint8).reshape(-1, 16)[hit], px0.view(np.uint8).reshape(-1, 16)[hit]), what
    assert np.array_equal(px.view(np.uint8), opx.view(np.uint8)), f"{what}: {int((px['rgba'] != opx['rgba']).any(axis=1).sum())} pixels differ"
    assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32)), what
    return hit, plain_variant


# ---- 0. the helper itself (no GPU) ----------------------------------------------------------------------------------------------
def test_helper_hit_pixels_are_the_oracle(env_oracle):
    W, H = 96, 54
    scene = load_config("shadows")
    img = sky_image(32, 16)
    px, rgb, hit = oracle_frame(env_oracle, scene, W, H, pinhole_dirs(W, H), np.eye(4), img, 0)
    opx, orgb, _ = oracle_ffi.render(scene, W, H)
    assert 0 < hit.sum() < W * H
    assert np.array_equal(px.view(np.uint8).reshape(-1, 16)[hit], opx.view(np.uint8).reshape(-1, 16)[hit])
    assert np.array_equal(rgb.view(np.uint32)[hit.reshape(H, W)], orgb.view(np.uint32)[hit.reshape(H, W)])
    bg = opx["rgba"][~hit]
    assert (bg == bg[0]).all() and (px["rgba"][~hit] != bg[0]).any()


def test_helper_lookup_known_answers(env_oracle):
    """Texel (x, y) is returned unfiltered at u = x / W, v = 1 - y / H; the column neighbour wraps, the row neighbour clamps; u = 1/2 is +x
    and u = 3/4 is +z."""
    W, H = 8, 4
    img = sky_image(W, H)
    out = np.zeros((4, 5), dtype=np.float32)
    d = np.array([[-1, 0, 0], [1, 0, 0], [0, 1, 0], [0, -1, 0]], dtype=np.float32)
    assert env_oracle.rpt_environment_oracle_lookup(d.ctypes.data, 4, img.ctypes.data, W, H, out.ctypes.data) == 0
    assert out[0, 0] == 1.0 and out[0, 1] == 0.5          # -x: atan2(0, -1) = pi -> u = 1: column W - 1 weight 0, wraps to column 0 weight 1
    assert np.array_equal(out[0, 2:], (img[2, 0] / np.float32(255)).astype(np.float32))
    assert out[1, 0] == 0.5                                # +x: the middle column
    assert np.array_equal(out[1, 2:], (img[2, 4] / np.float32(255)).astype(np.float32))
    assert out[2, 1] == 1.0 and np.array_equal(out[2, 2:], (img[0, 4] / np.float32(255)).astype(np.float32))      # +y: the top row
    assert abs(out[3, 1]) < 1e-7 and np.array_equal(out[3, 2:], (img[3, 4] / np.float32(255)).astype(np.float32))      # -y ((float)(pi/2) / pi > 1/2 by 1.4e-8): v = H clamps to the last row
    # +-z, which tell the image from its mirror: u = 3/4 is +z (column 6 of 8), u = 1/4 is -z (column 2), each texel unfiltered
    out = np.zeros((2, 5), dtype=np.float32)
    d = np.array([[0, 0, 1], [0, 0, -1]], dtype=np.float32)
    assert env_oracle.rpt_environment_oracle_lookup(d.ctypes.data, 2, img.ctypes.data, W, H, out.ctypes.data) == 0
    assert out[0, 0] == 0.75 and out[0, 1] == 0.5 and out[1, 0] == 0.25 and out[1, 1] == 0.5
    assert np.array_equal(out[0, 2:], (img[2, 6] / np.float32(255)).astype(np.float32))
    assert np.array_equal(out[1, 2:], (img[2, 2] / np.float32(255)).astype(np.float32))
    assert not np.array_equal(img[2, 6], img[2, 2])


# ---- 1. the lookup, bit for bit ----------------------------------------------------------------------------------------------
def _kat_directions(W, H, rng, n_random):
    special = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1], [0, 0, 0], [-1, 1e-30, 0], [-1, -1e-30, 0],
               [-1, 0, 1e-30], [-1, 0, -1e-30], [-1, 0, -0.0], [-1, 0, 1e-7], [-1, 0, -1e-7],
               [1e-40, 0, 0], [0, 1e-40, 1e-42], [1e-39, -1e-40, 1e-41], [3e38, 1, 1], [1, -3e38, 3e38], [3e38, 3e38, 3e38],
               [1e-20, 1e20, 1e-20], [1e20, 1e-20, -1e20], [np.inf, 0, 0], [0, np.nan, 1]]
    us, vs = [], []
    for k in range(-1, W + 2):
        for off in (0.0, 0.5):
            u = np.float32((k + off) / W)
            us += [u, np.nextafter(u, np.float32(-1)), np.nextafter(u, np.float32(2))]
    for k in range(-1, H + 2):
        for off in (0.0, 0.5):
            v = np.float32((k + off) / H)
            vs += [v, np.nextafter(v, np.float32(-1)), np.nextafter(v, np.float32(2))]
    uu, vv = np.meshgrid(np.array(us, dtype=np.float64), np.array(vs, dtype=np.float64))
    az, lat = 2 * np.pi * (uu.ravel() - 0.5), np.pi * (np.clip(vv.ravel(), 0, 1) - 0.5)
    grid = np.stack([np.cos(lat) * np.cos(az), np.sin(lat), np.cos(lat) * np.sin(az)], -1)
    rnd = rng.normal(size=(n_random, 3)) * np.exp(rng.uniform(-20, 20, size=(n_random, 1)))
    near_seam = np.stack([-np.ones(4096), rng.uniform(-1, 1, 4096), rng.normal(size=4096) * 1e-6], -1)
    with np.errstate(all="ignore"):
        return np.ascontiguousarray(np.concatenate([np.array(special, dtype=np.float64), grid, near_seam, rnd]).astype(np.float32))


def _same_bits(a, b):
    """Bit for bit, except that any NaN equals any NaN (a NaN's sign and payload are the platform's, not the model's)."""
    nan = np.isnan(a) & np.isnan(b)
    return bool(np.all((a.view(np.uint32) == b.view(np.uint32)) | nan))


@pytest.mark.gpu
@pytest.mark.parametrize("size", [(64, 32), (1, 1), (1, 9), (9, 1), (37, 23)])
def test_lookup_equals_the_restatement(renderer, env_oracle, size):
    W, H = size
    img = sky_image(W, H, seed=W + H)
    rng = np.random.default_rng(99 + W)
    d = _kat_directions(W, H, rng, 1_000_000 if size == (64, 32) else 100_000)
    renderer.set_environment(img)
    got = renderer.probe(7, d, 5)
    want = np.zeros_like(got)
    assert env_oracle.rpt_environment_oracle_lookup(d.ctypes.data, len(d), img.ctypes.data, W, H, want.ctypes.data) == 0
    bad = ~((got.view(np.uint32) == want.view(np.uint32)) | (np.isnan(got) & np.isnan(want))).all(axis=1)
    assert not bad.any(), (int(bad.sum()), d[bad][:5], got[bad][:5], want[bad][:5])
    finite = np.isfinite(want).all(axis=1)
    assert finite.sum() > 0.99 * len(d)
    # (u at atan2 = -(float)pi and v at asin = -(float)(pi/2) are -1.4e-8, not 0, the float pi's excess over pi: the indices clamp)
    assert (want[finite, 0] >= -2e-8).all() and (want[finite, 0] <= 1).all() and (want[finite, 1] >= -2e-8).all() and (want[finite, 1] <= 1).all()
    renderer.set_environment(None)
    with pytest.raises(RenderError, match=r"\(2\)"):          # RPT_ERR_STATE without an environment
        renderer.probe(7, d[:4], 5)


# ---- 2. frames, bit for bit ---------------------------------------------------------------------------------------------------
def _allsky_scene(camera, interval):
    """One small sphere straight behind the camera's motion (behind the view at rest): aberration keeps it there, every pixel is sky."""
    v = np.array(CAMERAS[camera])
    back = -v / np.linalg.norm(v) if v.any() else np.array([0.0, 0.0, -1.0])
    p = 10 * back
    return _scene(f"Os\n p{p[0]},{p[1]},{p[2]},0,0,1,0,0.3,0.3,0.3\n c1,0.8,0.6\n l1\n v0,0,0\nA0.2\nR\n", v=CAMERAS[camera], t=0.0, interval=interval)


@pytest.mark.gpu
@pytest.mark.parametrize("camera", list(CAMERAS))
@pytest.mark.parametrize("proj", ["pinhole", "equirect"])
@pytest.mark.parametrize("name", ["arch", "bunny", "allsky"])
def test_frames_equal_the_oracle(renderer, env_oracle, name, proj, camera):
    W, H = (192, 96) if proj == "equirect" else (160, 96)
    img = sky_image(128, 64)
    for interval in (-1, 0):
        if name == "allsky":
            scene = _allsky_scene(camera, interval)
        else:
            scene = load_config(name)
            scene.set_interval(interval)
            scene.set_camera(CAMERAS[camera], CONFIGS[name]["t"])
            scene.update_objects()
        p = None if proj == "pinhole" else (REDUCED if name == "allsky" else {})
        for flags in (0, dm.SHIFT, dm.BEAMING, dm.SHIFT | dm.BEAMING):
            _setup(renderer, scene, W, H, flags=flags, proj=p, upload=(flags == 0))
            hit, _ = _check_frame(renderer, env_oracle, scene, W, H, img, flags, p, f"{name} {proj} {camera} interval {interval} flags {flags}")
            if name == "allsky":
                assert not hit.any()
            elif proj == "pinhole" and camera == "rest":
                assert 0 < hit.sum() < W * H
    renderer.set_environment(None)


@pytest.mark.gpu
def test_full_hd_pinhole_frame(renderer, env_oracle):
    W, H = 1920, 1080
    scene = load_config("arch")
    img = sky_image(512, 256)
    _setup(renderer, scene, W, H, flags=3)
    hit, _ = _check_frame(renderer, env_oracle, scene, W, H, img, 3, None, "arch 1920x1080 0.95c shift + beaming")
    assert 0 < hit.sum() < W * H
    renderer.set_environment(None)


@pytest.mark.gpu
def test_identity_frame_is_a_plain_lookup_of_the_camera_direction(renderer, env_oracle):
    """E the exact identity, Doppler off: the sky pixel is the lookup (rpt_probe 7) of the pixel's direction, tonemapped."""
    W, H = 128, 64
    scene = _allsky_scene("rest", -1)
    img = sky_image(64, 32)
    _setup(renderer, scene, W, H, proj=REDUCED)          # (the scene's one sphere is behind this field of view)
    renderer.set_environment(img)
    renderer.set_environment_frame(None)
    _, rgb = _frame(renderer)
    def normalize32(v):                                  # the kernels' normalize in float32: sqrt((x x + y y) + z z), three divisions
        length = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
        return (v / length[:, None]).astype(np.float32)
    n = normalize32(normalize32(pano_dirs(W, H, **REDUCED)))          # the camera's normalize, then trace()'s; the lookup normalises E n again
    look = renderer.probe(7, n, 5)[:, 2:].astype(np.float32)
    A, B, Cc, D, E, F = (np.float32(x) for x in (0.15, 0.50, 0.10, 0.20, 0.02, 0.30))
    hable = lambda x: ((x * (A * x + Cc * B) + D * E) / (x * (A * x + B) + D * F)) - E / F
    wp = np.array(scene.params["white_point"], dtype=np.float32)
    want = np.minimum(hable(look) / hable(wp), np.float32(1)).astype(np.float32)
    assert np.array_equal(rgb.reshape(-1, 3).view(np.uint32), want.view(np.uint32))
    renderer.set_environment(None)


# ---- 3. off means off ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", ["bunny", "arch", "shadows"])
def test_switched_off_is_a_context_that_never_had_one(renderer, name):
    W, H = 256, 144
    scene = load_config(name)
    fresh = Renderer(0)
    try:
        for blocking in (True, False):
            frames = []
            for r in (fresh, renderer):
                _setup(r, scene, W, H)
                if r is renderer:
                    r.set_environment(sky_image(64, 32))
                    r.set_environment_frame(scene.camera_lorentz()[1])
                    r.render()
                    assert r.last_variant() in (641, 643, 644)
                    r.set_environment(None)
                if blocking:
                    r.render()
                else:
                    r.render_async()
                    r.sync()
                frames.append((r.read_framebuffer().copy(), r.read_debug_rgb().copy(), r.last_variant(), r.last_exact_rcp()))
            assert frames[0][2:] == frames[1][2:] and frames[0][2] in (41, 43, 44)
            assert np.array_equal(frames[0][0].view(np.uint8), frames[1][0].view(np.uint8))
            assert np.array_equal(frames[0][1].view(np.uint32), frames[1][1].view(np.uint32))
        # not shared by rpt_share_scene
        renderer.set_environment(sky_image(64, 32))
        fresh.share_scene(renderer)
        fresh.render()
        assert fresh.last_variant() in (41, 43, 44)
    finally:
        fresh.close()
        renderer.set_environment(None)


# ---- 4. physics on the device -------------------------------------------------------------------------------------------------
def _texel_directions(W, H):
    """The direction at which texel (x, y) is returned unfiltered: u = x / W, v = 1 - y / H (no half-texel offset in the reference's fetch)."""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    az, lat = 2 * np.pi * (x / W - 0.5), np.pi * (0.5 - y / H)
    return np.stack([np.cos(lat) * np.cos(az), np.sin(lat), np.cos(lat) * np.sin(az)], -1)


@pytest.mark.gpu
@pytest.mark.parametrize("beta,theta_sky", [(0.5, 90.0), (0.9, 90.0), (0.9, 140.0), (0.0, 60.0)])
def test_a_ring_of_sky_is_seen_where_aberration_puts_it(renderer, beta, theta_sky):
    """Camera at beta along +z; a bright ring at polar angle theta' from +z in the sky's frame is seen at theta with
    cos theta = (cos theta' + beta) / (1 + beta cos theta').
    Margin, one pixel pitch of the frame (2 pi / W): the ring is 3 texels wide and symmetric about theta' (half a texel pitch of
    quantisation in where its middle lies), the four-tap filter widens it by at most one texel on either side, symmetrically, and the
    brightness-weighted mean of the pixels' own polar angles samples it at pixel centres (half a pixel pitch at most).  The image has
    two texels per frame pixel and the sky is magnified by m = d theta / d theta' = sqrt(1 - beta^2) / (1 + beta cos theta') <= 1.41 in
    the cases here, so the texel quantisation is 0.25 m <= 0.36 pitch and the symmetric filter shifts nothing to first order: under
    one pitch in all."""
    W, H, TW, TH = 512, 256, 1024, 512
    d = _texel_directions(TW, TH)
    polar = np.degrees(np.arccos(np.clip(d[..., 2], -1, 1)))
    img = np.full((TH, TW, 3), 10, dtype=np.uint8)
    img[np.abs(polar - theta_sky) <= 1.5 * 180.0 / TH] = 250
    scene = _allsky_scene("rest", -1)
    scene.set_camera((0.0, 0.0, beta), 0.0)
    scene.update_objects()
    _setup(renderer, scene, W, H, proj={})
    renderer.set_environment(img)
    renderer.set_environment_frame(scene.camera_lorentz()[1])
    _, rgb = _frame(renderer)
    p = pano_dirs(W, H).astype(np.float64)
    n = p / np.linalg.norm(p, axis=1, keepdims=True)
    theta_pix = np.degrees(np.arccos(np.clip(n[:, 2], -1, 1)))
    lum = rgb.reshape(-1, 3).astype(np.float64).sum(axis=1)
    # the scene's one sphere sits straight behind (180 degrees, a few degrees wide once magnified): it must not count
    away = theta_pix < 165
    w = np.clip(lum - np.median(lum[away]), 0, None)
    keep = away & (w > 0.5 * w[away].max())
    assert keep.sum() > 50
    seen = float((w[keep] * theta_pix[keep]).sum() / w[keep].sum())
    b32 = float(np.float32(beta))
    c = math.cos(math.radians(theta_sky))
    want = math.degrees(math.acos((c + b32) / (1 + b32 * c)))
    assert abs(seen - want) <= 360.0 / W, (beta, theta_sky, seen, want)
    renderer.set_environment(None)


@pytest.mark.gpu
@pytest.mark.parametrize("beta", [0.2, 0.5])
def test_beaming_brightens_the_sky_ahead_by_the_models_factor(renderer, env_oracle, beta):
    W, H = 256, 128
    grey = 20
    img = np.full((16, 32, 3), grey, dtype=np.uint8)
    scene = _allsky_scene("rest", -1)
    scene.set_camera((0.0, 0.0, beta), 0.0)
    scene.update_objects()
    flags = dm.SHIFT | dm.BEAMING
    p = dict(h_fov=2 * math.pi, v_fov=1.0, yaw=0.0)             # (a band about the equator: the sphere behind covers the seam columns only)
    _setup(renderer, scene, W, H, flags=flags, proj=p)
    E = scene.camera_lorentz()[1]
    renderer.set_environment(img)
    renderer.set_environment_frame(E)
    _, rgb = _frame(renderer)
    _, orgb, hit = oracle_frame(env_oracle, scene, W, H, pano_dirs(W, H, **p), E, img, flags)
    fwd, rear = (H // 2, W // 2), (H // 2, 8)                   # looking along +z; and 8 columns from the seam, 168 degrees round
    assert not hit.reshape(H, W)[fwd] and not hit.reshape(H, W)[rear]
    assert np.array_equal(rgb[fwd].view(np.uint32), orgb[fwd].view(np.uint32))
    assert np.array_equal(rgb[rear].view(np.uint32), orgb[rear].view(np.uint32))
    # the model in float64 on the same matrix: D = interval / (E (interval, n)).t, S_f, the tonemap
    dirs = pano_dirs(W, H, **p).astype(np.float64).reshape(H, W, 3)
    hable = lambda x: ((x * (0.15 * x + 0.05) + 0.004) / (x * (0.15 * x + 0.5) + 0.06)) - 0.02 / 0.3
    wp = np.array(scene.params["white_point"], dtype=np.float64)
    vals = {}
    for key, at in (("fwd", fwd), ("rear", rear)):
        nrm = dirs[at] / np.linalg.norm(dirs[at])
        k = E.astype(np.float64) @ np.array([-1.0, *nrm])
        D = -1.0 / k[0]
        c = dm.S64(np.array([D]), np.full((1, 3), np.float32(grey) / np.float32(255), dtype=np.float64), flags)[0]
        vals[key] = (D, np.minimum(hable(c) / hable(wp), 1.0))
        assert np.allclose(rgb[at], vals[key][1], rtol=2e-4, atol=2e-6), (key, rgb[at], vals[key])
    b32 = float(np.float32(beta))
    assert vals["fwd"][0] == pytest.approx(math.sqrt((1 + b32) / (1 - b32)), rel=1e-3)
    assert vals["rear"][0] < 1 < vals["fwd"][0]
    assert rgb[fwd].sum() > rgb[rear].sum() and (vals["fwd"][1] < 1).all()      # (per channel the shift moves light between channels)
    renderer.set_environment(None)


# ---- 5. the culls --------------------------------------------------------------------------------------------------------------
GENERATORS = {"random": lambda rng: random_scene_text(rng)[0], "extreme": extreme_scene_text, "close": close_scene_text,
              "walls": walls_scene_text, "meshwalls": meshwalls_scene_text}
COMBOS = [(None, 0), (None, 3), ({}, 0), ({}, 3)]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CONFIGS))
def test_verify_frame_on_the_shipped_scenes(renderer, name):
    scene = load_config(name)
    img = sky_image(64, 32)
    for proj, flags in COMBOS:
        _setup(renderer, scene, 320, 160, flags=flags, proj=proj, upload=(proj is None and flags == 0))
        renderer.set_environment(img)
        renderer.set_environment_frame(scene.camera_lorentz()[1])
        assert renderer.verify_frame() == 0, (name, proj, flags)
        assert renderer.last_variant() in ((641, 643, 644) if proj is None else (741, 744))
    renderer.set_environment(None)


@pytest.mark.gpu
@pytest.mark.parametrize("gen", list(GENERATORS))
def test_verify_frame_on_fuzzed_scenes(renderer, gen):
    """40 scenes per generator (200 in all), each in pinhole and panorama with Doppler off and on."""
    rng = np.random.default_rng(1234 + len(gen))
    img = sky_image(64, 32)
    seen = set()
    for i in range(40):
        scene = _scene(GENERATORS[gen](rng))
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * rng.choice([0.0, 0.5, 0.95])
        scene.set_camera(tuple(float(c) for c in v), float(rng.uniform(-3, 20)))
        scene.update_objects()
        for proj, flags in COMBOS:
            _setup(renderer, scene, 256, 128, flags=flags, proj=proj, upload=(proj is None and flags == 0))
            renderer.set_environment(img)
            renderer.set_environment_frame(scene.camera_lorentz()[1])
            assert renderer.verify_frame() == 0, f"{gen} scene {i} {proj} {flags}"
            seen.add(renderer.last_variant())
    assert seen and seen <= {641, 643, 644, 741, 744}
    renderer.set_environment(None)


# ---- 6. plumbing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name,proj,flags", [("bunny", None, 0), ("cubes", None, 3), ("bunny", {}, 0), ("arch", {}, 3)])
def test_row_tiles_equal_the_whole_frame(renderer, name, proj, flags):
    W, H = 320, 184
    scene = load_config(name)
    scene.set_camera((0.3, 0.0, 0.1), 3.0)
    scene.update_objects()
    _setup(renderer, scene, W, H, flags=flags, proj=proj)
    renderer.set_environment(sky_image(96, 48))
    renderer.set_environment_frame(scene.camera_lorentz()[1])
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
    renderer.set_rows(0, 1, False)
    renderer.set_environment(None)


@pytest.mark.gpu
def test_four_contexts_in_flight_each_with_its_own_sky(env_oracle):
    W, H = 512, 288
    scene = load_config("bunny")
    imgs = [sky_image(64 + 16 * k, 32 + 8 * k, seed=k) for k in range(4)]
    cams = [(0.0, 0.0, 0.0), (0.0, 0.0, 0.5), (0.3, 0.0, 0.1), tuple(float(c) for c in 0.95 * OBLIQUE)]
    slots = [Renderer(0) for _ in range(4)]
    try:
        slots[0].upload_scene(scene)
        for s in slots[1:]:
            s.share_scene(slots[0])
        for k, s in enumerate(slots):
            s.set_scene_params(scene, W, H)
            s.set_output(None)
            s.set_debug_rgb(True)
            s.set_environment(imgs[k])
        frames = []
        for rounds in range(2):              # the second round launches on top of the first: matrices are launch arguments
            for k, s in enumerate(slots):
                scene.set_camera(cams[(k + rounds) % 4], 0.0)
                scene.update_objects()
                s.set_objects(scene)
                s.set_environment_frame(scene.camera_lorentz()[1])
                s.render_async()
                assert s.last_variant() in (641, 643)
        for s in slots:
            s.sync()
            frames.append((s.read_framebuffer().copy(), s.read_debug_rgb().copy()))
        for k in range(4):
            scene.set_camera(cams[(k + 1) % 4], 0.0)
            scene.update_objects()
            E = scene.camera_lorentz()[1]
            opx, orgb, _ = oracle_frame(env_oracle, scene, W, H, pinhole_dirs(W, H), E, imgs[k], 0)
            assert np.array_equal(frames[k][0].view(np.uint8), opx.view(np.uint8)), k
            assert np.array_equal(frames[k][1].view(np.uint32), orgb.view(np.uint32)), k
    finally:
        for s in slots:
            s.close()


@pytest.mark.gpu
def test_replacing_the_image_between_frames_in_flight(renderer, env_oracle):
    W, H = 640, 360
    scene = load_config("bunny")
    scene.set_camera((0.0, 0.0, 0.5), 0.0)
    scene.update_objects()
    E = scene.camera_lorentz()[1]
    _setup(renderer, scene, W, H)
    renderer.set_environment_frame(E)
    sizes = [(64, 32), (256, 128), (32, 16), (256, 128), (1, 1)]          # growing (a new buffer), shrinking and same-size replacements
    outs = []
    import torch
    bufs = [torch.empty(W * H * 16, dtype=torch.uint8, device="cuda:0") for _ in sizes]
    for k, (tw, th) in enumerate(sizes):
        renderer.set_environment(sky_image(tw, th, seed=k))
        renderer.set_output(bufs[k].data_ptr())
        renderer.render_async()             # (queued behind the previous frame, which still reads the previous image)
        if k == 2:
            renderer.set_environment(None)  # switched off and on again while frames are in flight
            renderer.set_environment(sky_image(tw, th, seed=k))
    renderer.sync()
    for k, (tw, th) in enumerate(sizes):
        got = bufs[k].cpu().numpy()
        opx, _, _ = oracle_frame(env_oracle, scene, W, H, pinhole_dirs(W, H), E, sky_image(tw, th, seed=k), 0)
        assert np.array_equal(got, opx.view(np.uint8).reshape(-1)), k
    renderer.set_output(None)
    renderer.set_environment(None)


@pytest.mark.gpu
def test_render_scene_takes_an_environment(env_oracle):
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 160, 96
    scene = load_config("cubes")
    img = sky_image(64, 32)
    px, rgb = render_scene(scene, W, H, debug_rgb=True, environment=img)
    opx, orgb, _ = oracle_frame(env_oracle, scene, W, H, pinhole_dirs(W, H), scene.camera_lorentz()[1], img, 0)
    assert np.array_equal(px.view(np.uint8), opx.view(np.uint8))
    assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32))


# ---- 7. refusals ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_variants_and_refusals(renderer):
    W, H = 256, 128
    bunny, arch = load_config("bunny"), load_config("arch")
    img = sky_image(64, 32)
    for scene, variant, proj, want in ((bunny, 0, None, 643), (arch, 0, None, 644), (bunny, 3, None, 603), (bunny, 41, None, 641),
                                       (bunny, 43, None, 643), (arch, 44, None, 644), (bunny, 44, None, 641),
                                       (bunny, 0, {}, 741), (arch, 0, {}, 744), (bunny, 3, {}, 703)):
        for flags in (0, 3):
            _setup(renderer, scene, W, H, variant, flags=flags, proj=proj)
            renderer.set_environment(img)
            renderer.render()
            assert renderer.last_variant() == want, (variant, proj, flags)
            assert renderer.last_exact_rcp() == (want in (641, 643, 741))
    _setup(renderer, bunny, W, H)
    renderer.set_environment(img)
    renderer.render_async()
    renderer.sync()
    assert renderer.last_variant() == 643         # (a small frame in flight waits for latency too, as 43 does)
    for variant in (1, 48, 49, 50, 51):
        _setup(renderer, bunny, W, H, variant)
        with pytest.raises(RenderError, match=r"\(1\).*variant"):
            renderer.render()
        with pytest.raises(RenderError, match=r"\(1\)"):
            renderer.verify_frame()
        renderer.set_environment(None)
        renderer.render()                          # the context is usable: without the sky the variant renders
        renderer.set_environment(img)
    _setup(renderer, bunny, W, H)
    renderer.set_msaa(2)
    with pytest.raises(RenderError, match=r"\(1\).*MSAA"):
        renderer.render()
    renderer.set_msaa(1)
    renderer.render()
    for proj in (None, {}):                        # the Doppler debug-record kernels, 240 and 540
        _setup(renderer, bunny, W, H, flags=3, proj=proj)
        renderer.set_debug_doppler(True)
        with pytest.raises(RenderError, match=r"\(1\).*debug"):
            renderer.render()
        renderer.set_debug_doppler(False)
        renderer.render()
        assert renderer.last_variant() == (643 if proj is None else 741)
    # an octree whose children are not consecutive (test_gpu_properties' construction): no derived layout, no environment kernel
    from relativitypathtracer_amd import _ffi
    shadows = load_config("shadows")
    oc = shadows.buffers()["octrees"].copy().view(np.int32).reshape(-1, 24)
    root = shadows.mesh_roots()[0]
    new = np.vstack([oc, oc[oc[root, 10]][None]])
    new[root, 10] = len(oc)
    d2 = _ffi.SceneDesc.from_buffer_copy(shadows.desc())
    raw = np.ascontiguousarray(new).view(np.uint8).reshape(-1)
    d2.octrees, d2.octree_count = raw.ctypes.data, len(new)
    _setup(renderer, shadows, W, H)
    renderer.upload_desc(d2)
    renderer.set_scene_params(shadows, W, H)
    with pytest.raises(RenderError, match=r"\(1\).*octree"):
        renderer.render()
    renderer.set_environment(None)
    renderer.render()
    assert renderer.last_variant() == 1
    # the settings themselves
    lib, h = renderer._lib, renderer._h
    buf = np.zeros(12, dtype=np.uint8)
    assert lib.rpt_set_environment(h, buf.ctypes.data, 0, 1) == 1
    assert lib.rpt_set_environment(h, buf.ctypes.data, 1, 0) == 1
    assert lib.rpt_set_environment(h, buf.ctypes.data, 1 << 15, 1 << 15) == 1        # 3 W H >= 2^31
    assert lib.rpt_set_environment(h, buf.ctypes.data, 26755, 26755) == 1            # 3 * 26755^2 = 2^31 + 4427
    assert lib.rpt_set_environment(h, buf.ctypes.data, 2, 2) == 0
    m = np.eye(4, dtype=np.float32)
    for bad in (np.nan, np.inf, -np.inf):
        m2 = m.copy()
        m2[2, 1] = bad
        with pytest.raises(RenderError, match=r"\(1\)"):
            renderer.set_environment_frame(m2)
    renderer.set_environment_frame(m)
    renderer.set_environment_frame(None)
    with pytest.raises(ValueError):
        renderer.set_environment(np.zeros((4, 4), dtype=np.uint8))
    renderer.set_environment(None)
