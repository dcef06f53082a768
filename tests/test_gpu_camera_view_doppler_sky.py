"""Doppler and the sky under the free-look camera on the MI355X, held to references outside the library: every shipped scene x the four
views of tests/test_gpu_camera_view.py (a look-back, a pitch-up with roll, a zoom below 20 degrees, a lens above 90 degrees) x camera at
rest and at 0.9c x light propagation on and off, through the blocking call, 41's form in flight and the un-culled kernel.

* the sky: tests/native/environment_oracle.c, as it stands, fed the lens's rays (s fx2, s fy2, 0.5f) formed in float32 by the test, the
  objects of rpt_orient_objects and E diag(1, R) of rpt_orient_matrix, while the context is handed the UN-turned objects and E: every sky
  pixel bit for bit with Doppler off and on, every hit pixel equal to the frame without the sky, and the whole frame, hit pixels
  included, with Doppler off and on (the oracle restates the sky's Doppler and, in tests/native/doppler_oracle.c, that of a ray that hits);
* Doppler's neutral cases (tests/test_gpu_doppler.py's): with light propagation off, or camera and scene at rest, the Doppler frame is the
  oracle's packed frame for the same rays;
* Doppler with a moving camera: on the scene with every object made flat (one colour each, no light, no texture, no flash) the lit colour
  is known — colour x ambient — and the frame must be the tonemap of S_f(D_cam, lit) of tests/doppler_model.py with D_cam = interval /
  (row 0 of the hit object's re-based Lorentz . (interval, n)), n the lens's ray, formed here in float64."""
import ctypes as C
import math

import numpy as np
import pytest

import doppler_model as dm
import oracle_ffi
from conftest import CONFIGS
from relativitypathtracer_amd.renderer import Renderer, orient_matrix, orient_objects
from relativitypathtracer_amd.scene import OBJECT_DTYPE
from test_camera_view import THREADS, lens_dirs, oracle_rays, ray_oracle  # noqa: F401  (ray_oracle: the fixture)
from test_gpu_camera_view import HALF_PI, LENS_OF, SHOTS, _config, _frame, _plain
from test_gpu_environment import env_oracle, sky_image  # noqa: F401  (env_oracle: the fixture)

pytestmark = pytest.mark.gpu
W, H = 256, 144
SELECTIONS = ((0, False), (41, True), (3, False))      # the blocking call (43's / 44's form), 41's form in flight, the un-culled kernel


@pytest.fixture(scope="module")
def renderer():
    r = Renderer(0)
    yield r
    r.close()


def env_frame(lib, scene, dirs, objects, E, img, flags):
    d, prm = scene.desc(), scene.params
    objects = np.ascontiguousarray(objects).view(np.uint8).reshape(-1)
    a = oracle_ffi.OracleArgs()
    a.objects, a.object_count = objects.ctypes.data, objects.size // 320
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


def _base_kernel(variant, wide, has_mesh):
    return 3 if (variant == 3 or wide) else (41 if variant == 41 else (43 if has_mesh else 44))


def _view(renderer, scene, variant, ypr, v_fov, flags):
    _plain(renderer, scene, W, H, variant)
    renderer.set_orientation(*ypr)
    renderer.set_field_of_view(0 if v_fov is None else v_fov)
    renderer.set_doppler(bool(flags & 1), bool(flags & 2))


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("speed", [0.0, 0.9])
@pytest.mark.parametrize("interval", [-1, 0])
def test_sky_and_neutral_doppler_equal_their_oracles(renderer, ray_oracle, env_oracle, name, speed, interval):
    scene = _config(name, v=(0.0, 0.0, speed), interval=interval)
    has_mesh = bool((scene.objects()["type"] == 2).any())
    at_rest = speed == 0.0 and not np.any(scene.velocities()[:, :3])
    img = sky_image(96, 48)
    E = scene.camera_lorentz()[1]
    for ypr, v_fov in SHOTS:
        dirs = lens_dirs(W, H, HALF_PI if v_fov is None else v_fov)
        objs = orient_objects(scene, *ypr)
        wide = v_fov is not None and v_fov > HALF_PI
        plain_px, _ = oracle_rays(ray_oracle, scene, W, H, dirs, objs)
        for flags in (0, 3):
            opx, orgb, hit = env_frame(env_oracle, scene, dirs, objs, orient_matrix(E, *ypr), img, flags)
            h2 = hit.reshape(H, W)
            for variant, in_flight in SELECTIONS:
                _view(renderer, scene, variant, ypr, v_fov, flags)
                px0, rgb0, k0, _ = _frame(renderer, in_flight)
                base = _base_kernel(variant, wide, has_mesh)
                what = f"{name} v={speed} interval={interval} view {ypr} fov {v_fov} flags {flags} variant {variant}"
                want0 = base + (200 if flags else 0)
                assert k0 == (want0 if v_fov is None else LENS_OF[base] + (10 if flags else 0)), (what, k0)
                if flags and (interval == 0 or at_rest):          # Doppler's neutral cases: the oracle's packed frame
                    assert np.array_equal(px0["rgba"], plain_px["rgba"]), f"{what}: neutral Doppler frame differs from the oracle"
                renderer.set_environment(img)
                renderer.set_environment_frame(E)                 # un-turned: the library re-bases it at the launch
                px, rgb, k, _ = _frame(renderer, in_flight)
                assert k == (base + 600 if v_fov is None else LENS_OF[base] + 20), (what, k)
                assert np.array_equal(rgb.view(np.uint32)[~h2], orgb.view(np.uint32)[~h2]), f"{what}: sky floats differ"
                assert np.array_equal(px.view(np.uint8).reshape(-1, 16)[~hit], opx.view(np.uint8).reshape(-1, 16)[~hit]), f"{what}: sky pixels differ"
                assert np.array_equal(rgb.view(np.uint32)[h2], rgb0.view(np.uint32)[h2]), f"{what}: a hit pixel changed with the sky"
                assert np.array_equal(px.view(np.uint8).reshape(-1, 16)[hit], px0.view(np.uint8).reshape(-1, 16)[hit]), what
                assert np.array_equal(px.view(np.uint8), opx.view(np.uint8)), f"{what}: {int((px['rgba'] != opx['rgba']).any(axis=1).sum())} pixels differ"
                assert np.array_equal(rgb.view(np.uint32), orgb.view(np.uint32)), what
    _plain(renderer, scene, W, H)


def _hable64(x):
    A, B, Cc, D, E, F = 0.15, 0.50, 0.10, 0.20, 0.02, 0.30
    return ((x * (A * x + Cc * B) + D * E) / (x * (A * x + B) + D * F)) - E / F


@pytest.mark.parametrize("name", list(CONFIGS))
@pytest.mark.parametrize("flags", [3, 1, 2])
def test_doppler_factor_follows_the_lens_ray(renderer, ray_oracle, name, flags):
    """Camera at 0.9c, light propagation on, every object flat: frame == tonemap(S_f(D_cam, colour x ambient)) within 1e-3 in the mapped
    colour (range 0..1) on every hit pixel.  The bound: the kernel's float32 D_cam is within 1e-5 relative of the float64 one (the bound
    tests/test_gpu_doppler.py holds the recorded factor to); S_f moves by at most (1.3 / 0.2) x 1e-5 relative through the spectrum's
    steepest segment (knots 0.2 apart, nu / D below 1.3) plus 4e-5 through D^3 / D^4, and the tonemap's slope is below 3 per unit of
    linear colour where the mapped colour is not clamped: some 4e-4 of a colour of order one, rounded up.  A ray that ignored the lens or
    the turn changes D_cam by tens of per cent at this speed."""
    scene = _config(name, v=(0.0, 0.0, 0.9), interval=-1)
    flat = scene.objects().copy()
    n_obj = len(flat)
    flat["light"], flat["textureIndex"], flat["flashPeriod"] = 0, -1, 0
    rng = np.random.default_rng(17)
    colours = rng.uniform(0.2, 1.0, size=(n_obj, 3)).astype(np.float32)
    flat["color"][:, :3] = colours
    ambient = np.float32(scene.params["ambient"])
    wp = np.asarray(scene.params["white_point"], dtype=np.float64)
    has_mesh = bool((flat["type"] == 2).any())
    varied = 0.0
    for ypr, v_fov in SHOTS:
        dirs = lens_dirs(W, H, HALF_PI if v_fov is None else v_fov)
        turned = orient_objects(flat, *ypr).reshape(-1).view(OBJECT_DTYPE)
        # which object each pixel sees: the oracle (no Doppler) on the flat, re-based objects; its colour there is colour x ambient exactly
        _, orgb = oracle_rays(ray_oracle, scene, W, H, dirs, turned)
        lit = (colours * ambient).astype(np.float32)
        mapped_plain = np.minimum(_hable64(lit.astype(np.float64)) / _hable64(wp), 1.0)
        dist = np.abs(orgb[:, :, None, :].astype(np.float64) - mapped_plain[None, None, :, :]).max(axis=-1)      # (H, W, objects)
        obj = dist.argmin(axis=-1)
        second = np.sort(dist, axis=-1)[..., 1] if n_obj > 1 else np.full((H, W), 1.0)
        hit = (dist.min(axis=-1) < 1e-5) & (second > 1e-4)          # (two objects whose colours clamp to the same mapped colour: not told apart, left out)
        n = dirs.astype(np.float64)
        n /= np.linalg.norm(n, axis=1, keepdims=True)
        L0 = turned["Lorentz"][:, 0, :].astype(np.float64)
        k0 = -1.0 * L0[obj.reshape(-1), 0] + np.einsum("pk,pk->p", L0[obj.reshape(-1), 1:], n)
        D = -1.0 / k0
        want = np.minimum(_hable64(dm.S64(D, lit.astype(np.float64)[obj.reshape(-1)], flags)) / _hable64(wp), 1.0).reshape(H, W, 3)
        wide = v_fov is not None and v_fov > HALF_PI
        for variant, in_flight in SELECTIONS:
            _view(renderer, scene, variant, ypr, v_fov, flags)
            renderer.set_objects(flat)                            # un-turned: the library re-bases them
            _, rgb, k, _ = _frame(renderer, in_flight)
            base = _base_kernel(variant, wide, has_mesh)
            what = f"{name} view {ypr} fov {v_fov} flags {flags} variant {variant}"
            assert k == (base + 200 if v_fov is None else LENS_OF[base] + 10), (what, k)
            if hit.any():
                err = np.abs(rgb.astype(np.float64) - want)[hit]
                assert err.max() <= 1e-3, f"{what}: mapped colour off the model by {err.max():.3g} on {int((err.max(axis=-1) > 1e-3).sum())} of {int(hit.sum())} hit pixels"
        if hit.any():
            varied = max(varied, float(np.ptp(D.reshape(H, W)[hit])))
    assert varied > 0.1, (name, varied)          # the factor does vary over the frames
    _plain(renderer, scene, W, H)
