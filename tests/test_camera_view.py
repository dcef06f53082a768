"""The free-look camera's host side (rpt_set_orientation's arithmetic, rpt_orient_objects / rpt_orient_matrix, look_at) without a GPU:
the re-basing against numpy float64, the sign conventions through the CPU oracle (which knows nothing of the new code), and the screen
regions' proofs on re-based objects under every lens (DESIGN.md "Free-look camera")."""
import ctypes as C
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_ffi
import test_screen_bounds as tsb
from conftest import CONFIGS, load_config
from relativitypathtracer_amd import Scene, _ffi
from relativitypathtracer_amd.renderer import look_at, orient_matrix, orient_objects, rotation_matrix
from relativitypathtracer_amd.scene import OBJECT_DTYPE
from scene_fuzz import close_scene_text, extreme_scene_text, random_scene_text, walls_scene_text

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PANO_SRC = os.path.join(ROOT, "tests", "native", "panorama_oracle.c")
CFLAGS = ["-O2", "-std=gnu11", "-fPIC", "-ffp-contract=off", "-fno-fast-math"]       # oracle/Makefile's
THREADS = min(16, os.cpu_count() or 1)
FULL = 3.0e38
VIEWS = [(math.pi, 0.0, 0.0), (0.4, 0.5, 0.3), (-1.1, -0.35, 2.0), (2.2, 0.9, -0.7)]      # yaw, pitch, roll: the orientations tried below


def _scene(text, v=(0.0, 0.0, 0.0), t=0.0, interval=None):
    s = Scene()
    s.inputScene(text)
    if interval is not None:
        s.set_interval(interval)
    s.set_camera(v, t)
    s.update_objects()
    return s


def _matrices(raw):
    o = np.ascontiguousarray(raw).view(np.uint8).reshape(-1, 320)
    f = o[:, 128:256].copy().view(np.float32).reshape(-1, 2, 4, 4)
    return f[:, 0], f[:, 1]          # Lorentz, InvLorentz


def _ulps(a, b):
    """Distance in float32 steps; equal bit patterns (NaN payloads included) count 0."""
    ia, ib = (np.ascontiguousarray(x, dtype=np.float32).view(np.int32).astype(np.int64) for x in (a, b))
    ia, ib = (np.where(i < 0, -(i & 0x7fffffff), i) for i in (ia, ib))
    return np.abs(ia - ib)


def _fuzz_objects(seed):
    rng = np.random.default_rng(seed)
    raws = []
    for k in range(6):
        text = [lambda: random_scene_text(rng)[0], lambda: extreme_scene_text(rng), lambda: close_scene_text(rng)][k % 3]()
        v = rng.normal(size=3)
        v = v / np.linalg.norm(v) * rng.choice([0.0, 0.5, 0.9, 0.99])
        s = _scene(text, tuple(float(c) for c in v), float(rng.uniform(-2, 10)))
        raws.append(np.ctypeslib.as_array(C.cast(s.desc().objects, C.POINTER(C.c_uint8)), shape=(int(s.desc().object_count) * 320,)).copy())
    return np.concatenate(raws).reshape(-1, 320)


# ---- 1. the arithmetic ---------------------------------------------------------------------------------------------------------------
def test_orient_objects_is_the_float64_product_rounded_once():
    """Every entry of Lorentz' = Lorentz diag(1, R) and InvLorentz' = diag(1, R^T) InvLorentz within one float ulp of the three-term sum
    formed in numpy float64 (the two libms may differ in the last bit of sin / cos; measured here: 0 ulp everywhere), every other byte
    of the object untouched.

    Lorentz' InvLorentz' stays as close to the identity as Lorentz InvLorentz was: R R^T = I up to 2.2e-16, so the turned product differs
    from the un-turned one only by the float rounding of the re-based entries, 2^-24 relative per entry of each factor — at most
    2 * 2^-24 * sum_k |L'_ik| |I'_kj| per entry of the product, which is what is asserted on top of the un-turned product's own largest
    deviation.  Measured over the objects below (boosts up to 0.9999c against a camera at up to 0.99c, 16 orientations): among objects
    whose un-turned product is not the exact identity the largest deviation grows by a factor of at most 2.9; the largest increase in
    absolute terms is 4.5e-4, on a product whose entries are of the order 1e4 (gamma in the thousands)."""
    raw = _fuzz_objects(11)
    assert len(raw) >= 12
    L, I = _matrices(raw)
    rng = np.random.default_rng(5)
    worst, worst_abs = 0.0, 0.0
    for ypr in VIEWS + [tuple(float(a) for a in rng.uniform(-4, 4, size=3)) for _ in range(12)]:
        out = orient_objects(raw, *ypr)
        R = rotation_matrix(*ypr)
        L2, I2 = _matrices(out)
        Ld, Id = L.astype(np.float64), I.astype(np.float64)
        wantL, wantI = Ld.copy(), Id.copy()
        for c in range(3):
            wantL[:, :, 1 + c] = Ld[:, :, 1] * R[0, c] + Ld[:, :, 2] * R[1, c] + Ld[:, :, 3] * R[2, c]
            wantI[:, 1 + c, :] = R[0, c] * Id[:, 1, :] + R[1, c] * Id[:, 2, :] + R[2, c] * Id[:, 3, :]
        with np.errstate(over="ignore", invalid="ignore"):
            assert _ulps(L2, wantL.astype(np.float32)).max() <= 1, ypr
            assert _ulps(I2, wantI.astype(np.float32)).max() <= 1, ypr
        assert np.array_equal(L2[:, :, 0], L[:, :, 0]) and np.array_equal(I2[:, 0, :], I[:, 0, :])      # the time column / row: copied
        rest = np.ones(320, dtype=bool)
        rest[128:256] = False
        assert np.array_equal(out[:, rest], raw[:, rest])
        for k in range(len(raw)):
            before = np.abs(Ld[k] @ Id[k] - np.eye(4))
            after = np.abs(L2[k].astype(np.float64) @ I2[k].astype(np.float64) - np.eye(4))
            allowance = 2.0 * 2.0 ** -24 * (np.abs(L2[k].astype(np.float64)) @ np.abs(I2[k].astype(np.float64))) * 1.01 + 1e-30
            assert (after <= before.max() + allowance).all(), (ypr, k, float(after.max()), float(before.max()))
            if before.max() > 0:
                worst = max(worst, float(after.max() / before.max()))
            worst_abs = max(worst_abs, float(after.max() - before.max()))
    print(f"max |L I - 1| under re-basing: largest growth x{worst:.3f} (objects with a non-zero residual), largest increase {worst_abs:.3g}")


def test_no_turn_keeps_the_bytes():
    raw = _fuzz_objects(12)
    raw[0, 128:132] = np.frombuffer(np.float32(-0.0).tobytes(), np.uint8)          # -0.0f and a NaN keep their bit patterns
    raw[1, 196:200] = np.frombuffer(np.uint32(0x7fc01234).tobytes(), np.uint8)
    assert np.array_equal(orient_objects(raw, 0.0, 0.0, 0.0), raw)
    assert np.array_equal(orient_objects(raw, -0.0, 0.0, -0.0), raw)
    out = np.empty_like(raw)
    assert _ffi.hip().rpt_orient_objects(raw.ctypes.data, len(raw), None, out.ctypes.data) == 0
    assert np.array_equal(out, raw)
    E = np.arange(16, dtype=np.float32).reshape(4, 4)
    E[2, 3] = -0.0
    assert np.array_equal(orient_matrix(E).view(np.uint32), E.view(np.uint32))
    fp = C.POINTER(C.c_float)
    out16 = np.empty(16, dtype=np.float32)
    assert _ffi.hip().rpt_orient_matrix(E.ctypes.data_as(fp), None, out16.ctypes.data_as(fp)) == 0
    assert np.array_equal(out16.view(np.uint32), E.reshape(16).view(np.uint32))


def test_orient_matrix_is_the_objects_lorentz_rule():
    raw = _fuzz_objects(13)
    L, _ = _matrices(raw)
    for ypr in VIEWS:
        L2, _ = _matrices(orient_objects(raw, *ypr))
        for k in range(0, len(raw), 3):
            assert np.array_equal(orient_matrix(L[k], *ypr).view(np.uint32), L2[k].view(np.uint32))


def test_in_place_is_allowed():
    raw = _fuzz_objects(14)
    want = orient_objects(raw, *VIEWS[1])
    buf = raw.copy()
    assert _ffi.hip().rpt_orient_objects(buf.ctypes.data, len(buf), (C.c_float * 3)(*VIEWS[1]), buf.ctypes.data) == 0
    assert np.array_equal(buf, want)


# ---- 2. the convention ---------------------------------------------------------------------------------------------------------------
def test_each_angle_alone():
    q = math.pi / 2
    ez, ex, ey = np.array([0, 0, 1.0]), np.array([1.0, 0, 0]), np.array([0, 1.0, 0])
    assert np.allclose(rotation_matrix(q, 0, 0) @ ez, ex, atol=1e-7)        # yaw: the view turns towards +x
    assert np.allclose(rotation_matrix(0, q, 0) @ ez, ey, atol=1e-7)        # pitch: towards +y
    assert np.allclose(rotation_matrix(0, 0, q) @ ez, ez, atol=1e-7)        # roll: the view direction stays ...
    assert np.allclose(rotation_matrix(0, 0, q) @ ey, ex, atol=1e-7)        # ... the image's up is the old +x: the world's up is drawn on the left
    assert np.allclose(rotation_matrix(0, 0, q) @ ex, -ey, atol=1e-7)
    # the library's matrix is this one: the un-turned camera's +z column of an identity Lorentz block is R's third column, etc.
    E = np.eye(4, dtype=np.float32)
    for ypr in VIEWS:
        assert np.abs(orient_matrix(E, *ypr)[1:, 1:].astype(np.float64) - rotation_matrix(*ypr)).max() <= 2.0 ** -24
    # and it composes as Ry Rx Rz
    y, p, r = 0.3, -0.7, 1.9
    assert np.allclose(rotation_matrix(y, p, r), rotation_matrix(y, 0, 0) @ rotation_matrix(0, p, 0) @ rotation_matrix(0, 0, r), atol=1e-15)
    R = rotation_matrix(y, p, r)
    assert np.allclose(R @ R.T, np.eye(3), atol=1e-15) and abs(np.linalg.det(R) - 1) < 1e-15


def test_look_at_returns_the_direction():
    rng = np.random.default_rng(7)
    dirs = [rng.normal(size=3) for _ in range(400)]
    dirs += [np.array(d, dtype=float) for d in ((0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 5, 1e-9), (1e-13, -3, 0))]
    for d in dirs:
        ypr = look_at(d)
        R = rotation_matrix(*ypr)
        n = d / np.linalg.norm(d)
        assert np.abs(R @ np.array([0, 0, 1.0]) - n).max() <= 3e-7, (d, ypr)          # (the angles go through float32)
        up = R @ np.array([0, 1.0, 0])
        if abs(n[1]) < 1 - 1e-9:             # away from the poles: the image's up is the world's, as far as the view allows
            want = np.array([0, 1.0, 0]) - n * n[1]
            assert np.abs(up - want / np.linalg.norm(want)).max() <= 1e-5, (d, ypr)
    # the poles: the yaw is defined by `up`.  Default up = +y is parallel to the view there: yaw 0, roll 0.
    assert look_at((0, 1, 0)) == (0.0, math.pi / 2, 0.0) and look_at((0, -2, 0)) == (0.0, -math.pi / 2, 0.0)
    # looking straight up with the image's up towards -z: the head tilted back from +z, yaw 0
    y, p, r = look_at((0, 1, 0), up=(0, 0, -1))
    assert abs(y) < 1e-12 and abs(p - math.pi / 2) < 1e-12 and abs(r) < 1e-12
    for up in ((1, 0, 0), (0.3, 0, -2), (-1, 5, 1)):
        for d in ((0, 1, 0), (0, -1, 0)):
            R = rotation_matrix(*look_at(d, up=up))
            w = np.array(up, dtype=float) - np.array(d, dtype=float) * float(np.dot(up, d))
            assert np.abs(R @ np.array([0, 1.0, 0]) - w / np.linalg.norm(w)).max() <= 3e-7
            assert np.abs(R @ np.array([0, 0, 1.0]) - np.array(d, dtype=float)).max() <= 3e-7
    with pytest.raises(ValueError):
        look_at((0, 0, 0))
    with pytest.raises(ValueError):
        look_at((float("nan"), 0, 1))


# ---- 3. geometry through the oracle ------------------------------------------------------------------------------------------------
W3, H3 = 64, 36


def _centre_hit(scene, objects):
    _, rgb, _ = oracle_ffi.render(scene, W3, H3, objects=objects, rows=(H3 // 2, H3 // 2 + 1))      # pixel (W/2, H/2) looks along exactly (0, 0, 1/2)
    return not np.array_equal(rgb[H3 // 2, W3 // 2], tsb._background(scene, W3, H3))


def _sphere_text(d, dist=10.0, radius=0.25):
    p = np.asarray(d, dtype=float) / np.linalg.norm(d) * dist
    return f"Os\n p{p[0]:.6f},{p[1]:.6f},{p[2]:.6f},0,0,1,0,{radius},{radius},{radius}\n c1,0.5,0.25\n l1\nA1\nR\n"


DIRECTIONS = [(1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (-1, 0.2, 0.1), (0.5, 0.6, -0.7), (0.3, -0.8, 0.4), (-0.6, -0.1, -0.9)]


@pytest.mark.parametrize("d", DIRECTIONS)
def test_camera_at_rest_sees_what_it_looks_at(d):
    scene = _scene(_sphere_text(d), interval=-1)
    raw = scene.objects().copy()
    assert not _centre_hit(scene, raw)                                       # the un-turned camera looks down +z, elsewhere
    assert _centre_hit(scene, orient_objects(raw, *look_at(d)))
    assert not _centre_hit(scene, orient_objects(raw, *look_at(-np.asarray(d, dtype=float))))
    y, p, r = look_at(d)
    assert _centre_hit(scene, orient_objects(raw, y, p, r + 1.3))            # a roll turns the image about its centre


@pytest.mark.parametrize("d", DIRECTIONS)
@pytest.mark.parametrize("b", [(0, 0, 1), (1, 0, 0), (0.6, -0.3, 0.5)])
def test_camera_at_09c_sees_it_in_the_aberrated_direction(d, b):
    """A sphere at rest in the scene, in direction d of a camera that passes the origin at t = 0 with velocity 0.9 b: its light arrives
    from d in the scene's frame and from n' = (d_perp / gamma + (d.b + beta) b) / (1 + beta d.b) in the camera's (b the unit velocity):
    the source is displaced towards the direction of motion."""
    beta = 0.9
    b = np.asarray(b, dtype=float) / np.linalg.norm(b)
    n = np.asarray(d, dtype=float) / np.linalg.norm(d)
    gamma = 1.0 / math.sqrt(1.0 - beta * beta)
    par = float(n @ b)
    seen = ((n - par * b) / gamma + (par + beta) * b) / (1.0 + beta * par)
    assert abs(np.linalg.norm(seen) - 1.0) < 1e-12
    scene = _scene(_sphere_text(d, radius=0.12), v=tuple(float(c) for c in beta * b), t=0.0, interval=-1)
    raw = scene.objects().copy()
    assert _centre_hit(scene, orient_objects(raw, *look_at(seen)))
    if float(seen @ n) < 0.999:                                               # where aberration moved it visibly, the un-aberrated direction misses
        assert not _centre_hit(scene, orient_objects(raw, *look_at(n)))


# ---- 4. the proofs on re-based objects, under every lens -------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ray_oracle(tmp_path_factory):
    if shutil.which("gcc") is None:
        pytest.fail("gcc is needed to build tests/native/panorama_oracle.c")
    so = str(tmp_path_factory.mktemp("lens") / "libpanorama_oracle.so")
    p = subprocess.run(["gcc", *CFLAGS, "-shared", "-o", so, PANO_SRC, "-lm", "-lpthread"], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    lib = C.CDLL(so)
    lib.rpt_panorama_oracle_render.restype = C.c_int
    lib.rpt_panorama_oracle_render.argtypes = [C.POINTER(oracle_ffi.OracleArgs), C.c_void_p, C.c_int, C.c_int, C.c_int]
    return lib


def lens_dirs(W, H, v_fov):
    """(H * W, 3) float32 (s fx2, s fy2, 0.5f) as the lens kernels form them: createCamRayDir's float32 steps, then the two products."""
    s = np.float32(math.tan(0.5 * float(np.float32(v_fov))))
    y, x = np.mgrid[0:H, 0:W].astype(np.float32)
    fx2 = (x / np.float32(W) - np.float32(0.5)) * (np.float32(W) / np.float32(H))
    fy2 = y / np.float32(H) - np.float32(0.5)
    return np.ascontiguousarray(np.stack([s * fx2, s * fy2, np.full_like(fx2, 0.5)], -1).reshape(-1, 3).astype(np.float32))


def oracle_rays(lib, scene, W, H, dirs, objects, rows=None):
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
    a.out_pixels, a.out_rgb = px.ctypes.data, rgb.ctypes.data
    r0, r1 = (0, H) if rows is None else rows          # (rows outside stay zero)
    assert lib.rpt_panorama_oracle_render(C.byref(a), dirs.ctypes.data, r0, r1, THREADS) == 0
    return px, rgb


def _root(scene, objs, i):
    if int(objs["type"][i]) != 2:
        return None
    n = scene.octrees()[int(objs["meshIndex"][i])]
    return (C.c_float * 6)(*n["min"][:3], *n["max"][:3])


def _bounds(fn, raw, interval, root):
    b = (C.c_float * 8)()
    assert fn(raw.ctypes.data, interval, root, b) == 0
    return tuple(b)


def _claims_nothing(b):
    return b[0] <= -FULL and b[1] <= -FULL and b[2] >= FULL and b[3] >= FULL


def _check_regions(lib, scene, ypr, label, fovs=(0.2, 1.0, math.pi / 2), W=128, H=72):
    """Per object: the proposal on the re-based object, the proof's verdict, and — if it is accepted — no oracle hit of the object
    outside the region on a grid of each lens's rays.  Returns (proposals that claim something, of which accepted)."""
    lib_hip = _ffi.hip()
    turned = orient_objects(scene, *ypr).reshape(-1).view(OBJECT_DTYPE)
    interval = scene.params["interval"]
    claims = accepted = 0
    for i in range(min(len(turned), 64)):
        raw, root = turned[i:i + 1].copy(), _root(scene, turned, i)
        prop = _bounds(lib_hip.rpt_object_screen_bounds_proposed, raw, interval, root)
        used = _bounds(lib_hip.rpt_object_screen_bounds, raw, interval, root)
        if _claims_nothing(prop):
            continue
        claims += 1
        if _claims_nothing(used):
            continue                                  # not proven: the object is tested for every pixel
        assert lib_hip.rpt_certify_screen_bounds(raw.ctypes.data, interval, root, (C.c_float * 8)(*used), None) == 1
        accepted += 1
        only = raw.copy()
        only["light"], only["textureIndex"], only["flashPeriod"] = 0, -1, 0
        only["color"] = (1.0, 0.5, 0.25, 0.0)
        for v_fov in fovs:
            dirs = lens_dirs(W, H, v_fov)
            _, rgb = oracle_rays(lib, scene, W, H, dirs, only)
            hit = ~((rgb == tsb._background(scene, W, H)).all(axis=2))
            u, v = dirs[:, 0].reshape(H, W).astype(np.float64), dirs[:, 1].reshape(H, W).astype(np.float64)
            bad = hit & ~tsb.inside_bounds(used, u, v)
            assert not bad.any(), f"{label}: view {ypr}, v_fov {v_fov}: object {i}: PROVEN region {used} leaves out {int(bad.sum())} hit pixels"
    return claims, accepted


@pytest.mark.parametrize("name", list(CONFIGS))
def test_proven_regions_hold_on_turned_shipped_scenes(ray_oracle, name):
    """The proof takes Lorentz as 'a 4 x 4 the kernel multiplies by' (its conditions — A3 invertible, |c| < 1, the noise bound — are
    CHECKED on the matrices it is given, not derived from their being a boost), so a turned camera needs no change to it; this test is
    the evidence.  Not vacuous: at every orientation tried at least half of the proposals that claim anything are accepted (measured:
    all of them, on every shipped scene and view; printed below)."""
    scene = load_config(name)
    for ypr in VIEWS:
        claims, accepted = _check_regions(ray_oracle, scene, ypr, name, W=96, H=54)
        print(f"{name} view {ypr}: {accepted} of {claims} claims proven")
        assert 2 * accepted >= claims, (name, ypr, claims, accepted)


@pytest.mark.parametrize("seed", range(12))
def test_proven_regions_hold_on_turned_generated_scenes(ray_oracle, seed):
    rng = np.random.default_rng(900 + seed)
    gens = [lambda: random_scene_text(rng)[0], lambda: extreme_scene_text(rng), lambda: close_scene_text(rng), lambda: walls_scene_text(rng)]
    text = gens[seed % 4]()
    v = rng.normal(size=3)
    v = v / np.linalg.norm(v) * rng.choice([0.0, 0.5, 0.9])
    scene = _scene(text, tuple(float(c) for c in v), float(rng.uniform(-2, 12)))
    ypr = tuple(float(a) for a in rng.uniform(-math.pi, math.pi, size=3))
    claims, accepted = _check_regions(ray_oracle, scene, ypr, f"seed {900 + seed}\n{text}", W=96, H=54)
    print(f"seed {900 + seed} view {ypr}: {accepted} of {claims} claims proven")


# ---- 5. arguments --------------------------------------------------------------------------------------------------------------------
def test_argument_validation():
    lib = _ffi.hip()
    raw = _fuzz_objects(15)[:2].copy()
    out = np.empty_like(raw)
    f3 = lambda *a: (C.c_float * 3)(*a)
    assert lib.rpt_orient_objects(raw.ctypes.data, 2, f3(0.1, 0.2, 0.3), out.ctypes.data) == 0
    for bad in (f3(float("nan"), 0, 0), f3(0, float("inf"), 0), f3(0, 0, -float("inf"))):
        assert lib.rpt_orient_objects(raw.ctypes.data, 2, bad, out.ctypes.data) == 1
    assert lib.rpt_orient_objects(raw.ctypes.data, -1, f3(0, 0, 0), out.ctypes.data) == 1
    assert lib.rpt_orient_objects(None, 2, f3(0, 0, 0), out.ctypes.data) == 1
    assert lib.rpt_orient_objects(raw.ctypes.data, 2, f3(0, 0, 0), None) == 1
    assert lib.rpt_orient_objects(None, 0, None, None) == 0                      # nothing to do is not an error
    fp = C.POINTER(C.c_float)
    E = np.eye(4, dtype=np.float32)
    o = np.empty(16, dtype=np.float32)
    assert lib.rpt_orient_matrix(E.ctypes.data_as(fp), f3(1, 2, 3), o.ctypes.data_as(fp)) == 0
    assert lib.rpt_orient_matrix(None, f3(1, 2, 3), o.ctypes.data_as(fp)) == 1
    assert lib.rpt_orient_matrix(E.ctypes.data_as(fp), f3(1, 2, 3), None) == 1
    assert lib.rpt_orient_matrix(E.ctypes.data_as(fp), f3(float("nan"), 2, 3), o.ctypes.data_as(fp)) == 1
    # the context's setters reject a null context without touching it (their ranges are checked on the GPU, where a context exists)
    assert lib.rpt_set_orientation(None, f3(0, 0, 0)) == 1
    assert lib.rpt_set_field_of_view(None, 1.0) == 1
    with pytest.raises(ValueError):
        orient_objects(raw, float("nan"), 0, 0)
    with pytest.raises(ValueError):
        orient_objects(np.zeros(100, np.uint8))
