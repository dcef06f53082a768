"""The sky's ground-truth cases — TEST INFRASTRUCTURE shared by tests/test_sky_ground_truth.py (no GPU) and
tests/test_gpu_sky_ground_truth.py: the images, the cameras, the camera forms, the scenes, the case list, and for each case what the
device (or the C restatement) is handed and what the float64 model of tests/sky_truth.py says.  No tests in it.

A case fixes (scene, camera form, camera velocity, sky velocity, frame, image); light delay on / off and the four Doppler flags are
walked inside a case (`SETTINGS`), since they share the case's directions.  The list is no full product: every value of every axis
occurs, every camera form meets every camera, and tests/test_sky_ground_truth.py::test_case_list_covers_every_axis says so."""
from __future__ import annotations

import collections
import functools
import math

import numpy as np

import events_oracle as eo
import mesh_truth
import primitive_truth as pt
import raymap_cases as rc
import sky_truth as st

FRAMES = ((128, 72), (67, 41))                 # 67 x 41: no multiple of any tile
IMAGES = ((64, 32), (37, 19))                  # (W, H); 37 x 19: odd, no power of two
OBLIQUE = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
CAMERAS = {"rest": (0.0, 0.0, 0.0), "0.5c+z": (0.0, 0.0, 0.5), "0.95c-oblique": tuple(float(c) for c in 0.95 * OBLIQUE)}
SKIES = {"scene": None, "moving": (-0.4, 0.2, 0.1)}      # at rest in the scene frame (the library's own matrix is handed over) / a velocity of its own
SETTINGS = ((-1, 0), (-1, 1), (-1, 2), (-1, 3), (0, 0), (0, 3))      # (interval, Doppler flags); with interval 0 the flags change nothing
YPR = (0.4, -0.25, 0.15)
PANO_PART = dict(h_fov=2.0, v_fov=1.2, yaw=0.3)
LENS60, LENS100 = 60.0 * math.pi / 180.0, 100.0 * math.pi / 180.0
FORMS = ("pinhole", "lens60", "lens100", "turned", "pano_full", "pano_part", "fisheye")
MIN_PIXELS = 500
CAP_LOOSE, CAP_UNDECIDED = 0.01, 0.02


def settings(case):
    """A case's (interval, flags) pairs.  A windowed case keeps light delay on: without it every event of an object at rest against the
    camera has one time, choose_windows' median bound IS that time, and the verdict of every such pixel turns on a rounding."""
    return tuple(s for s in SETTINGS if s[0] != 0) if case.windowed else SETTINGS


Case = collections.namedtuple("Case", "name scene form camera sky frame image windowed")


def sky_image(W, H, seed=1):
    """Smooth, periodic in azimuth, with no mirror symmetry in azimuth or latitude; on top the one-texel markers of
    test_gpu_environment.sky_image: six scattered, one on the wrap column, one on the last column, one in each pole row."""
    y, x = np.mgrid[0:H, 0:W]
    az, lat = 2 * np.pi * x / W, np.pi * (0.5 - (y + 0.5) / H)
    r = 128 + 80 * np.sin(az + 0.7) + 35 * np.sin(2 * az + 0.3) * np.cos(lat)
    g = 40 + 170 * ((y + 0.5) / H) ** 1.5 + 20 * np.cos(az - 2.0)
    b = 128 + 55 * np.cos(az - 1.1) + 45 * np.sin(3 * lat + az)
    img = np.clip(np.rint(np.stack([r, g, b], -1)), 0, 255).astype(np.uint8)
    rng = np.random.default_rng(seed)
    for k in range(6):
        img[rng.integers(0, H), rng.integers(0, W)] = (255, 255 * (k & 1), 0)
    img[H // 2, 0] = (0, 255, 255)
    img[H // 3, W - 1] = (255, 0, 255)
    img[0, W // 2] = (255, 255, 255)
    img[H - 1, W // 4] = (0, 0, 0)
    return np.ascontiguousarray(img)


@functools.lru_cache(maxsize=None)
def image(size):
    img = sky_image(*size, seed=size[0])
    img.setflags(write=False)
    return img


def _cases():
    out = []
    for f, form in enumerate(FORMS):
        for c, camera in enumerate(CAMERAS):
            sky = "moving" if (f + c) % 2 else "scene"
            frame, img = FRAMES[(f + c + (c == 2)) % 2], IMAGES[(f // 2 + c) % 2]
            if form == "pano_full" and c == 2:
                frame = FRAMES[0]          # ahead of 0.95c the sky is compressed sixfold: 67 x 41 pixels step over a pole row of the image there
            out.append(Case(f"allsky-{form}-{camera}-{sky}", "allsky", form, camera, sky, frame, img, False))
    for f, form in enumerate(FORMS):
        camera = list(CAMERAS)[f % 3]
        out.append(Case(f"cubes-{form}-{camera}", "cubes", form, camera, "scene" if f % 2 else "moving", FRAMES[0], IMAGES[f % 2], False))
    # (windows need objects of a dozen pixels and more: at 0.95c the cubes shrink below that ahead of the camera)
    for f, (form, camera) in enumerate((("pinhole", "0.5c+z"), ("pano_part", "rest"), ("fisheye", "rest"))):
        out.append(Case(f"cubes-windowed-{form}-{camera}", "cubes", form, camera, "scene", FRAMES[0], IMAGES[(f + 1) % 2], True))
    return out


CASES = {c.name: c for c in _cases()}


def case_ids():
    return list(CASES)


# ---- the camera forms ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def form_rays(form, frame):
    """(dirs (N, 3) float32 as the CPU references take them, mask of pixels that have a ray or None, ypr, the renderer's view settings)"""
    W, H = frame
    if form == "pinhole":
        return eo.pinhole_dirs(W, H), None, (0.0, 0.0, 0.0), {}
    if form in ("lens60", "lens100"):
        v = LENS60 if form == "lens60" else LENS100
        return eo.pinhole_dirs(W, H, eo.lens_scale(v)), None, (0.0, 0.0, 0.0), dict(v_fov=v)
    if form == "turned":
        return eo.pinhole_dirs(W, H), None, YPR, dict(ypr=YPR)
    if form == "pano_full":
        return eo.pano_dirs(W, H), None, (0.0, 0.0, 0.0), dict(pano={})
    if form == "pano_part":
        return eo.pano_dirs(W, H, **PANO_PART), None, (0.0, 0.0, 0.0), dict(pano=PANO_PART)
    from relativitypathtracer_amd.renderer import raymap
    m = raymap("fisheye", W, H, fov=math.pi, fit=0)
    return rc.oracle_dirs(m), rc.has_ray(m), (0.0, 0.0, 0.0), dict(ray_map=m)


# ---- the scenes ------------------------------------------------------------------------------------------------------------------------
TRIANGLE = "MModels/triangle.obj\n"
CUBES_TIMES = {"rest": 3.0, "0.5c+z": 0.0, "0.95c-oblique": 0.0}      # the moving cameras pass the origin at t = 0 (events_oracle.load_scene's rule)


def allsky_text(camera, flavour="analytic"):
    """One tiny object far behind the camera's motion (behind the view at rest): next to every pixel is sky whatever the camera form.
    flavour "mesh": a small triangle instead of the sphere, so that the walk kernels are chosen."""
    v = np.array(CAMERAS[camera])
    back = -v / np.linalg.norm(v) if v.any() else np.array([0.0, 0.0, -1.0])
    p = 60.0 * back
    if flavour == "analytic":
        return f"Os\n p{p[0]},{p[1]},{p[2]},0,0,1,0,0.02,0.02,0.02\n c1,0.8,0.6\n l1\n v0,0,0\nA0.2\nR\n"
    return TRIANGLE + f"Om0\n p{p[0]},{p[1]},{p[2]},0,0,1,0,0.02,0.02,0.02\n c1,0.8,0.6\n v0,0,0\nA0.2\nR\n"


def scene_of(case, interval, flavour="analytic", extra_obj=None):
    """The case's scene.  An all-sky case has flavours: "analytic" (the sphere), "mesh" (the triangle) and, with extra_obj the path of an
    .obj file that puts the mesh pool outside the exact reciprocal's domain (kernel_choice_cases.HUGE_OBJ, named by no object), the scene
    on which the walk kernels take their IEEE form."""
    from relativitypathtracer_amd import Scene
    if case.scene == "allsky":
        s = Scene()
        s.inputScene(allsky_text(case.camera, flavour))
        if extra_obj:
            s.ReadOBJ(extra_obj)
        s.set_interval(interval)
        s.set_camera(CAMERAS[case.camera], 0.0)
        s.update_objects()
        return s
    s = Scene.from_file("cubes")
    s.set_interval(interval)
    s.set_camera(CAMERAS[case.camera], CUBES_TIMES[case.camera])
    s.update_objects()
    return s


# ---- what the float programs are handed, and what the model says -------------------------------------------------------------------------
def device_matrix(case, scene):
    """E as the device and the restatement get it, UN-turned: the library's own camera_lorentz()[1] for a sky at rest in the scene frame
    (so that matrix is held to physics too), the float32 rounding of the model's float64 product for a sky with a velocity of its own."""
    if SKIES[case.sky] is None:
        return scene.camera_lorentz()[1]
    return st.sky_frame(CAMERAS[case.camera], SKIES[case.sky]).astype(np.float32)


def matrix_error(case):
    if SKIES[case.sky] is None:
        return st.library_matrix_error(CAMERAS[case.camera])
    return st.EPS


def model(case, interval, flags, white_point, frame_fn=None):
    dirs, _, ypr, _ = form_rays(case.form, case.frame)
    fn = st.frame if frame_fn is None else frame_fn
    return fn(dirs, image(case.image), v_cam=CAMERAS[case.camera], v_sky=SKIES[case.sky] or (0.0, 0.0, 0.0), ypr=ypr, interval=interval, flags=flags,
              white_point=white_point, e_matrix=matrix_error(case))


def verdict(case, scene, interval, windows=None):
    """Which pixels are sky: primitive_truth's verdict on the UN-turned objects along the float64 directions R n — (clear misses, clear
    hits, undecided), each (N,) bool; pixels of a ray map without a ray are in none of them."""
    dirs, mask, ypr, _ = form_rays(case.form, case.frame)
    d = dirs.astype(np.float64) @ st.rotation(*ypr).T
    objs = scene.objects()
    has_mesh = bool((objs["type"] == 2).any())
    m = pt.frame(objs, d, interval, windows=windows, mesh_arrays=mesh_truth.arrays(scene) if has_mesh else None, colour=False)
    ray = np.ones(len(d), dtype=bool) if mask is None else mask
    well = m["well_rec"] & ray
    return well & (m["object"] < 0), well & (m["object"] >= 0), ray & ~m["well_rec"]


def seam_and_poles(case, mod, sky):
    """For the full-sphere cases: compared pixels on both sides of the seam (last and first texel column) and in both pole rows."""
    W, H = case.image
    x, y = mod["texel"][sky, 0], mod["texel"][sky, 1]
    return bool((x == W - 1).any() and (x == 0).any() and (y == 0).any() and (y == H - 1).any())


def crafted_directions(W, H):
    """Directions at which the lookup alone is held to the model: the axes, both sides of the seam, within 1e-3 of each pole, texel centres
    (integer (U, V)) and texel corners (half-integer)."""
    d = [[1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]]
    for y in (-0.6, 0.0, 0.3):
        for z in (1e-2, 1e-4, 1e-6):
            d += [[-1, y, z], [-1, y, -z]]
    for s in (1.0, -1.0):
        for h in (1e-3, 5e-4, 2e-4):
            for a in (0.3, 1.7, 2.9, 4.0, 5.5):
                d.append([h * math.cos(a), s * math.sqrt(1 - h * h), h * math.sin(a)])
    d = [np.array(d, dtype=np.float64)]
    for off in (0.0, 0.5):
        y, x = np.mgrid[0:H, 0:W].astype(np.float64)
        u, v = (x + off) / W, 1.0 - (y + off) / H
        az, lat = 2 * np.pi * (u - 0.5), np.pi * (v - 0.5)
        d.append(np.stack([np.cos(lat) * np.cos(az), np.sin(lat), np.cos(lat) * np.sin(az)], -1).reshape(-1, 3))
    return np.ascontiguousarray(np.concatenate(d).astype(np.float32))
