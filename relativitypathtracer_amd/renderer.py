"""Renderer — Python face of the C-ABI render path (include/rpt.h, librpt_hip.so).

Mirrors the reference's device-runtime glue (CLSetup.h:22-26): ``initOpenCL`` -> ``Renderer()``,
the eight buffer uploads of main.cpp:33-55 -> ``upload_scene``, ``initCLKernel`` ->
``set_params``/``set_output``, the per-frame ``enqueueWriteBuffer(cl_objects)`` -> ``set_objects``,
``runKernel`` -> ``render``.  Everything executes in the HIP library; there is no fallback path.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Mapping, Optional, Sequence, Tuple, Union

import numpy as np

from . import _ffi
from .events import EVENT_DTYPE
from .scene import Scene

PIXEL_DTYPE = np.dtype([("x", "<f4"), ("y", "<f4"), ("rgba", "u1", (4,)), ("unspecified", "<u4")])
TILE_ROWS = 8
DOPPLER_SHIFT, DOPPLER_BEAMING = 1, 2     # rpt_set_doppler flags (include/rpt.h)
DOPPLER_RECORD = 11                       # floats per pixel of the Doppler debug record
PROJECTIONS = {"pinhole": 0, "equirect": 1, "raymap": 2}   # RPT_PROJECTION_* (include/rpt.h)
RAYMAP_KINDS = {"fisheye": 0, "equisolid": 1, "stereographic": 2, "cube_strip": 3}   # RPT_RAYMAP_* (include/rpt.h)


class RenderError(RuntimeError):
    """A call of the library failed; `code` is its return code (include/rpt.h: RPT_ERR_*), None where no call is behind it."""
    code = None


def _projection_args(mode: str, h_fov: float, v_fov: float, yaw: float):
    if mode not in PROJECTIONS:
        raise ValueError(f"projection is one of {sorted(PROJECTIONS)}, not {mode!r}")
    params = (C.c_float * 3)(h_fov, v_fov, yaw) if mode == "equirect" else None
    return PROJECTIONS[mode], params


def projection_tables(width: int, height: int, h_fov: float = 2 * math.pi, v_fov: float = math.pi, yaw: float = 0.0,
                      mode: str = "equirect") -> Tuple[np.ndarray, np.ndarray]:
    """The two tables the panorama kernels read for a width x height frame (rpt_projection_tables; host code, no device needed):
    cols (width, 2) = {sin, cos} of each column's longitude, rows (height, 2) = {sin, cos} of each row's latitude, float32."""
    m, params = _projection_args(mode, h_fov, v_fov, yaw)
    cols = np.empty((max(int(width), 0), 2), dtype=np.float32)
    rows = np.empty((max(int(height), 0), 2), dtype=np.float32)
    rc = _ffi.hip().rpt_projection_tables(m, params, int(width), int(height), cols.ctypes.data, rows.ctypes.data)
    if rc != 0:
        raise ValueError(f"rpt_projection_tables({mode!r}, {h_fov}, {v_fov}, {yaw}, {width}x{height}) failed ({rc})")
    return cols, rows


def raymap(kind: str, width: int, height: int, fov: float = math.pi, fit: int = 0) -> np.ndarray:
    """A standard ray map for a width x height frame (rpt_raymap_fill; host code, no device needed): (height, width, 3) float32, row 0
    the bottom, (0, 0, 0) where a pixel has no ray.  kind: "fisheye" (equidistant), "equisolid" or "stereographic" with the full angle
    fov in radians across the image circle, which fit = 0 inscribes in the frame and fit = 1 stretches to its diagonal; or "cube_strip"
    (width = 6 height; faces +x, -x, +y, -y, +z, -z from the left; fov and fit are not used)."""
    if kind not in RAYMAP_KINDS:
        raise ValueError(f"a ray map's kind is one of {sorted(RAYMAP_KINDS)}, not {kind!r}")
    params = None if kind == "cube_strip" else (C.c_float * 2)(float(fov), float(fit))
    dirs = np.empty((max(int(height), 0), max(int(width), 0), 3), dtype=np.float32)
    rc = _ffi.hip().rpt_raymap_fill(RAYMAP_KINDS[kind], params, int(width), int(height), dirs.ctypes.data)
    if rc != 0:
        raise ValueError(f"rpt_raymap_fill({kind!r}, fov={fov}, fit={fit}, {width}x{height}) failed ({rc})")
    return dirs


def _ypr(yaw: float, pitch: float, roll: float):
    return (C.c_float * 3)(float(yaw), float(pitch), float(roll))


def rotation_matrix(yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0) -> np.ndarray:
    """R = Ry(yaw) Rx(pitch) Rz(roll) of rpt_set_orientation (include/rpt.h), float64, from the angles rounded to float32 as the library
    takes them: a direction n of the turned camera is the direction R n of the un-turned one; the view direction is R (0, 0, 1)."""
    y, p, r = (float(np.float32(a)) for a in (yaw, pitch, roll))
    cy, sy, cp, sp, cr, sr = math.cos(y), math.sin(y), math.cos(p), math.sin(p), math.cos(r), math.sin(r)
    ry = np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
    rx = np.array([[1, 0, 0], [0, cp, sp], [0, -sp, cp]])
    rz = np.array([[cr, sr, 0], [-sr, cr, 0], [0, 0, 1]])
    return ry @ (rx @ rz)


def look_at(direction: Sequence[float], up: Sequence[float] = (0.0, 1.0, 0.0)) -> Tuple[float, float, float]:
    """(yaw, pitch, roll) for Renderer.set_orientation such that the view direction R (0, 0, 1) is `direction` (any non-zero length) and
    the image's up, R (0, 1, 0), is `up` made perpendicular to it.  Host arithmetic only.  At the poles (direction parallel to the y
    axis) the yaw is taken from `up` (for direction = +y: the yaw that puts -up in the image centre's forward half-plane, i.e. the way
    the head tilted back from); if `up` is parallel to `direction` as well, or zero, the yaw is 0 and the roll is 0."""
    d = np.asarray(direction, dtype=np.float64)
    n = float(np.linalg.norm(d))
    if not (n > 0.0 and math.isfinite(n)):
        raise ValueError("look_at: the direction must be finite and non-zero")
    d = d / n
    u = np.asarray(up, dtype=np.float64)
    u = u - d * float(u @ d)                       # up, perpendicular to the view
    un = float(np.linalg.norm(u))
    pitch = math.asin(max(-1.0, min(1.0, float(d[1]))))
    horizontal = math.hypot(float(d[0]), float(d[2]))
    if horizontal > 1e-12:
        yaw = math.atan2(float(d[0]), float(d[2]))
    elif un > 1e-12:                               # a pole: with roll 0, R (0, 1, 0) = (-sin yaw sin pitch, cos pitch, -cos yaw sin pitch)
        sgn = 1.0 if d[1] > 0 else -1.0
        yaw = math.atan2(-sgn * float(u[0]), -sgn * float(u[2]))
    else:
        yaw = 0.0
    if un <= 1e-12:
        return yaw, pitch, 0.0
    u = u / un
    # roll: R (0, 1, 0) = cos(roll) e_up + sin(roll) e_right, e_up / e_right the image's up / right at roll 0
    r0 = rotation_matrix(yaw, pitch, 0.0)
    roll = math.atan2(float(u @ r0[:, 0]), float(u @ r0[:, 1]))
    return yaw, pitch, roll


def orient_objects(objects, yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0) -> np.ndarray:
    """rpt_orient_objects (host code, no device needed): the Object[] a context with set_orientation(yaw, pitch, roll) renders — Lorentz and
    InvLorentz re-based to the turned camera frame, every other byte copied.  objects: a Scene or n x 320 bytes; returns uint8 (n, 320)."""
    if isinstance(objects, Scene):
        d = objects.desc()
        raw = np.ctypeslib.as_array(C.cast(d.objects, C.POINTER(C.c_uint8)), shape=(int(d.object_count) * 320,)).copy() if d.object_count else np.zeros(0, np.uint8)
    else:
        raw = np.ascontiguousarray(objects).view(np.uint8).reshape(-1).copy()
    if raw.size % 320:
        raise ValueError("objects are 320 bytes each")
    out = np.empty_like(raw)
    rc = _ffi.hip().rpt_orient_objects(raw.ctypes.data, raw.size // 320, _ypr(yaw, pitch, roll), out.ctypes.data)
    if rc != 0:
        raise ValueError(f"rpt_orient_objects({yaw}, {pitch}, {roll}) failed ({rc})")
    return out.reshape(-1, 320)


def orient_matrix(matrix, yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0) -> np.ndarray:
    """rpt_orient_matrix: E diag(1, R) for a 4 x 4 matrix of Object.Lorentz's layout (the sky's frame as a turned context uses it)."""
    m = np.ascontiguousarray(matrix, dtype=np.float32).reshape(16).copy()
    out = np.empty(16, dtype=np.float32)
    fp = C.POINTER(C.c_float)
    rc = _ffi.hip().rpt_orient_matrix(m.ctypes.data_as(fp), _ypr(yaw, pitch, roll), out.ctypes.data_as(fp))
    if rc != 0:
        raise ValueError(f"rpt_orient_matrix({yaw}, {pitch}, {roll}) failed ({rc})")
    return out.reshape(4, 4)


class Renderer:
    def __init__(self, device: int = 0, diag: bool = False):
        self._lib = _ffi.hip_diag() if diag else _ffi.hip()      # diag: librpt_hip_diag.so (measurement arms; tools and tests only)
        h = C.c_void_p()
        rc = self._lib.rpt_create(C.byref(h), int(device))
        if rc != 0 or not h:
            raise RenderError(f"rpt_create(device={device}) failed with status {rc}: no usable gfx950 device "
                              "(the render path has no CPU fallback)")
        self._h = h
        self.device = device
        self.width = self.height = 0
        self._rows = (0, 1, False)
        self._events_size = None             # (width, height) of the last event frame: what read_events shapes its result by
        self._run = 1

    def close(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._lib.rpt_destroy(h)

    __del__ = close

    def _check(self, rc: int, what: str):
        if rc != 0:
            e = RenderError(f"{what} failed ({rc}): {self._lib.rpt_last_error(self._h).decode()}")
            e.code = int(rc)
            raise e

    # -- reference enqueue sequence ------------------------------------------------------------
    def upload_scene(self, scene: Scene):
        d = scene.desc()
        self._check(self._lib.rpt_upload_scene(self._h, C.byref(d)), "rpt_upload_scene")

    def share_scene(self, owner: "Renderer"):
        """Use the scene resident in `owner` (same device) instead of uploading a second copy: frames in flight."""
        self._check(self._lib.rpt_share_scene(self._h, owner._h), "rpt_share_scene")

    def upload_desc(self, desc: _ffi.SceneDesc):
        self._check(self._lib.rpt_upload_scene(self._h, C.byref(desc)), "rpt_upload_scene")

    def set_object_windows(self, windows):
        """Per-object time windows (include/rpt.h, rpt_set_object_windows): an (object_count, 2) array of {t0, t1} in each object's own
        rest frame — the object, as a surface, an occluder and a light, exists for t0 <= t < t1; -inf / +inf are the defaults — copied
        by the library.  None clears the setting.  Per context.  While set, the windowed kernels render (last_variant() >= 2000)."""
        self._scene_windows = None          # (what set_objects(scene) last passed on is no longer what the context holds)
        if windows is None:
            self._check(self._lib.rpt_set_object_windows(self._h, None, 0), "rpt_set_object_windows")
            return
        w = np.ascontiguousarray(windows, dtype=np.float32)
        if not (w.ndim == 2 and w.shape[1] == 2):
            raise ValueError(f"windows are an (object_count, 2) array, not {w.shape}")
        self._check(self._lib.rpt_set_object_windows(self._h, w.ctypes.data, int(w.shape[0])), "rpt_set_object_windows")

    def set_objects(self, scene_or_bytes):
        if isinstance(scene_or_bytes, Scene):
            d = scene_or_bytes.desc()
            self._check(self._lib.rpt_set_objects(self._h, d.objects, d.object_count), "rpt_set_objects")
            # the scene's `w` commands (Scene.windows() is cached by the scene): passed on when they are not what this call passed on
            # last — behind the objects, so that the upload the library repeats for them is of these objects — and cleared when a
            # scene without any follows one that had some.  Windows set by hand (set_object_windows) are left alone.
            w, last = scene_or_bytes.windows(), getattr(self, "_scene_windows", None)
            if w is None:
                if last is not None:
                    self.set_object_windows(None)
            elif last is None or not np.array_equal(w, last):
                self.set_object_windows(w)
                self._scene_windows = w
            # ... and the scene's `d` commands likewise (Scene.readouts() is cached by the scene too)
            d, last = scene_or_bytes.readouts(), getattr(self, "_scene_readouts", None)
            if d is None:
                if last is not None:
                    self.set_readouts(None)
            elif last is None or d != last:
                self.set_readouts(d)
                self._scene_readouts = d
        else:
            raw = np.ascontiguousarray(scene_or_bytes).view(np.uint8)
            assert raw.size % 320 == 0
            self._check(self._lib.rpt_set_objects(self._h, raw.ctypes.data, raw.size // 320), "rpt_set_objects")

    def set_params(self, white_point: Sequence[float], ambient: float, width: int, height: int, interval: int):
        wp = (C.c_float * 3)(*white_point)
        self._check(self._lib.rpt_set_params(self._h, wp, float(ambient), int(width), int(height), int(interval)),
                    "rpt_set_params")
        self.width, self.height = int(width), int(height)

    def set_scene_params(self, scene: Scene, width: int, height: int):
        p = scene.params
        self.set_params(p["white_point"], p["ambient"], width, height, p["interval"])

    def set_output(self, device_ptr: Optional[int]):
        self._check(self._lib.rpt_set_output(self._h, C.c_void_p(device_ptr or 0)), "rpt_set_output")

    def set_rows(self, first_tile: int = 0, tile_step: int = 1, colour_plane: bool = False):
        self._check(self._lib.rpt_set_rows(self._h, first_tile, tile_step, int(colour_plane)), "rpt_set_rows")
        self._rows = (first_tile, tile_step, colour_plane)
        self._run = 1

    def set_tile_pattern(self, first_tile: int, tile_step: int, run: int, colour_plane: bool = False):
        """Per period of `tile_step` tiles, the `run` (power of two) consecutive tiles from first_tile on (rpt_set_rows: run 1)."""
        self._check(self._lib.rpt_set_tile_pattern(self._h, first_tile, tile_step, run, int(colour_plane)), "rpt_set_tile_pattern")
        self._rows = (first_tile, tile_step, colour_plane)
        self._run = run

    def set_plane_output(self, device_ptr: Optional[int]):
        self._check(self._lib.rpt_set_plane_output(self._h, C.c_void_p(device_ptr or 0)), "rpt_set_plane_output")

    def set_stream(self, hip_stream: Optional[int]):
        self._check(self._lib.rpt_set_stream(self._h, C.c_void_p(hip_stream or 0)), "rpt_set_stream")

    def set_debug_rgb(self, enable: bool = True):
        self._check(self._lib.rpt_set_debug_rgb(self._h, C.c_void_p(1 if enable else 0)), "rpt_set_debug_rgb")

    def set_variant(self, variant: int):
        self._check(self._lib.rpt_set_variant(self._h, int(variant)), "rpt_set_variant")

    def set_msaa(self, samples_per_axis: int):
        """MSAASAMPLES of opencl_kernel.cl:7 (1 = the reference as shipped)."""
        self._check(self._lib.rpt_set_msaa(self._h, int(samples_per_axis)), "rpt_set_msaa")

    def set_adaptive_aa(self, samples: int, threshold: int = 8):
        """Adaptive anti-aliasing (include/rpt.h, rpt_set_adaptive_aa; not in the reference; off by default): colour frames are the
        one-sample frame with every pixel whose 8-bit colour differs from a 4-neighbour's by more than `threshold` in some channel
        rendered again with samples x samples rays.  samples = 1 switches it off; threshold -1 refines every pixel, 255 none (the
        default of 8 is a knob, not a claim; adaptive.refine_mask previews what a threshold selects).  Every camera and colour mode;
        what it cannot serve (set_msaa > 1, set_rows, the Doppler debug kernel, variants other than 0, 3, 41, 43, 44) refuses at the launch."""
        self._check(self._lib.rpt_set_adaptive_aa(self._h, int(samples), int(threshold)), "rpt_set_adaptive_aa")

    def last_aa_refined(self) -> int:
        """Pixels the refine pass of the last finished adaptive frame re-rendered (0 with the setting off)."""
        return self._last_counts("rpt_last_aa_refined")[0]

    def last_aa_variant(self) -> int:
        """The refine kernel (include/rpt.h, rpt_set_adaptive_aa) of the last colour frame; 0 if it had no refine pass."""
        return int(self._lib.rpt_last_aa_variant(self._h))

    def set_doppler(self, shift: bool = True, beaming: bool = True):
        """Relativistic Doppler shift and / or searchlight beaming (not in the reference; off by default).  set_doppler(False, False)
        turns it off again.  Kernels without a Doppler twin (variants 1, 50, 51, MSAA > 1) then refuse at the launch."""
        flags = (DOPPLER_SHIFT if shift else 0) | (DOPPLER_BEAMING if beaming else 0)
        self._check(self._lib.rpt_set_doppler(self._h, flags), "rpt_set_doppler")

    def set_projection(self, mode: str = "pinhole", h_fov: float = 2 * math.pi, v_fov: float = math.pi, yaw: float = 0.0):
        """The camera: "pinhole" (the reference's, the default), "equirect", a panorama of h_fov x v_fov radians centred on longitude
        yaw (0 = +z; include/rpt.h, rpt_set_projection), or "raymap", the directions of set_raymap (the angles are not used).  Per
        context.  In panorama only variants 0 and 3 render, at MSAA 1; under a ray map variants 0, 3, 41, 43 and 44, at MSAA 1."""
        m, params = _projection_args(mode, h_fov, v_fov, yaw)
        self._check(self._lib.rpt_set_projection(self._h, m, params), "rpt_set_projection")

    projection_tables = staticmethod(projection_tables)
    raymap = staticmethod(raymap)

    def set_raymap(self, dirs: Optional[np.ndarray], width: Optional[int] = None, height: Optional[int] = None):
        """The ray map (include/rpt.h, rpt_set_raymap): one direction per pixel, (H, W, 3) float32 with row 0 the bottom — or (H W, 3)
        with width and height given — copied by the library; (0, 0, 0) = the pixel has no ray and is written black.  None drops the
        map.  Per context; used while set_projection("raymap") is set, and its size must then be the frame's at every launch."""
        if dirs is None:
            self._check(self._lib.rpt_set_raymap(self._h, None, 0, 0), "rpt_set_raymap")
            return
        d = np.ascontiguousarray(dirs, dtype=np.float32)
        if d.ndim == 3 and d.shape[2] == 3 and width is None and height is None:
            height, width = d.shape[0], d.shape[1]
        elif not (d.ndim == 2 and d.shape[1] == 3 and width is not None and height is not None and d.shape[0] == int(width) * int(height)):
            raise ValueError(f"a ray map is an (H, W, 3) array, or an (H W, 3) array with width and height given, not {d.shape}")
        self._check(self._lib.rpt_set_raymap(self._h, d.ctypes.data, int(width), int(height)), "rpt_set_raymap")

    def set_orientation(self, yaw: float = 0.0, pitch: float = 0.0, roll: float = 0.0):
        """Turn the camera: R = Ry(yaw) Rx(pitch) Rz(roll) in radians, the view direction R (0, 0, 1) — positive yaw towards +x, positive
        pitch towards +y, positive roll turns the image counter-clockwise (include/rpt.h, rpt_set_orientation).  Per context, every
        projection and kernel; takes effect at the next launch.  Three zeros: the reference's camera again."""
        self._check(self._lib.rpt_set_orientation(self._h, _ypr(yaw, pitch, roll)), "rpt_set_orientation")

    def set_field_of_view(self, v_fov: float = 0.0):
        """The pinhole's vertical field of view in radians, 0.01 .. 3.0; 0 = the reference's lens (90 degrees, the default).  Pinhole only,
        MSAA 1, variants 0, 3, 41, 43, 44: anything else refuses at the launch (include/rpt.h, rpt_set_field_of_view)."""
        self._check(self._lib.rpt_set_field_of_view(self._h, float(v_fov)), "rpt_set_field_of_view")

    def look_at(self, direction: Sequence[float], up: Sequence[float] = (0.0, 1.0, 0.0)) -> Tuple[float, float, float]:
        """set_orientation(*look_at(direction, up)); returns the angles."""
        ypr = look_at(direction, up)
        self.set_orientation(*ypr)
        return ypr

    orient_objects = staticmethod(orient_objects)

    def set_environment(self, image: Optional[np.ndarray]):
        """The sky: an equirectangular H x W x 3 uint8 image (row 0 the top), copied by the library; None switches it off (the constant
        background again).  Per context.  Seen through the matrix of set_environment_frame (include/rpt.h, rpt_set_environment)."""
        if image is None:
            self._check(self._lib.rpt_set_environment(self._h, None, 0, 0), "rpt_set_environment")
            return
        img = np.ascontiguousarray(image)
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != 3:
            raise ValueError(f"the environment is an H x W x 3 uint8 array, not {img.dtype} {img.shape}")
        self._check(self._lib.rpt_set_environment(self._h, img.ctypes.data, int(img.shape[1]), int(img.shape[0])), "rpt_set_environment")

    def set_environment_frame(self, matrix=None):
        """E, the 4 x 4 Lorentz matrix from the camera frame to the sky's rest frame (rows t, x, y, z); None = the identity.  For a sky
        at rest in the scene's frame: Scene.camera_lorentz()[1], every frame."""
        if matrix is None:
            self._check(self._lib.rpt_set_environment_frame(self._h, None), "rpt_set_environment_frame")
            return
        m = np.ascontiguousarray(matrix, dtype=np.float32)
        if m.size != 16:
            raise ValueError("the environment frame is a 4 x 4 matrix")
        self._check(self._lib.rpt_set_environment_frame(self._h, m.ctypes.data_as(C.POINTER(C.c_float))), "rpt_set_environment_frame")

    def set_debug_doppler(self, enable: bool = True):
        """While enabled (and Doppler is on) frames come from the Doppler debug kernel, which writes the per-pixel record."""
        self._check(self._lib.rpt_set_debug_doppler(self._h, C.c_void_p(1 if enable else 0)), "rpt_set_debug_doppler")

    def read_debug_doppler(self) -> np.ndarray:
        """(H, W, 11) float32: D_cam, D of the first contributing light, reference colour rgb, colour after the light factors rgb,
        final linear colour rgb (include/rpt.h, rpt_set_debug_doppler); all zero on a miss pixel."""
        out = np.empty((self.height, self.width, DOPPLER_RECORD), dtype=np.float32)
        self._check(self._lib.rpt_read_debug_doppler(self._h, out.ctypes.data, out.nbytes), "rpt_read_debug_doppler")
        return out

    def last_variant(self) -> int:
        """The kernel variant (include/rpt.h) the last launch of this context was made with: what variant 0 resolved to."""
        return int(self._lib.rpt_last_variant(self._h))

    def last_exact_rcp(self) -> bool:
        """Whether the last launch's triangle test took 1 / det through the exact reciprocal (kernels 41 / 43 on a scene in its domain)."""
        return bool(self._lib.rpt_last_exact_rcp(self._h))

    def last_sky_split(self) -> Optional[Tuple[int, int, int, int]]:
        """The box of 8x8 tiles (x0, y0, x1, y1; x1 and y1 exclusive) the last launch's own kernel ran over when the frame was a sky
        split — a fill wrote every pixel outside it (include/rpt.h, rpt_last_sky_split) — or None: one launch over the whole frame."""
        box = (C.c_int * 4)()
        return tuple(int(v) for v in box) if self._lib.rpt_last_sky_split(self._h, box) else None

    def verify_frame(self) -> int:
        """Pixels whose packed colour differs between the kernel a frame would get and the un-culled kernel (0 = the culls changed nothing)."""
        n = C.c_uint64(0)
        self._check(self._lib.rpt_verify_frame(self._h, C.byref(n)), "rpt_verify_frame")
        return int(n.value)

    def render(self):
        self._check(self._lib.rpt_render(self._h), "rpt_render")

    def render_async(self):
        self._check(self._lib.rpt_render_async(self._h), "rpt_render_async")

    def sync(self):
        self._check(self._lib.rpt_sync(self._h), "rpt_sync")

    def _run_pass(self, call: str, async_: bool):
        """One pass over the rendered frame: `call` of include/rpt.h, or with async_ its _async form, which enqueues only."""
        name = call + "_async" if async_ else call
        self._check(getattr(self._lib, name)(self._h), name)

    def _last_counts(self, call: str, n: int = 1) -> Tuple[int, ...]:
        """The n 64-bit counts a rpt_last_* call reports of its pass."""
        counts = (C.c_uint64 * n)()
        self._check(getattr(self._lib, call)(self._h, counts), call)
        return tuple(int(c) for c in counts)

    def _set_records(self, call: str, records, record, what: str):
        """The records of a splat pass for its rpt_set_* call: an array with one `record` (a ctypes structure of _ffi) per entry; None
        or an empty one switches the pass off.  Another size raises ValueError(what)."""
        if records is None or len(records) == 0:
            self._check(getattr(self._lib, call)(self._h, None, 0), call)
            return
        raw = np.ascontiguousarray(records)
        size = C.sizeof(record)
        if raw.nbytes % size or raw.nbytes // size != len(raw):
            raise ValueError(what)
        self._check(getattr(self._lib, call)(self._h, C.cast(raw.ctypes.data, C.POINTER(record)), len(raw)), call)

    def _set_measurement(self, call: str, timed: bool):
        """A rpt_set_*_measurement call: time the two kernels of every pass, or no longer."""
        self._check(getattr(self._lib, call)(self._h, int(bool(timed))), call)

    def _last_ms(self, call: str) -> Tuple[float, float]:
        """The (splat, resolve) device milliseconds a rpt_last_*_ms call reports of its last pass."""
        ms = (C.c_float * 2)(0.0, 0.0)
        self._check(getattr(self._lib, call)(self._h, ms), call)
        return float(ms[0]), float(ms[1])

    # -- the event pass (include/rpt.h, rpt_render_events; not in the reference) ------------------
    def set_events_output(self, device_ptr: Optional[int]):
        """The record buffer of the event pass: a device pointer to width * height * 32 B, or None for a library-owned one."""
        self._check(self._lib.rpt_set_events_output(self._h, C.c_void_p(device_ptr or 0)), "rpt_set_events_output")

    def render_events(self, async_: bool = False) -> Optional[np.ndarray]:
        """One event frame with the context's current objects, params, rows, projection, orientation and lens: per pixel the object
        hit (-1 = none), the distance, the emission event in the hit object's rest frame and the surface (u, v).  Blocking: returns the
        (H, W) array of EVENT_DTYPE (row 0 = the bottom row).  async_=True: enqueues only and returns None (sync, then read_events)."""
        if async_:
            self._check(self._lib.rpt_render_events_async(self._h), "rpt_render_events_async")
            self._events_size = (self.width, self.height)
            return None
        self._check(self._lib.rpt_render_events(self._h), "rpt_render_events")
        self._events_size = (self.width, self.height)
        return self.read_events()

    def read_events(self) -> np.ndarray:
        """The last event frame's records, (H, W) of EVENT_DTYPE with W and H as they were when that frame was rendered (set_scene_params
        since then does not change them); rows that are not this context's hold what the buffer held."""
        width, height = self._events_size or (self.width, self.height)      # (before the first pass the call refuses: RPT_ERR_STATE)
        out = np.empty((height, width), dtype=EVENT_DTYPE)
        self._check(self._lib.rpt_read_events(self._h, out.ctypes.data, out.nbytes), "rpt_read_events")
        return out

    def pick(self, x: int, y: int) -> np.void:
        """One record of the last event frame (rpt_pick): pixel (x, y), y counted from the bottom row."""
        out = np.zeros(1, dtype=EVENT_DTYPE)
        self._check(self._lib.rpt_pick(self._h, int(x), int(y), out.ctypes.data), "rpt_pick")
        return out[0]

    def last_events_variant(self) -> int:
        """The event kernel (include/rpt.h, rpt_render_events) the last event pass ran with; 0 before the first one."""
        return int(self._lib.rpt_last_events_variant(self._h))

    def last_events_exact_rcp(self) -> bool:
        """Whether the last event pass's triangle test took 1 / det through the exact reciprocal (941 / 911 / 921 on a scene in its domain)."""
        exact = C.c_int(0)
        self._check(self._lib.rpt_last_events_exact_rcp(self._h, C.byref(exact)), "rpt_last_events_exact_rcp")
        return bool(exact.value)

    # -- the overlay pass (include/rpt.h, rpt_set_overlay; not in the reference) -------------------
    def set_overlay(self, **layers):
        """The layers of the overlay pass, as keywords (events.overlay_settings): outlines=True, outline_rgba=(R, G, B, A);
        delay_step=..., delay_rgba; clock_step=..., clock_rgba; lattice_step=one step or (sx, sy, sz), lattice_rgba; tint=True,
        tint_t_max (0 = the frame's largest delay, found on the device), tint_alpha.  No keyword at all switches the pass off.  A
        description the library refuses (a step <= 0 for a layer that is on, ...) raises RenderError."""
        from .events import overlay_settings
        s = overlay_settings(**layers)
        d = _ffi.OverlayDesc()
        d.layers = s["layers"]
        d.delay_step = s["delay_step"] if s["delay_step"] is not None else 0.0
        d.clock_step = s["clock_step"] if s["clock_step"] is not None else 0.0
        d.lattice_step[:] = s["lattice_step"] if s["lattice_step"] is not None else (0.0, 0.0, 0.0)
        d.tint_t_max = s["tint_t_max"]
        d.outline_rgba[:], d.delay_rgba[:], d.clock_rgba[:], d.lattice_rgba[:] = s["outline_rgba"], s["delay_rgba"], s["clock_rgba"], s["lattice_rgba"]
        d.tint_alpha = int(s["tint_alpha"])
        self._check(self._lib.rpt_set_overlay(self._h, C.byref(d) if s["layers"] else None), "rpt_set_overlay")

    def render_overlay(self, async_: bool = False):
        """Blend the layers of set_overlay into the framebuffer, in place, from the records of the last event frame.  The context must
        have rendered (or enqueued) a colour frame and an event frame of the current view first; calling it twice blends twice.
        async_=True enqueues only (sync waits)."""
        self._run_pass("rpt_render_overlay", async_)

    def last_overlay_pixels(self) -> int:
        """Pixels whose RGBA the last finished overlay pass changed (0 before the first)."""
        return self._last_counts("rpt_last_overlay_pixels")[0]

    # -- the readout pass (include/rpt.h, rpt_set_readouts; not in the reference) ------------------
    def set_readouts(self, readouts):
        """The objects' displays: a list with one entry per object of the scene, None (no display) or a dict of the keywords of
        events.readout_settings — rate, offset, digits, decimals, rect=(u0, v0, u1, v1), on_rgba, off_rgba; the display shows
        offset + rate * the object's own time (event[0] of the event pass) of the light each pixel receives.  None or an empty list
        clears the setting.  An unknown keyword raises TypeError; what the library refuses raises RenderError.  Per context; copied to the device here, not per frame."""
        self._scene_readouts = None         # (what set_objects(scene) last passed on is no longer what the context holds)
        if not readouts:
            self._check(self._lib.rpt_set_readouts(self._h, None, 0), "rpt_set_readouts")
            return
        raw = (_ffi.Readout * len(readouts))()
        for r, d in zip(raw, readouts):
            if d is None:
                continue
            d = dict(d)
            unknown = set(d) - {"rate", "offset", "digits", "decimals", "rect", "on_rgba", "off_rgba"}
            if unknown:                     # (a misspelt key would silently leave the object without a display)
                raise TypeError(f"unknown readout keyword(s): {sorted(unknown)}")
            r.rate, r.offset, r.digits, r.decimals = d.get("rate", 1.0), d.get("offset", 0.0), d.get("digits", 0), d.get("decimals", 0)
            r.u0, r.v0, r.u1, r.v1 = d.get("rect", (0.1, 0.25, 0.9, 0.75))
            r.on_rgba[:], r.off_rgba[:] = d.get("on_rgba", (255, 0, 0, 255)), d.get("off_rgba", (0, 0, 0, 160))
        self._check(self._lib.rpt_set_readouts(self._h, raw, len(readouts)), "rpt_set_readouts")

    def render_readouts(self, async_: bool = False):
        """Draw the displays of set_readouts into the framebuffer, in place, from the records of the last event frame.  The context must
        have rendered (or enqueued) a colour frame and an event frame of the current view first; calling it twice blends twice.
        Independent of render_overlay: either may run first.  async_=True enqueues only (sync waits)."""
        self._run_pass("rpt_render_readouts", async_)

    def last_readout_pixels(self) -> int:
        """Pixels whose RGBA the last finished readout pass changed (0 before the first)."""
        return self._last_counts("rpt_last_readout_pixels")[0]

    # -- the star-field pass (include/rpt.h, rpt_set_stars; not in the reference) -------------------
    def set_stars(self, catalogue, temperatures=None):
        """The star catalogue: an array of stars.STAR_DTYPE records (or anything of n x 32 bytes in that layout: dir, rgb, two floats of
        padding), e.g. from stars.random_catalogue / stars.from_arrays / stars.load; None or an empty array switches the pass off.
        dir is the direction one looks in to see the star, in the sky's rest frame (set_environment_frame); rgb its linear colour at
        rest.  Copied by the library; per context; what the library refuses raises RenderError.  temperatures: if given, passed to
        set_star_temperatures after the catalogue (None leaves the temperatures of the context as they are)."""
        if temperatures is not None:
            self.set_stars(catalogue)
            self.set_star_temperatures(temperatures)
            return
        self._set_records("rpt_set_stars", catalogue, _ffi.Star, "a star catalogue has one 32-byte record (stars.STAR_DTYPE) per star")

    def _set_temperatures(self, call: str, kelvin):
        if kelvin is None or len(kelvin) == 0:
            self._check(getattr(self._lib, call)(self._h, None, 0), call)
            return
        raw = np.ascontiguousarray(kelvin, dtype=np.float32).reshape(-1)
        self._check(getattr(self._lib, call)(self._h, raw.ctypes.data_as(C.POINTER(C.c_float)), len(raw)), call)

    def set_star_temperatures(self, kelvin):
        """Thermal stars (include/rpt.h, rpt_set_star_temperatures): one temperature in kelvin per star of the catalogue,
        in its order — 0 for a star that keeps the piecewise-linear spectrum, otherwise 500 .. 1e8.  With the Doppler shift on, a star
        with a temperature is shifted as a blackbody (at D it is one of D T) and is never moved out of the band.  None or an empty
        array switches the thermal law off.  Kept when the catalogue is replaced; render_stars refuses a count that differs from the
        catalogue's."""
        self._set_temperatures("rpt_set_star_temperatures", kelvin)

    def render_stars(self, async_: bool = False):
        """Add the stars of set_stars to the miss pixels of the framebuffer, in place.  The context must have rendered (or enqueued) a
        colour frame and an event frame of the current view first; calling it twice adds them twice.  Independent of render_overlay and
        render_readouts.  async_=True enqueues only (sync waits)."""
        self._run_pass("rpt_render_stars", async_)

    def last_stars(self) -> Tuple[int, int]:
        """(stars with at least one tap inside the frame, pixels whose bytes changed) of the last finished star-field pass."""
        inside, changed = self._last_counts("rpt_last_stars", 2)
        return inside, changed

    def set_stars_measurement(self, timed: bool = False):
        """Measurement only (tools/stars_cost.py): time the two kernels of every pass (last_stars_ms)."""
        self._set_measurement("rpt_set_stars_measurement", timed)

    def last_stars_ms(self) -> Tuple[float, float]:
        """(splat, resolve) device milliseconds of the last pass, which must have been timed (set_stars_measurement)."""
        return self._last_ms("rpt_last_stars_ms")

    # -- the particle pass (include/rpt.h, rpt_set_particles; not in the reference) -----------------
    def set_particles(self, particles, temperatures=None):
        """The particle set: an array of particles.PARTICLE_DTYPE records (or anything of n x 32 bytes in that layout: pos, object,
        rgb, one float of padding), e.g. from particles.lattice / particles.at_events / particles.load; None or an empty array switches
        the pass off.  pos is the position in the rest frame of the scene's object number `object` (the coordinates of an event
        record's event[1..3]); rgb the linear colour at rest.  Copied by the library; per context; what the library refuses raises
        RenderError.  temperatures: if given, passed to set_particle_temperatures after the set (None leaves the temperatures of the
        context as they are)."""
        if temperatures is not None:
            self.set_particles(particles)
            self.set_particle_temperatures(temperatures)
            return
        self._set_records("rpt_set_particles", particles, _ffi.Particle, "a particle set has one 32-byte record (particles.PARTICLE_DTYPE) per particle")

    def set_particle_temperatures(self, kelvin):
        """Thermal particles (rpt_set_particle_temperatures): as set_star_temperatures, one temperature per particle of the set."""
        self._set_temperatures("rpt_set_particle_temperatures", kelvin)

    def set_particle_options(self, inverse_square: bool = False, depth_bias: float = 0.0):
        """inverse_square: divide a particle's colour by its squared rest-frame distance (rgb is then an intensity, not what a pixel
        gets).  depth_bias >= 0, in units of the records' dist: a tap is drawn where dist - depth_bias < the record's dist, so a
        particle ON a surface (particles.at_events) shows with a small bias and is hidden, by rounding, without one."""
        self._check(self._lib.rpt_set_particle_options(self._h, 1 if inverse_square else 0, float(depth_bias)), "rpt_set_particle_options")

    def set_particle_lighting(self, lit: bool = False, shadows: bool = False, ambient: bool = False):
        """Lit particles (include/rpt.h, rpt_set_particle_lighting): dust.  lit: a particle's rgb is an albedo, and its
        colour at rest is what it scatters from the scene's lights — with light delay on the light -> grain leg too, the light's
        Doppler factor and its time window (set_object_windows: a lamp switched on shows its front expanding through the dust).
        shadows: a shadow ray per (grain, light), the one the renderer shoots for a surface.  ambient: add rgb * ambient, as a surface
        gets it.  shadows and ambient need lit; the default, all off, is the self-luminous pass.  With light propagation off
        (interval 0) the scene lights nothing and a lit pass equals the plain one."""
        flags = (1 if lit else 0) | (2 if shadows else 0) | (4 if ambient else 0)      # RPT_PARTICLES_LIT, _SHADOWED, _AMBIENT
        self._check(self._lib.rpt_set_particle_lighting(self._h, flags), "rpt_set_particle_lighting")

    def last_particle_lighting(self) -> Tuple[int, int]:
        """((particle, light) pairs that lit, pairs a shadow ray found occluded) of the last finished particle pass, over the particles
        last_particles counts as seen; (0, 0) for a pass that was not lit."""
        lit, shadowed = self._last_counts("rpt_last_particle_lighting", 2)
        return lit, shadowed

    def render_particles(self, async_: bool = False):
        """Add the particles of set_particles to the framebuffer, in place, each tap depth-tested against the last event frame.  The
        context must have rendered (or enqueued) a colour frame and an event frame of the current view first; calling it twice adds them
        twice.  Independent of the other passes.  async_=True enqueues only (sync waits)."""
        self._run_pass("rpt_render_particles", async_)

    def last_particles(self) -> Tuple[int, int]:
        """(particles with at least one tap inside the frame that passed the depth test, pixels whose bytes changed) of the last
        finished particle pass."""
        seen, changed = self._last_counts("rpt_last_particles", 2)
        return seen, changed

    def set_particles_measurement(self, timed: bool = False):
        """Measurement only (tools/particles_cost.py): time the two kernels of every pass (last_particles_ms)."""
        self._set_measurement("rpt_set_particles_measurement", timed)

    def last_particles_ms(self) -> Tuple[float, float]:
        """(splat, resolve) device milliseconds of the last pass, which must have been timed (set_particles_measurement)."""
        return self._last_ms("rpt_last_particles_ms")

    # -- the segment pass (include/rpt.h, rpt_set_segments; not in the reference) -------------------
    def set_segments(self, segments):
        """The rods: an array of segments.SEGMENT_DTYPE records (or anything of n x 48 bytes in that layout: a, object, b, padding, rgb,
        padding), e.g. from segments.box_edges / segments.rod_lattice / segments.polyline / segments.load; None or an empty array
        switches the pass off.  a and b are the ends in the rest frame of the scene's object number `object`; rgb is the linear colour
        at rest PER UNIT REST-FRAME LENGTH.  Copied by the library; per context; what the library refuses raises RenderError."""
        self._set_records("rpt_set_segments", segments, _ffi.Segment, "a segment set has one 48-byte record (segments.SEGMENT_DTYPE) per rod")

    def set_segment_options(self, inverse_square: bool = False, depth_bias: float = 0.0, pieces: int = 16):
        """inverse_square, depth_bias: as set_particle_options, for every element of a rod.  pieces: 1, 2, 4, ..., 64 — the parts a rod is
        cut into; its pieces + 1 nodes are placed exactly, between them the image is a chord.  count x pieces may not exceed 2^21."""
        self._check(self._lib.rpt_set_segment_options(self._h, 1 if inverse_square else 0, float(depth_bias), int(pieces)), "rpt_set_segment_options")

    def render_segments(self, async_: bool = False):
        """Add the rods of set_segments to the framebuffer, in place, each tap depth-tested against the last event frame.  The context
        must have rendered (or enqueued) a colour frame and an event frame of the current view first; calling it twice adds them twice.
        Independent of the other passes.  async_=True enqueues only (sync waits)."""
        self._run_pass("rpt_render_segments", async_)

    def last_segments(self) -> Tuple[int, int]:
        """(pieces with at least one tap inside the frame that passed the depth test, pixels whose bytes changed) of the last finished
        segment pass."""
        drawn, changed = self._last_counts("rpt_last_segments", 2)
        return drawn, changed

    def set_segments_measurement(self, timed: bool = False):
        """Measurement only (tools/segments_cost.py): time the two kernels of every pass (last_segments_ms)."""
        self._set_measurement("rpt_set_segments_measurement", timed)

    def last_segments_ms(self) -> Tuple[float, float]:
        """(splat, resolve) device milliseconds of the last pass, which must have been timed (set_segments_measurement)."""
        return self._last_ms("rpt_last_segments_ms")

    # -- the ballistic pass (include/rpt.h, rpt_set_ballistics; not in the reference) ----------------
    def set_ballistics(self, ballistics, temperatures=None):
        """Point sources with a velocity of their own: an array of ballistics.BALLISTIC_DTYPE records (or anything of n x 48 bytes in
        that layout: pos, object, rgb, t0, u, t1), e.g. from ballistics.from_arrays / ballistics.jet / ballistics.shell /
        ballistics.load; None or an empty array switches the pass off.  pos is where the particle is at time 0 of the rest-frame clock
        of the scene's object number `object`, u its proper velocity gamma * beta in that frame, [t0, t1) the window of that clock in
        which it shines, rgb the linear colour at rest in the particle's own frame.  Copied by the library; per context; what the
        library refuses raises RenderError.  temperatures: if given, passed to set_ballistic_temperatures after the set."""
        if temperatures is not None:
            self.set_ballistics(ballistics)
            self.set_ballistic_temperatures(temperatures)
            return
        self._set_records("rpt_set_ballistics", ballistics, _ffi.Ballistic, "a ballistic set has one 48-byte record (ballistics.BALLISTIC_DTYPE) per particle")

    def set_ballistic_temperatures(self, kelvin):
        """Thermal ballistic particles (rpt_set_ballistic_temperatures): as set_star_temperatures, one temperature per record of the set."""
        self._set_temperatures("rpt_set_ballistic_temperatures", kelvin)

    def set_ballistic_options(self, inverse_square: bool = False, depth_bias: float = 0.0):
        """As set_particle_options, for the ballistic pass alone; inverse_square divides by the squared distance of the camera in the
        PARTICLE's rest frame."""
        self._check(self._lib.rpt_set_ballistic_options(self._h, 1 if inverse_square else 0, float(depth_bias)), "rpt_set_ballistic_options")

    def render_ballistics(self, async_: bool = False):
        """Add the particles of set_ballistics to the framebuffer, in place, each tap depth-tested against the last event frame.  The
        context must have rendered (or enqueued) a colour frame and an event frame of the current view first; calling it twice adds them
        twice.  Independent of the other passes.  async_=True enqueues only (sync waits)."""
        self._run_pass("rpt_render_ballistics", async_)

    def last_ballistics(self) -> Tuple[int, int]:
        """(records with at least one tap inside the frame that passed the depth test, pixels whose bytes changed) of the last finished
        ballistic pass."""
        seen, changed = self._last_counts("rpt_last_ballistics", 2)
        return seen, changed

    def set_ballistics_measurement(self, timed: bool = False):
        """Measurement only (tools/ballistics_cost.py): time the two kernels of every pass (last_ballistics_ms)."""
        self._set_measurement("rpt_set_ballistics_measurement", timed)

    def last_ballistics_ms(self) -> Tuple[float, float]:
        """(splat, resolve) device milliseconds of the last pass, which must have been timed (set_ballistics_measurement)."""
        return self._last_ms("rpt_last_ballistics_ms")

    # -- glare for the point-source passes (include/rpt.h, rpt_set_glare; not in the reference) ------
    def set_glare(self, layers=None):
        """A point-spread function for the stars, the particles, the segments, the ballistic records and the rockets:
        a list of up to three (weight, sigma) layers, e.g. glare.preset("soft"); sigma in pixels, in [0.5, 32/3], every weight > 0 and
        their sum <= 1 (the rest stays in the source's own pixel).  From the next pass on, each of those passes spreads what it has
        summed before it tonemaps, so a brighter source looks bigger.  None or [] switches glare off, which is the default: the passes
        then launch the kernels they always did.  glare.apply is the same arithmetic on the host."""
        layers = [] if layers is None else [(float(w), float(s)) for w, s in layers]
        if len(layers) > 3:
            raise ValueError(f"glare has at most 3 layers, {len(layers)} were given")
        desc = _ffi.Glare()
        desc.layers = len(layers)
        for k, (w, s) in enumerate(layers):
            desc.weight[k], desc.sigma[k] = w, s
        self._check(self._lib.rpt_set_glare(self._h, C.byref(desc) if layers else None), "rpt_set_glare")

    # -- the rocket pass (include/rpt.h, rpt_set_rockets; not in the reference) ----------------------
    def set_rockets(self, rockets, temperatures=None):
        """Point sources under constant proper acceleration: an array of rockets.ROCKET_DTYPE records (or anything of n x 64 bytes in
        that layout: pos, object, rgb, t0, u, t1, acc, reserved), e.g. from rockets.from_arrays / rockets.launch / rockets.fleet /
        rockets.trip / rockets.load; None or an empty array switches the pass off.  pos, object, rgb, u and [t0, t1) as in
        set_ballistics; acc is the proper acceleration the crew feels, in the rocket's own rest frame at the object's time 0.  Copied by
        the library; per context; what the library refuses raises RenderError.  temperatures: if given, passed to
        set_rocket_temperatures after the set."""
        if temperatures is not None:
            self.set_rockets(rockets)
            self.set_rocket_temperatures(temperatures)
            return
        self._set_records("rpt_set_rockets", rockets, _ffi.Rocket, "a rocket set has one 64-byte record (rockets.ROCKET_DTYPE) per rocket")

    def set_rocket_temperatures(self, kelvin):
        """Thermal rockets (rpt_set_rocket_temperatures): as set_star_temperatures, one temperature per record of the set."""
        self._set_temperatures("rpt_set_rocket_temperatures", kelvin)

    def set_rocket_options(self, inverse_square: bool = False, depth_bias: float = 0.0):
        """As set_ballistic_options, for the rocket pass alone; inverse_square divides by the squared distance of the camera in the
        ROCKET's rest frame at emission."""
        self._check(self._lib.rpt_set_rocket_options(self._h, 1 if inverse_square else 0, float(depth_bias)), "rpt_set_rocket_options")

    def render_rockets(self, async_: bool = False):
        """Add the rockets of set_rockets to the framebuffer, in place, each tap depth-tested against the last event frame.  The
        context must have rendered (or enqueued) a colour frame and an event frame of the current view first; calling it twice adds them
        twice.  Independent of the other passes.  async_=True enqueues only (sync waits)."""
        self._run_pass("rpt_render_rockets", async_)

    def last_rockets(self) -> Tuple[int, int]:
        """(records with at least one tap inside the frame that passed the depth test, pixels whose bytes changed) of the last finished
        rocket pass."""
        seen, changed = self._last_counts("rpt_last_rockets", 2)
        return seen, changed

    def set_rockets_measurement(self, timed: bool = False):
        """Measurement only (tools/rockets_cost.py): time the two kernels of every pass (last_rockets_ms)."""
        self._set_measurement("rpt_set_rockets_measurement", timed)

    def last_rockets_ms(self) -> Tuple[float, float]:
        """(splat, resolve) device milliseconds of the last pass, which must have been timed (set_rockets_measurement)."""
        return self._last_ms("rpt_last_rockets_ms")

    # -- results -------------------------------------------------------------------------------
    def local_tiles(self) -> int:
        first, step, _ = self._rows
        tiles = (self.height + TILE_ROWS - 1) // TILE_ROWS
        if first >= tiles:
            return 0
        full, rest = divmod(tiles - first, step)
        return full * self._run + min(rest, self._run)

    def output_ptr(self) -> int:
        return self._lib.rpt_output_ptr(self._h) or 0

    def colour_plane_ptr(self) -> int:
        return self._lib.rpt_colour_plane_ptr(self._h) or 0

    def read_framebuffer(self) -> np.ndarray:
        """16 B/pixel framebuffer as a structured array [height*width] (row 0 = bottom row)."""
        out = np.empty(self.width * self.height, dtype=PIXEL_DTYPE)
        self._check(self._lib.rpt_read_framebuffer(self._h, out.ctypes.data, out.nbytes), "rpt_read_framebuffer")
        return out

    def read_colour_plane(self) -> np.ndarray:
        out = np.empty((self.local_tiles() * TILE_ROWS, self.width), dtype=np.uint32)
        self._check(self._lib.rpt_read_framebuffer(self._h, out.ctypes.data, out.nbytes), "rpt_read_framebuffer")
        return out

    def read_debug_rgb(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 3), dtype=np.float32)
        self._check(self._lib.rpt_read_debug_rgb(self._h, out.ctypes.data, out.nbytes), "rpt_read_debug_rgb")
        return out

    def last_frame_ms(self) -> float:
        ms = C.c_float()
        self._check(self._lib.rpt_last_frame_ms(self._h, C.byref(ms)), "rpt_last_frame_ms")
        return ms.value

    def timed_frames(self, frames: int) -> float:
        ms = C.c_float()
        self._check(self._lib.rpt_timed_frames(self._h, int(frames), C.byref(ms)), "rpt_timed_frames")
        return ms.value

    def scatter_colour_plane(self, planes_ptr: int, out16_ptr: int, width: int, height: int, n_ranks: int,
                             plane_stride_words: int, stream: Optional[int] = None):
        self._check(self._lib.rpt_scatter_colour_plane_on(self._h, C.c_void_p(stream or 0), C.c_void_p(planes_ptr),
                                                          C.c_void_p(out16_ptr), width, height, n_ranks, plane_stride_words),
                    "rpt_scatter_colour_plane")

    def pack_colour_plane3(self, plane4_ptr: int, plane3_ptr: int, pixels: int, stream: Optional[int] = None):
        """4 B/pixel colour plane -> 3 B/pixel (the alpha byte is the constant 1), on `stream` or the launch stream."""
        self._check(self._lib.rpt_pack_colour_plane3_on(self._h, C.c_void_p(stream or 0), C.c_void_p(plane4_ptr), C.c_void_p(plane3_ptr),
                                                        int(pixels)), "rpt_pack_colour_plane3_on")

    def scatter_helper_planes3(self, planes3_ptr: int, out16_ptr: int, width: int, height: int, n_ranks: int, root_run: int,
                               stride_bytes: int, stream: Optional[int] = None):
        self._check(self._lib.rpt_scatter_helper_planes3_on(self._h, C.c_void_p(stream or 0), C.c_void_p(planes3_ptr), C.c_void_p(out16_ptr),
                                                            width, height, n_ranks, root_run, int(stride_bytes)), "rpt_scatter_helper_planes3_on")

    def scatter_colour_plane3(self, planes3_ptr: int, out16_ptr: int, width: int, height: int, n_ranks: int, stride_bytes: int,
                              stream: Optional[int] = None):
        self._check(self._lib.rpt_scatter_colour_plane3_on(self._h, C.c_void_p(stream or 0), C.c_void_p(planes3_ptr), C.c_void_p(out16_ptr),
                                                           width, height, n_ranks, int(stride_bytes)), "rpt_scatter_colour_plane3_on")

    def read_counters(self):
        out = (C.c_uint64 * 16)()
        self._check(self._lib.rpt_read_counters(self._h, out), "rpt_read_counters")
        return list(out)

    def read_wave_times(self) -> np.ndarray:
        n = ((self.width + 31) // 32) * self.local_tiles() * 4 * 10
        out = np.zeros(n, dtype=np.uint64)
        got = C.c_size_t()
        self._check(self._lib.rpt_read_wave_times(self._h, out.ctypes.data, n, C.byref(got)), "rpt_read_wave_times")
        return out[:got.value].reshape(-1, 10)

    def build_octree(self, scene: Scene, first_triangle_word: int):
        """GPU octree build for the geometry `scene.ReadOBJ(..., octree=False)` just imported; appends it to the scene."""
        d = scene.desc()
        nodes, tris = C.c_void_p(), C.c_void_p()
        n_nodes, n_tris = C.c_size_t(), C.c_size_t()
        self._check(self._lib.rpt_build_octree(self._h, d.vertices, d.vertex_count, d.triangles, d.triangle_words,
                                               first_triangle_word, d.octree_count, d.octree_tri_count,
                                               C.byref(nodes), C.byref(n_nodes), C.byref(tris), C.byref(n_tris)),
                    "rpt_build_octree")
        try:
            scene.append_octree(nodes.value, n_nodes.value, tris.value, n_tris.value)
        finally:
            self._lib.rpt_free_host(nodes)
            self._lib.rpt_free_host(tris)

    def probe(self, which: int, inputs: np.ndarray, out_width: int) -> np.ndarray:
        """rpt_probe (include/rpt.h); which = 6: the Doppler colour operator, (n, 5) {D, r, g, b, flags} -> (n, 3); which = 8: the thermal
        point sources' operator, (n, 6) {D, r, g, b, flags, x_G} -> (n, 3)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.float32)
        n = inputs.shape[0]
        out = np.empty((n, out_width), dtype=np.float32)
        self._check(self._lib.rpt_probe(self._h, which, inputs.ctypes.data, out.ctypes.data, n), "rpt_probe")
        return out

    def probe_reciprocal(self, lo: float, hi: float, max_samples: int = 16):
        """rpt_probe_reciprocal (include/rpt.h): (counts[5], samples[max_samples, 2])."""
        counts = (C.c_uint64 * 5)()
        samples = np.zeros((max_samples, 2), dtype=np.float32)
        self._check(self._lib.rpt_probe_reciprocal(self._h, float(lo), float(hi), counts, samples.ctypes.data, max_samples), "rpt_probe_reciprocal")
        return [int(c) for c in counts], samples

    def probe_object(self, which: int, object_index: int, inputs: np.ndarray) -> np.ndarray:
        """rpt_probe_object (include/rpt.h): which = 0 (n, 8) rest-frame rays -> (n, 8); 1 (n, 9) shadow rays -> (n, 2) {un-culled, culled}
        occlusion; 2 (n, 4) vectors -> (n, 16) the four transforms; 3 (n, 3) camera directions -> (n, 8)."""
        inputs = np.ascontiguousarray(inputs, dtype=np.float32)
        n = inputs.shape[0]
        out = np.empty((n, {0: 8, 1: 2, 2: 16, 3: 8}[which]), dtype=np.float32)
        self._check(self._lib.rpt_probe_object(self._h, int(which), int(object_index), inputs.ctypes.data, out.ctypes.data, n), "rpt_probe_object")
        return out

    def mesh_segment_cull_record(self, object_index: int) -> np.ndarray:
        out = np.zeros(10, dtype=np.float32)
        self._check(self._lib.rpt_mesh_segment_cull_record(self._h, int(object_index), out.ctypes.data_as(C.POINTER(C.c_float))), "rpt_mesh_segment_cull_record")
        return out

    def probe_walk(self, object_index: int, rays: np.ndarray) -> np.ndarray:
        """rays (n, 6) = object-space origin and direction -> (n, 3, 8): {hit, dist, normal.xyz, uv.xy, 0} from the reference-layout
        walk, the throughput walk and the latency walk (include/rpt.h, rpt_probe_walk)."""
        rays = np.ascontiguousarray(rays, dtype=np.float32)
        n = rays.shape[0]
        out = np.empty((n, 3, 8), dtype=np.float32)
        self._check(self._lib.rpt_probe_walk(self._h, int(object_index), rays.ctypes.data, out.ctypes.data, n), "rpt_probe_walk")
        return out


def render_scene(scene: Scene, width: int, height: int, device: int = 0, debug_rgb: bool = False,
                 projection: Union[None, str, Mapping, np.ndarray] = None, environment: Optional[np.ndarray] = None,
                 orientation: Optional[Sequence[float]] = None, v_fov: Optional[float] = None, events: bool = False,
                 adaptive_aa: Optional[Tuple[int, int]] = None, overlay: Optional[Mapping] = None,
                 fov: float = math.pi, fit: int = 0, readouts=None, stars=None, particles=None,
                 particle_options: Optional[Mapping] = None, star_temperatures=None, particle_temperatures=None,
                 segments=None, segment_options: Optional[Mapping] = None, particle_lighting: Optional[Mapping] = None,
                 ballistics=None, ballistic_options: Optional[Mapping] = None, ballistic_temperatures=None,
                 rockets=None, rocket_options: Optional[Mapping] = None, rocket_temperatures=None, glare=None):
    """Convenience: upload, render one frame, read back. Returns (pixels, rgb-or-None), and with events=True (pixels, rgb-or-None,
    records): the (H, W) event records of the same view (Renderer.render_events).  projection: None (the pinhole), a mode name
    for Renderer.set_projection, or a mapping of its keyword arguments, e.g. {"mode": "equirect", "yaw": 1.0}; or a ray-map camera:
    "fisheye", "equisolid", "stereographic" (with fov, the full angle in radians, and fit: renderer.raymap) or "cube_strip" (width = 6
    height), or an (H, W, 3) float32 array of directions for Renderer.set_raymap.  environment: an
    H x W x 3 uint8 sky image at rest in the scene's frame (its frame is set from the scene's camera; call update_objects() first).
    orientation: (yaw, pitch, roll) for Renderer.set_orientation; v_fov: the pinhole's vertical field of view (set_field_of_view).
    adaptive_aa: (samples per axis, threshold) for Renderer.set_adaptive_aa.  overlay: the keywords of Renderer.set_overlay, e.g.
    dict(outlines=True, clock_step=0.5); it implies events=True and runs the three passes — the colour frame, the event frame, the
    overlay — so the pixels returned carry the lines (rgb, the float colours before packing, does not).  readouts: the list
    Renderer.set_readouts takes, or True for the scene's own (`d` commands, Scene.readouts()); it implies events=True too and runs the
    readout pass last: the colour frame, the event frame, the overlay if asked for, the readouts.  stars: a catalogue for
    Renderer.set_stars, at rest in the scene's frame (the sky's frame is set from the scene's camera, as for environment); it implies
    events=True as well and runs the star-field pass right after the event frame, under the overlay's lines and the readouts.
    particles: a set for Renderer.set_particles (particles.lattice, particles.at_events, ...), particle_options the keywords of
    Renderer.set_particle_options; it implies events=True too — the pass depth-tests against the event frame — and runs behind the
    stars, under the overlay's lines and the readouts.  star_temperatures, particle_temperatures: kelvin per star and per particle
    (Renderer.set_star_temperatures, set_particle_temperatures): those sources are Doppler-shifted as blackbodies.  segments: rods for
    Renderer.set_segments (segments.box_edges, segments.rod_lattice, ...), segment_options the keywords of
    Renderer.set_segment_options; it implies events=True as the particles do, and the pass runs right behind them.  particle_lighting:
    the keywords of Renderer.set_particle_lighting, e.g. dict(lit=True, shadows=True): the particles are dust that scatters the
    scene's lights.  ballistics: a set for Renderer.set_ballistics (ballistics.jet, ballistics.shell, ...), ballistic_options the
    keywords of Renderer.set_ballistic_options, ballistic_temperatures kelvin per record; it implies events=True as the particles do,
    and the pass runs right behind the segments.  rockets: a set for Renderer.set_rockets (rockets.launch, rockets.fleet, rockets.trip,
    ...), rocket_options the keywords of Renderer.set_rocket_options, rocket_temperatures kelvin per record; it implies events=True too,
    and the pass runs right behind the ballistic one.  glare: the layers of Renderer.set_glare, e.g. glare.preset("soft"): every
    point-source pass asked for spreads its sources by that point-spread function."""
    r = Renderer(device)
    try:
        r.set_glare(glare)
        if adaptive_aa is not None:
            r.set_adaptive_aa(*adaptive_aa)
        if orientation is not None:
            r.set_orientation(*orientation)
        if v_fov is not None:
            r.set_field_of_view(v_fov)
        if isinstance(projection, np.ndarray) or (isinstance(projection, str) and projection in RAYMAP_KINDS):
            r.set_raymap(projection if isinstance(projection, np.ndarray) else raymap(projection, width, height, fov=fov, fit=fit))
            r.set_projection("raymap")
        elif projection is not None:
            r.set_projection(**({"mode": projection} if isinstance(projection, str) else dict(projection)))
        if environment is not None:
            r.set_environment(environment)
        if environment is not None or stars is not None:
            r.set_environment_frame(scene.camera_lorentz()[1])
        r.upload_scene(scene)
        if scene.windows() is not None:       # (the scene's `w` commands)
            r.set_object_windows(scene.windows())
        r.set_scene_params(scene, width, height)
        r.set_output(None)
        if debug_rgb:
            r.set_debug_rgb(True)
        r.render()
        if overlay is not None or readouts is not None or stars is not None or particles is not None or segments is not None or ballistics is not None or rockets is not None:
            records = r.render_events()
            if stars is not None:
                r.set_stars(stars, star_temperatures)
                r.render_stars()
            if particles is not None:
                r.set_particles(particles, particle_temperatures)
                r.set_particle_options(**dict(particle_options or {}))
                r.set_particle_lighting(**dict(particle_lighting or {}))
                r.render_particles()
            if segments is not None:
                r.set_segment_options(**dict(segment_options or {}))
                r.set_segments(segments)
                r.render_segments()
            if ballistics is not None:
                r.set_ballistics(ballistics, ballistic_temperatures)
                r.set_ballistic_options(**dict(ballistic_options or {}))
                r.render_ballistics()
            if rockets is not None:
                r.set_rockets(rockets, rocket_temperatures)
                r.set_rocket_options(**dict(rocket_options or {}))
                r.render_rockets()
            if overlay is not None:
                r.set_overlay(**overlay)
                r.render_overlay()
            if readouts is not None:
                r.set_readouts(scene.readouts() if readouts is True else readouts)
                r.render_readouts()
            return r.read_framebuffer(), (r.read_debug_rgb() if debug_rgb else None), records
        frame = r.read_framebuffer(), (r.read_debug_rgb() if debug_rgb else None)
        return frame + (r.render_events(),) if events else frame
    finally:
        r.close()
