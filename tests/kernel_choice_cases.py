"""The host's kernel choice, driven through every combination of settings that bears on it: which kernel a frame, an event pass or
rpt_verify_frame gets, or which refusal.  tools/record_kernel_choice.py records the outcomes of one commit into
tests/golden/kernel_choice.json; tests/test_gpu_kernel_choice.py replays the same products on the code under test and asks for equality.

An outcome is [return code, rpt_last_error's text ("" unless refused), rpt_last_variant, rpt_last_exact_rcp, rpt_last_aa_variant]; for an
event pass the last three are rpt_last_events_variant and rpt_last_events_exact_rcp.  The numbers are read after a refusal as well: what a
refused launch leaves in them is part of the record, and the products are always walked in the same order."""
from __future__ import annotations

import base64
import ctypes as C
import os
import tempfile
import zlib

import numpy as np

VARIANTS = (0, 1, 3, 41, 43, 44, 48, 49, 50, 51)
SCENES = ("analytic", "mesh", "mesh_children_apart", "mesh_outside_rcp_exact")
FRAMES = ((16, 8), (72, 8))                # 72 x 8 is wider than 4 : 1: outside the window the screen regions are proven for
DOPPLER = ("off", "flags3", "flags3_record")
PROJECTIONS = ("pinhole", "equirect")
LENSES = (0.0, 1.0, 2.0)                   # v_fov: off, tan(v_fov / 2) < 1, tan(v_fov / 2) > 1
SMALL_FRAME = (2048, 1472)                 # 3 014 656 pixels: just above RPT_LATENCY_KERNEL_MAX_PIXELS = 3 000 000
SKY = np.arange(4 * 2 * 3, dtype=np.uint8).reshape(2, 4, 3) * 10

ANALYTIC_TEXT = "Os\n p-1,0,6,0,0,0,0,1,1,1\n l1\n c10,10,10\nOc\n p1,0,6,0,0,0,0,1,1,1\n c1,1,1\nA0.2\nR\n"
MESH_TEXT = "MModels/triangle.obj\nOs\n p-2,2,6,0,0,0,0,0.5,0.5,0.5\n l1\n c10,10,10\nOm0\n p0,0,6,0,0,0,0,1,1,1\n c1,1,1\nA0.2\nR\n"
HUGE_OBJ = ("v -2147483648 -2147483648 8589934592\nv 2147483648 -2147483648 8589934592\nv 0 2147483648 8589934592\n"
            "vt 0 0\nvn 0 0 1\nf 1/1/1 2/1/1 3/1/1\n")          # |e1| |e2| > 2^60 (test_gpu_exact_division.py)


def _scene(text, extra_obj=None):
    from relativitypathtracer_amd import Scene
    s = Scene()
    s.inputScene(text)
    if extra_obj:
        s.ReadOBJ(extra_obj)               # in the mesh pool, named by no object: its triangles alone put the scene outside the domain
    s.set_camera((0.0, 0.0, 0.0), 0.0)
    s.update_objects()
    return s


class Driver:
    """One context and the four scenes; every setter goes to the library directly and must succeed (refusals come at the launch)."""

    def __init__(self, renderer):
        self.r = renderer
        self.lib, self.h = renderer._lib, renderer._h
        self.tmp = tempfile.TemporaryDirectory()
        huge = os.path.join(self.tmp.name, "huge.obj")
        with open(huge, "w") as f:
            f.write(HUGE_OBJ)
        self.scenes = {"analytic": _scene(ANALYTIC_TEXT), "mesh": _scene(MESH_TEXT), "mesh_children_apart": _scene(MESH_TEXT),
                       "mesh_outside_rcp_exact": _scene(MESH_TEXT, huge)}
        self.scene = None

    def close(self):
        self.tmp.cleanup()

    def ok(self, rc):
        assert rc == 0, (rc, self.lib.rpt_last_error(self.h).decode())

    def set_scene(self, name):
        self.scene = s = self.scenes[name]
        if name != "mesh_children_apart":
            self.r.upload_scene(s)
            return
        # an octree whose children are not consecutive (test_gpu_environment.py::test_variants_and_refusals): no derived layout
        from relativitypathtracer_amd import _ffi
        oc = s.buffers()["octrees"].copy().view(np.int32).reshape(-1, 24)
        root = s.mesh_roots()[0]
        assert oc[root, 10] != -1, "the mesh's root is a leaf: there are no children to move apart"
        new = np.vstack([oc, oc[oc[root, 10]][None]])
        new[root, 10] = len(oc)
        d2 = _ffi.SceneDesc.from_buffer_copy(s.desc())
        raw = np.ascontiguousarray(new).view(np.uint8).reshape(-1)
        d2.octrees, d2.octree_count = raw.ctypes.data, len(new)
        self.r.upload_desc(d2)

    def set_frame(self, size):
        self.r.set_scene_params(self.scene, *size)
        self.r.set_output(None)

    def set_sky(self, on):
        self.r.set_environment(SKY if on else None)

    def set_variant(self, v):
        self.ok(self.lib.rpt_set_variant(self.h, v))

    def set_msaa(self, n):
        self.ok(self.lib.rpt_set_msaa(self.h, n))

    def set_doppler(self, mode):
        self.ok(self.lib.rpt_set_doppler(self.h, 0 if mode == "off" else 3))
        self.ok(self.lib.rpt_set_debug_doppler(self.h, C.c_void_p(1 if mode == "flags3_record" else 0)))

    def set_projection(self, mode):
        self.r.set_projection(mode)

    def set_lens(self, v_fov):
        self.ok(self.lib.rpt_set_field_of_view(self.h, v_fov))

    def set_aa(self, n):
        self.ok(self.lib.rpt_set_adaptive_aa(self.h, n, 8))

    # -- the calls -----------------------------------------------------------------------------------------------------------------
    def _colour_outcome(self, rc):
        lib, h = self.lib, self.h
        return (rc, lib.rpt_last_error(h).decode() if rc else "", lib.rpt_last_variant(h), lib.rpt_last_exact_rcp(h), lib.rpt_last_aa_variant(h))

    def render(self):
        return self._colour_outcome(self.lib.rpt_render(self.h))

    def render_async(self):
        rc = self.lib.rpt_render_async(self.h)
        return self._colour_outcome(rc if rc else self.lib.rpt_sync(self.h))

    def verify_frame(self):
        n = C.c_uint64(0)
        return self._colour_outcome(self.lib.rpt_verify_frame(self.h, C.byref(n)))

    def render_events(self):
        lib, h = self.lib, self.h
        rc = lib.rpt_render_events(h)
        exact = C.c_int(0)
        self.ok(lib.rpt_last_events_exact_rcp(h, C.byref(exact)))
        return (rc, lib.rpt_last_error(h).decode() if rc else "", lib.rpt_last_events_variant(h), exact.value)


# Every product: its axes in the order they are walked (the first is the outermost loop), each a (name, values, setter) triple, and the call.
def products():
    scene = ("scene", SCENES, "set_scene")
    variant = ("variant", VARIANTS, "set_variant")
    doppler = ("doppler", DOPPLER, "set_doppler")
    projection = ("projection", PROJECTIONS, "set_projection")
    lens = ("lens", LENSES, "set_lens")
    sky = ("sky", (False, True), "set_sky")
    aa = ("adaptive_aa", (1, 2), "set_aa")
    frame = ("frame", FRAMES, "set_frame")
    one_mesh = ("scene", ("mesh",), "set_scene")
    return {
        "render": dict(axes=[scene, frame, sky, ("msaa", (1, 2), "set_msaa"), variant, doppler, projection, lens, aa, ("call", ("render", "render_async"), None)],
                       call=None),
        "render_events": dict(axes=[scene, frame, variant, projection, lens], call="render_events"),
        "verify_frame": dict(axes=[scene, ("frame", FRAMES[:1], "set_frame"), variant, doppler, projection, lens], call="verify_frame"),
        # rpt_set_rows(1, 2, 1): every second row of tiles, into a colour plane (16 x 32: four rows of tiles, two of them this context's)
        "rows": dict(axes=[one_mesh, ("frame", ((16, 32),), "set_frame"), ("variant", (0,), "set_variant"), doppler, projection, lens, aa,
                           ("call", ("render", "render_async"), None)], call=None, rows=(1, 2, 1)),
        # the small-frame rule: in flight, a frame just above the limit gets the throughput walk (41 and its forms), not 43
        "small_frame": dict(axes=[one_mesh, ("frame", (SMALL_FRAME,), "set_frame"), ("variant", (0,), "set_variant"), doppler,
                                  projection, lens, sky, aa], call="render_async"),
    }


def reset(d):
    d.ok(d.lib.rpt_set_rows(d.h, 0, 1, 0))
    d.set_sky(False)
    d.set_msaa(1)
    d.set_variant(0)
    d.set_doppler("off")
    d.set_projection("pinhole")
    d.set_lens(0.0)
    d.set_aa(1)


def walk(d, product):
    """The outcomes of one product, in the order of itertools.product over its axes (the first axis is the outermost loop)."""
    axes, call = product["axes"], product["call"]
    out = []

    def level(k):
        if k == len(axes):
            out.append(getattr(d, call)())
            return
        _, values, setter = axes[k]
        for v in values:
            if setter is None:               # the call axis, the innermost: the value names the call
                out.append(getattr(d, v)())
            else:
                getattr(d, setter)(v)
                level(k + 1)

    reset(d)
    if "rows" in product:
        d.ok(d.lib.rpt_set_rows(d.h, *product["rows"]))
    level(0)
    reset(d)
    return out


def run_all(renderer):
    """{product name: list of outcomes}, every product on one context."""
    d = Driver(renderer)
    try:
        return {name: walk(d, p) for name, p in products().items()}
    finally:
        d.close()


def axes_record(product):
    return [[name, [list(v) if isinstance(v, tuple) else v for v in values]] for name, values, _ in product["axes"]]


def pack_index(index):
    """One index per combination as the record stores it: little-endian uint16, zlib, base64."""
    return base64.b64encode(zlib.compress(np.asarray(index, dtype="<u2").tobytes(), 9)).decode()


def unpack_index(text):
    return np.frombuffer(zlib.decompress(base64.b64decode(text)), dtype="<u2").tolist()
