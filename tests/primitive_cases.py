"""The committed case list of the primitive ground truth (tests/primitive_truth.py) — TEST INFRASTRUCTURE shared by
tests/test_primitive_ground_truth.py (no GPU) and tests/test_gpu_primitive_ground_truth.py.

A case is (name, group, builder of the Scene, W, H, windows rule, lens).  Frames are 128 x 72, or 64 x 36 where a mesh is brute-forced.
Every case meets every cap of the test; a case that could not was replaced by another view or seed, none is exempt.
Groups and what each must show (NON_VACUITY; asserted over the group's cases by the test):
  shipped     all eight files of assets/reference/Scenes at events_oracle.SCENE_TIMES, interval -1 and 0, camera at rest, and the
              moving cameras below on those that keep >= 300 model hit pixels under them
  five        the issue's five-object scene (floor, flashing moving sphere, turned moving cube, a lamp at 0.8c, a lamp at rest) under
              every camera, and once from INSIDE the floor slab (the far walls; the bottom wall shadowed by the slab itself)
  windowed    the five-object scene with windows that act on a hit object, on an occluder and on a lamp, chosen as
              window_oracle.choose_windows does, both alternations
  generated   fixed seeds of scene_fuzz's random, extreme, close, walls and ellipsoids generators
  textured    synthetic textures (1 x 1, 2 x 2, 3 x 5, 5 x 3 and 16 x 16, all seeded noise) written as PNG files into a scratch asset root:
              spheres seen at the seam and at both poles; the camera inside a textured room with a turned moving cube, a 1 x 1 sphere and
              a 2 x 2 cube; the five-object scene textured (floor lit by the moving lamp and shadowed by the moving cube, the flashing sphere),
              once at gamma = 5; the pear (1602 vt) textured, moving, lit, in a cube's shadow and its own, and untextured; Scenes/bunny.txt's
              arrangement (a textured vt-less mesh and a lamp) at rest and receding
Moving cameras pass the origin at t = 0 (events_oracle.load_scene's rule) unless a case says otherwise; MIN_HIT_PIXELS holds for every case.
"""
import numpy as np

import events_oracle as eo
import scene_fuzz

FIVE = ("Oc\n p0,-3,8,0,0,1,0,12,1,12\n c0.6,0.6,0.6\n"
        "Os\n p-1.5,-0.8,7,0,0,1,0,1.2,1.2,1.2\n v0.6,0,0\n c0.8,0.3,0.2\n f1.5,0.6\n"
        "Oc\n p2,-1,9,0.6,0.2,1,0.1,1,1.5,0.7\n v-0.5,0,0.3\n c0.2,0.5,0.9\n"
        "Os\n p-2,4,6,0,0,1,0,0.3,0.3,0.3\n v0.8,0,0\n c1.0,0.9,0.7\n l1\n"
        "Os\n p3,3,10,0,0,1,0,0.4,0.4,0.4\n c0.5,0.7,1.0\n l1\nA0.3\nR\n")
FIVE_FLOOR, FIVE_SPHERE, FIVE_CUBE, FIVE_MOVING_LAMP, FIVE_LAMP = range(5)
MIN_HIT_PIXELS = 300
GAMMA5 = 0.98                                # gamma = 5.03
# name -> (velocity, time or None for the scene's own, position)
CAMERAS = {
    "rest": ((0.0, 0.0, 0.0), None, (0.0, 0.0, 0.0)),
    "oblique": ((0.3, 0.0, 0.5), 0.0, (0.0, 0.0, 0.0)),
    "receding": ((0.0, 0.0, -0.6), 0.0, (0.0, 0.0, 0.0)),
    "gamma5": ((0.0, 0.0, GAMMA5), 0.0, (0.0, 0.0, 0.0)),         # head-on: the view ahead shrinks tenfold, the floor fills it
    "gamma5x": ((GAMMA5, 0.0, 0.0), 0.0, (0.0, 0.0, 0.0)),        # sideways: what lies ahead is seen swung towards +x
}
LENS_HALF = 2.0 * float(np.arctan(0.5))                          # v_fov of half the default plane: four times the pixels per object
GENERATORS = {"random": lambda rng: scene_fuzz.random_scene_text(rng)[0], "extreme": scene_fuzz.extreme_scene_text,
              "close": scene_fuzz.close_scene_text, "walls": scene_fuzz.walls_scene_text, "ellipsoids": scene_fuzz.ellipsoids_scene_text}
# seeds chosen on the CPU oracle alone: >= MIN_HIT_PIXELS model hit pixels and the caps of the test met; the extreme ones (but 8, meshes
# at 0.99c) so that a sphere or cube at 0.999c or 0.9999c is hit
SEEDS = {"random": (1, 3, 5), "extreme": (8, 28, 143, 156, 185, 207, 772), "close": (0, 8, 12), "walls": (1, 13), "ellipsoids": (0, 4, 10)}
# (ellipsoids seed 4 stands where seed 2 stood: seed 2's textured needles, scale ratio 236 and 180 seen from 220 object units, have a
# derived (u, v) bound of 0.007 ... 0.02, 6 to 16 texels of their 800 x 400 texture, so 95 % of its pixels have no finite texture term
# under any camera of CAMERAS or lens; seed 4 is the generator's most unequal textured scene, ratio 119, that meets the caps)
# (scene, camera, v_fov or None)
SHIPPED_MOVING = (("arch", "oblique", None), ("arch", "receding", None), ("shadows", "oblique", None),
                  ("cubes", "receding", None), ("cubes", "oblique", None), ("soccer", "gamma5x", None), ("cube", "receding", None),
                  ("cube", "oblique", LENS_HALF), ("bunny", "receding", None), ("ladder_paradox", "receding", None))
# at rest the bunny covers 99 of 64 x 36 pixels: seen through the half lens.  arch.txt's untextured pillars are a few pixels wide and
# stand flush on the floor (exact ties in distance between two objects, which no float program can be held to): through the default
# pinhole 77 % of their pixels are well-conditioned for colours, through the half lens 82 %, through a 1.2 rad lens, which keeps the flush
# feet small and the lintel large, 89 % — the view used
ARCH_LENS = 1.2
SHIPPED_LENS = {"bunny": LENS_HALF, "arch": ARCH_LENS}
FAST = 0.9985                                # a "fast" primitive: a sphere or cube at this speed or more (the generators' 0.999c and 0.9999c)

# What each group must show on WELL-CONDITIONED pixels.  Every group is asked for everything its scenes can show: no shipped scene has a
# window or a camera inside a shape, and its one flashing scene, rulers.txt, is textured — its flash is asked for in colour as well as in
# the records' clock since textured hits carry a colour; the generated scenes have no windows, and must show the generators' own regime
# too: a sphere or cube at >= 0.999c hit and coloured.  (Lit by a lamp AND
# below the tonemap's clamp it is not: of extreme seeds 0-3999 every lit fast primitive is a lamp itself or clamps at 1 — `fast_primitive_lit`
# is computed by the test and printed, not asked.)  The textured group is asked for every way a texture or a mesh enters a colour:
# `clamped_tap` is x0 = W - 1 or y0 = H - 1, `second_texture_in_pool` a hit object whose texture starts at a byte offset > 0,
# `vt_less_mesh_textured` a textured mesh whose corners all read the one padded uv entry, `mesh_shadowed` a mesh hit in the shadow of
# ANOTHER object, `all_cube_faces_textured` the six faces (axis and side) of textured cubes over the group's cases.
NON_VACUITY = {
    "shipped": ("lit", "shadowed", "lit_by_moving_lamp", "flashing_clock", "not_flashing_clock", "flashing", "not_flashing", "textured_flashing",
                "textured_not_flashing", "textured_lit", "textured_shadowed", "mesh_lit", "mesh_self_shadowed", "vt_less_mesh_textured",
                "clamped_tap"),                                                                          # (shadows.txt's occluders are at rest)
    "five": ("lit", "shadowed", "lit_by_moving_lamp", "shadowed_by_moving_occluder", "self_shadowed", "flashing", "not_flashing", "inside"),
    "windowed": ("lit", "shadowed", "lit_by_moving_lamp", "shadowed_by_moving_occluder", "windowed_out", "flashing", "not_flashing"),
    "generated": ("lit", "shadowed", "shadowed_by_moving_occluder", "flashing_clock", "not_flashing_clock", "inside", "fast_primitive_hit",
                  "fast_primitive_coloured"),
    "textured": ("lit", "shadowed", "lit_by_moving_lamp", "shadowed_by_moving_occluder", "inside", "textured_lit", "textured_shadowed",
                 "textured_flashing", "textured_not_flashing", "mesh_lit", "mesh_shadowed", "mesh_self_shadowed", "all_cube_faces_textured",
                 "clamped_tap", "second_texture_in_pool", "vt_less_mesh_textured", "sphere_seam_both_sides", "sphere_both_poles"),
}


# ---- the textured group: synthetic textures in a scratch asset root ------------------------------------------------------------------------
# (width, height) of the synthetic textures, every byte seeded noise so that every tap and every channel matters
TEXTURES = {"noise16": (16, 16), "t3x5": (3, 5), "t5x3": (5, 3), "t1x1": (1, 1), "t2x2": (2, 2)}
_HEAD = "".join(f"TTextures/{n}.png\n" for n in ("noise16", "t3x5", "t5x3", "t1x1", "t2x2"))      # pool order: t0 .. t4
_LAMP = "Os\n p{},0,0,1,0,0.3,0.3,0.3\n c1.0,0.95,0.9\n l1\n"
# the seam (u = 0 | 1) is the object's -x meridian, the poles its +-y axis: one sphere turned so that the seam faces the camera, one
# showing its south and one its north pole; the second moves
TEX_SPHERES = (_HEAD + "Os\n p-2.7,0,7,-1.5708,0,1,0,1.2,1.2,1.2\n t0\n"
               "Os\n p0,-0.3,7.5,1.5708,1,0,0,1.2,1.2,1.2\n v0.5,0,0\n t1\n"
               "Os\n p2.7,0.2,7,-1.5708,1,0,0,1.2,1.2,1.2\n t2\n" + _LAMP.format("0,4,3") + "A0.3\nR\n")
# the camera inside a textured room (its five far walls), a turned moving cube (its near faces, -z among them), a 1 x 1 sphere and a
# 2 x 2 cube: every +1 tap of those two clamps
TEX_ROOM = (_HEAD + "Oc\n p0,0,4,0,0,1,0,9,6,9\n t2\n"
            "Oc\n p1.8,-1,7,0.6,0.2,1,0.1,1,1.5,0.7\n v-0.5,0,0.3\n t0\n"
            "Os\n p-2.2,0.8,6.5,0.4,1,1,0,1,1,1\n t3\n"
            "Oc\n p-1.5,-2.5,8,0.5,0,1,0,1,0.6,1\n t4\n" + _LAMP.format("0.5,3,3") + "A0.3\nR\n")
# the five-object scene, its floor textured by the 3 x 5 (byte offset 768 in the pool), the flashing sphere by the noise, the cube by the 5 x 3
TEX_FIVE = _HEAD + (FIVE.replace(" c0.6,0.6,0.6\n", " c0.6,0.6,0.6\n t1\n").replace(" c0.8,0.3,0.2\n", " c0.8,0.3,0.2\n t0\n")
                    .replace(" c0.2,0.5,0.9\n", " c0.2,0.5,0.9\n t2\n"))
# the pear (1602 vt) textured, moving, lit, on a textured floor; a small cube between the lamp and the pear
_PEAR = ("Oc\n p0,-3,8,0,0,1,0,12,1,12\n c0.6,0.6,0.6\n t1\n"
         "Om0\n p0.3,-1.6,6.5,0.5,0,1,0,1.1,1.1,1.1\n v0.3,0,0\n c0.85,0.86,0.40\n{}"
         "Oc\n p-1.25,1.15,5.75,0.3,1,1,0,0.3,0.3,0.3\n c0.2,0.5,0.9\n" + _LAMP.format("-3,4,5") + "A0.3\nR\n")
TEX_PEAR = "MModels/pear.obj\n" + _HEAD + _PEAR.format(" t0\n")
PLAIN_PEAR = "MModels/pear.obj\n" + _HEAD + _PEAR.format("")
# Scenes/bunny.txt's arrangement: a vt-less mesh, textured (every corner reads the one padded uv entry), and a lamp; here the texture is
# the 5 x 3, third in the pool
TEX_BUNNY = "MModels/bunny.obj\n" + _HEAD + "Om0\n p-0.5,-3,5,3.14,0,1,0,20,20,20\n t2\nOs\n l1\n p0,2,4,0,0,0,0,0.1,0.1,0.1\n c1,1,1\nA0.2\nR\n"
# the scene of the device's camera forms (tests/test_gpu_primitive_ground_truth.py): the five-object scene with the floor textured by
# the 3 x 5 and the cube by the noise, and the pear added, textured by the 5 x 3; 64 x 36
TEX_FORMS = ("MModels/pear.obj\n" + _HEAD + FIVE.replace(" c0.6,0.6,0.6\n", " c0.6,0.6,0.6\n t1\n").replace(" c0.2,0.5,0.9\n", " c0.2,0.5,0.9\n t0\n")
             .replace("A0.3\nR\n", "Om0\n p0.2,-1.2,5,0.5,0,1,0,0.8,0.8,0.8\n v0.2,0,0\n c0.85,0.86,0.40\n t2\nA0.3\nR\n"))
# (name, text, camera, W, H, lens)
TEXTURED = (("tex-spheres-rest", TEX_SPHERES, "rest", 128, 72, None), ("tex-room-rest", TEX_ROOM, "rest", 128, 72, None),
            ("tex-room-oblique", TEX_ROOM, "oblique", 128, 72, None),
            ("tex-five-rest", TEX_FIVE, "rest", 128, 72, None), ("tex-five-oblique", TEX_FIVE, "oblique", 128, 72, None),
            ("tex-five-gamma5", TEX_FIVE, "gamma5", 128, 72, None),
            ("tex-pear-rest", TEX_PEAR, "rest", 64, 36, LENS_HALF), ("tex-pear-receding", TEX_PEAR, "receding", 64, 36, None),
            ("plain-pear-receding", PLAIN_PEAR, "receding", 64, 36, None),
            ("tex-bunny-rest", TEX_BUNNY, "rest", 64, 36, LENS_HALF), ("tex-bunny-receding", TEX_BUNNY, "receding", 64, 36, None))
_ROOT = []


def texture_bytes(name):
    """The synthetic texture `name` as (H, W, 3) uint8: seeded noise."""
    import zlib
    w, h = TEXTURES[name]
    return np.random.default_rng(zlib.crc32(name.encode())).integers(0, 256, size=(h, w, 3), dtype=np.uint8)


def asset_root():
    """A scratch asset root, made once per process and removed at its end: the synthetic textures as PNG files (decoded by the front
    end's own Pillow path) and the two committed models the group uses."""
    if not _ROOT:
        import atexit
        import os
        import shutil
        import tempfile
        from PIL import Image
        from relativitypathtracer_amd.scene import ASSET_ROOT
        root = tempfile.mkdtemp(prefix="rpt_textured_")
        atexit.register(shutil.rmtree, root, ignore_errors=True)
        os.makedirs(os.path.join(root, "Textures"))
        os.makedirs(os.path.join(root, "Models"))
        for name in TEXTURES:
            Image.fromarray(texture_bytes(name), "RGB").save(os.path.join(root, "Textures", name + ".png"))
        for model in ("pear.obj", "bunny.obj"):
            shutil.copy(os.path.join(ASSET_ROOT, "Models", model), os.path.join(root, "Models", model))
        _ROOT.append(root)
    return _ROOT[0]


FORMS_POSITION = (0.0, -0.8, 2.0)             # nearer the floor and the objects than the origin: at 64 x 36 every camera form keeps the caps


def textured_forms_scene(camera):
    return _text(TEX_FORMS, camera, -1, t=2.0, position=FORMS_POSITION, root=asset_root())


def _camera(scene, camera, own_time=0.0):
    v, t, pos = CAMERAS[camera]
    scene.set_camera(v, own_time if t is None else t, pos)
    scene.update_objects()
    return scene


def _shipped(name, camera, interval):
    from relativitypathtracer_amd import Scene
    s = Scene.from_file(name)
    s.set_interval(interval)
    return _camera(s, camera, eo.SCENE_TIMES[name])


def _text(text, camera, interval, t=0.0, position=None, root=None):
    from relativitypathtracer_amd import Scene
    s = Scene() if root is None else Scene(asset_root=root, aliases={})
    s.inputScene(text)
    if interval is not None:
        s.set_interval(interval)
    if position is not None:
        s.set_camera(CAMERAS[camera][0], t, position)
        s.update_objects()
        return s
    return _camera(s, camera, t)


def _size(name):
    return (64, 36) if name in ("bunny", "shadows") else (128, 72)


def cases():
    """[(name, group, build, W, H, windows, v_fov)]: build() -> Scene with its objects up to date; windows None, or "choose" /
    "choose_flip" (window_oracle.choose_windows on the case's own frame, the alternation as given); v_fov None for the default
    pinhole, else the lens (events_oracle.lens_scale)."""
    out = []
    for name in eo.SHIPPED:
        for interval in (-1, 0):
            out.append((f"{name}-rest-i{interval}", "shipped", (lambda n=name, i=interval: _shipped(n, "rest", i)), *_size(name), None, SHIPPED_LENS.get(name)))
    for name, camera, lens in SHIPPED_MOVING:
        out.append((f"{name}-{camera}-i-1", "shipped", (lambda n=name, c=camera: _shipped(n, c, -1)), *_size(name), None, lens))
    for camera in ("rest", "oblique", "receding", "gamma5"):
        for interval in (-1, 0):
            out.append((f"five-{camera}-i{interval}", "five", (lambda c=camera, i=interval: _text(FIVE, c, i, t=2.0)), 128, 72, None, None))
    out.append(("five-inside-floor-i-1", "five", (lambda: _text(FIVE, "rest", -1, t=2.0, position=(0.0, -3.0, 8.0))), 128, 72, None, None))
    for rule in ("choose", "choose_flip"):
        out.append((f"five-windowed-{rule}", "windowed", (lambda: _text(FIVE, "rest", -1, t=2.0)), 128, 72, rule, None))
    out.append(("five-windowed-oblique", "windowed", (lambda: _text(FIVE, "oblique", -1)), 128, 72, "choose", None))
    for kind, seeds in SEEDS.items():
        for seed in seeds:
            text = generated_text(kind, seed)
            size = (64, 36) if "\nOm" in "\n" + text else (128, 72)
            out.append((f"{kind}-{seed}", "generated", (lambda tx=text: _text(tx, "rest", None)), *size, None, None))
    for name, text, camera, W, H, lens in TEXTURED:
        t = 2.0 if text is TEX_FIVE else 0.0
        out.append((name, "textured", (lambda tx=text, c=camera, t=t: _text(tx, c, -1, t=t, root=asset_root())), W, H, None, lens))
    return out


def generated_text(kind, seed):
    return GENERATORS[kind](np.random.default_rng(20261019 + seed))


def generated(kind, seed):
    return _text(generated_text(kind, seed), "rest", None)


def case_ids():
    return [c[0] for c in cases()]
