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
SEEDS = {"random": (1, 3, 5), "extreme": (8, 28, 143, 156, 185, 207, 772), "close": (0, 8, 12), "walls": (1, 13), "ellipsoids": (0, 2, 10)}
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
# window or a camera inside a shape (its one flashing scene, rulers.txt, is textured: the flash is seen in the records' clock, its
# colour is not compared); the generated scenes have no windows and their flashing objects are textured or lamps at the clamp (the
# flash is seen in the records' clock), and must show the generators' own regime instead: a sphere or cube at >= 0.999c hit and coloured.  (Lit by a lamp AND
# below the tonemap's clamp it is not: of extreme seeds 0-3999 every lit fast primitive is a lamp itself or clamps at 1 — `fast_primitive_lit`
# is computed by the test and printed, not asked.)
NON_VACUITY = {
    "shipped": ("lit", "shadowed", "lit_by_moving_lamp", "flashing_clock", "not_flashing_clock"),        # (shadows.txt's occluders are at rest)
    "five": ("lit", "shadowed", "lit_by_moving_lamp", "shadowed_by_moving_occluder", "self_shadowed", "flashing", "not_flashing", "inside"),
    "windowed": ("lit", "shadowed", "lit_by_moving_lamp", "shadowed_by_moving_occluder", "windowed_out", "flashing", "not_flashing"),
    "generated": ("lit", "shadowed", "shadowed_by_moving_occluder", "flashing_clock", "not_flashing_clock", "inside", "fast_primitive_hit",
                  "fast_primitive_coloured"),
}


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


def _text(text, camera, interval, t=0.0, position=None):
    from relativitypathtracer_amd import Scene
    s = Scene()
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
    return out


def generated_text(kind, seed):
    return GENERATORS[kind](np.random.default_rng(20261019 + seed))


def generated(kind, seed):
    return _text(generated_text(kind, seed), "rest", None)


def case_ids():
    return [c[0] for c in cases()]
