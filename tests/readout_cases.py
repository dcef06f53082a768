"""The scenes, cameras, sizes and displays of the readout tests — TEST INFRASTRUCTURE shared by tests/test_readout_model.py (no GPU: it
asserts on CPU event frames that every case here has pixels of every kind the pass distinguishes) and tests/test_gpu_readout.py (which
runs exactly these on the device)."""
import numpy as np

import events_oracle as eo
from relativitypathtracer_amd import worldline
from relativitypathtracer_amd.renderer import orient_objects

SIZES = [(128, 72), (67, 41), (65, 9)]       # 67 x 41: no multiple of the kernel's 64 x 8 tile; 65 x 9: one pixel into the second tile both ways
YPR = (0.2, -0.1, 0.15)
PANO = dict(h_fov=3.0, v_fov=1.2, yaw=0.1)
LENS_V_FOV = 1.2
CAMERAS = ["pinhole", "panorama", "lens"]    # "lens" is the lens turned by YPR

# a cube of scale (2, 1, 0.5) at z = 3 that moves at 0.6 c along x and carries the display, a sphere beside it that has none
CUBE_TEXT = "Oc p0,0,3,0,0,1,0,2,1,0.5 c0.3,0.5,0.9 v0.6,0,0\nOs p-0.2,1.15,3.2,0,0,1,0,0.5,0.5,0.5 c0.9,0.6,0.2\nR\n"
CUBE_READOUTS = [dict(rate=1.0, offset=50.0, digits=3, decimals=1, rect=(0.05, 0.2, 0.95, 0.8), on_rgba=(255, 40, 0, 255), off_rgba=(0, 0, 0, 160)), None]

# for the 65 x 9 frame, whose pinhole sees +-82 degrees across and +-45 up: a wide cube close to the camera with one large digit, so that
# a segment still covers whole pixels, and a sphere beside it
STRIP_TEXT = "Oc p0,0,1.3,0,0,1,0,2.4,0.8,0.3 c0.3,0.5,0.9 v0.3,0,0\nOs p4.2,0,1.2,0,0,1,0,0.45,0.45,0.45 c0.9,0.6,0.2\nR\n"
STRIP_READOUTS = [dict(rate=0.1, offset=8.0, digits=1, decimals=0, rect=(0.15, 0.05, 0.85, 0.95), on_rgba=(255, 40, 0, 255), off_rgba=(0, 0, 0, 160)), None]

# a sphere turned so that its uv seam faces the camera, inside the display's rectangle (the whole circumference, mirrored in u); a cube without a display behind it
SPHERE_TEXT = "Os p0,0,3,4.73,0,1,0,1.2,1.2,1.2 c0.8,0.8,0.8\nOc p1.6,0.9,5,0,0,1,0,0.5,0.5,0.5 c0.2,0.7,0.3\nR\n"
SPHERE_READOUTS = [dict(rate=-2.0, offset=3.0, digits=9, decimals=3, rect=(1.0, 0.35, 0.0, 0.65), on_rgba=(0, 255, 80, 200), off_rgba=(20, 20, 20, 255)), None]

# `shadows`, the shipped scene with the mesh: a display on the mesh (object 4) and one on the wall behind it (object 3)
MESH_READOUTS = [None, None, None, dict(rate=1.0, offset=0.0, digits=4, decimals=2, rect=(0.3, 0.3, 0.7, 0.6)),
                 dict(rate=10.0, offset=0.0, digits=2, decimals=0, rect=(0.0, 0.0, 1.0, 1.0), on_rgba=(255, 255, 0, 255), off_rgba=(0, 0, 64, 128))]


def many_objects_text():
    """70 objects: 69 small spheres in a ring and, as object 66, a cube that carries the display — beyond the 64 objects whose
    "has a display" the kernel reads from its arguments."""
    lines = []
    for k in range(70):
        if k == 66:
            lines.append("Oc p0,0,3,0,0,1,0,2,1,0.5 c0.3,0.5,0.9 v0,0.3,0")
        else:
            a = 2.0 * np.pi * k / 70.0
            lines.append(f"Os p{2.6 * np.cos(a):.4f},{1.3 * np.sin(a):.4f},4,0,0,1,0,0.12,0.12,0.12 c0.9,0.9,0.2")
    return "\n".join(lines) + "\nR\n"


MANY_READOUTS = [None] * 66 + [dict(rate=1.0, offset=-7.25, digits=4, decimals=2, rect=(0.05, 0.2, 0.95, 0.8))] + [None] * 3


def turnaround():
    """(worldline, scene text, camera time): a cube that goes out along +x at 0.6 c, turns and comes back, every leg with a display of
    the body's proper time (worldline.to_dsl(readout=...)); and a sphere at rest without a display.  At the camera time the light of
    both legs has left: without the windows both legs are there at once."""
    wl = worldline.piecewise([(0.0, -3.0, 0.0, 4.0), (5.0, 0.0, 0.0, 4.0), (10.0, -3.0, 0.0, 4.0)])
    text = wl.to_dsl("Oc", scale=(1.6, 0.8, 0.4), extra="c0.3,0.5,0.9", readout="3,1,0.05,0.2,0.95,0.8", tau0=2.0)
    return wl, text + "Os p1.5,1.2,5,0,0,1,0,0.4,0.4,0.4 c0.9,0.6,0.2\nR\n", 7.5


def scenes():
    """{case name: (scene, readouts)}; built once per test module."""
    shadows = eo.load_scene("shadows", "rest", -1)
    wl, text, t = turnaround()
    turn = eo.scene_from_text(text, t=t)
    return {
        "cube": (eo.scene_from_text(CUBE_TEXT, t=2.0), CUBE_READOUTS),
        "strip": (eo.scene_from_text(STRIP_TEXT, t=0.5), STRIP_READOUTS),
        "sphere": (eo.scene_from_text(SPHERE_TEXT, t=1.0), SPHERE_READOUTS),
        "mesh": (shadows, MESH_READOUTS),
        "many": (eo.scene_from_text(many_objects_text(), t=1.0), MANY_READOUTS),
        "turnaround": (turn, turn.readouts()),
    }


# the GPU cases: (scene, camera, size).  The cube runs every camera at the two larger sizes and the strip every camera at 65 x 9 (there
# the cube's digits would be thinner than a pixel); the others the pinhole at the two larger sizes, and the 70 objects, whose
# "has a display" takes the table's path, the panorama and the turned lens at 67 x 41 too
CASES = [("cube", camera, size) for camera in CAMERAS for size in SIZES[:2]] + [("strip", camera, SIZES[2]) for camera in CAMERAS] + [(name, "pinhole", size) for name in ("sphere", "mesh", "many") for size in SIZES[:2]] + [("many", "panorama", SIZES[1]), ("many", "lens", SIZES[1])]


def cpu_events(lib, scene, W, H, camera):
    """The (H, W) records of tests/native/event_oracle.c for one of CAMERAS."""
    if camera == "pinhole":
        return eo.oracle_events(lib, scene, W, H)
    if camera == "panorama":
        return eo.oracle_events(lib, scene, W, H, dirs=eo.pano_dirs(W, H, **PANO))
    assert camera == "lens"
    return eo.oracle_events(lib, scene, W, H, dirs=eo.pinhole_dirs(W, H, eo.lens_scale(LENS_V_FOV)), objects=orient_objects(scene, *YPR))
