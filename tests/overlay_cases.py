"""The scenes, cameras, sizes and layer settings of the overlay tests — TEST INFRASTRUCTURE shared by tests/test_overlay_model.py (no GPU:
it asserts on the CPU event frames that every line layer chosen here marks more than 1 % and fewer than 50 % of a scene's hit pixels)
and tests/test_gpu_overlay.py (which runs exactly these on the device)."""
import numpy as np

import events_oracle as eo
from relativitypathtracer_amd.renderer import orient_objects

SCENES = ["rulers", "ladder_paradox", "shadows", "arch"]       # light delay on (interval -1) in all four; shadows holds the mesh
SIZES = [(128, 72), (67, 41)]            # 67 is no multiple of the kernel's 64-pixel tile width, 41 none of its 8-pixel height
YPR = (0.4, -0.25, 0.15)
PANO = dict(h_fov=2.0, v_fov=1.2, yaw=0.3)
LENS_V_FOV = 1.2
CAMERAS = ["pinhole", "panorama", "lens"]                      # "lens" is the lens turned by YPR

# contour steps per scene, in the scene's units: chosen so that each layer draws a readable number of lines at 128 x 72
STEPS = {
    "rulers":         dict(delay_step=0.5, clock_step=0.5, lattice_step=(1.0, 1.0, 1.0)),
    "ladder_paradox": dict(delay_step=0.5, clock_step=0.5, lattice_step=(1.0, 1.0, 1.0)),
    "shadows":        dict(delay_step=2.0, clock_step=2.0, lattice_step=(2.0, 2.0, 2.0)),
    "arch":           dict(delay_step=2.0, clock_step=2.0, lattice_step=(4.0, 4.0, 4.0)),
}
COLOURS = dict(outline_rgba=(255, 255, 255, 200), delay_rgba=(255, 255, 0, 160), clock_rgba=(0, 255, 255, 255),
               lattice_rgba=(255, 0, 255, 96), tint_alpha=128)


def layer_settings(name):
    """{layer name: the keywords that switch that layer alone on} for scene `name`, and "all": the five together."""
    st = STEPS[name]
    alone = {
        "outlines": dict(outlines=True, outline_rgba=COLOURS["outline_rgba"]),
        "delay": dict(delay_step=st["delay_step"], delay_rgba=COLOURS["delay_rgba"]),
        "clock": dict(clock_step=st["clock_step"], clock_rgba=COLOURS["clock_rgba"]),
        "lattice": dict(lattice_step=st["lattice_step"], lattice_rgba=COLOURS["lattice_rgba"]),
        "tint": dict(tint=True, tint_alpha=COLOURS["tint_alpha"]),
    }
    both = {}
    for kw in alone.values():
        both.update(kw)
    return dict(alone, all=both)


def cpu_events(lib, scene, W, H, camera):
    """The (H, W) records of tests/native/event_oracle.c for one of CAMERAS."""
    if camera == "pinhole":
        return eo.oracle_events(lib, scene, W, H)
    if camera == "panorama":
        return eo.oracle_events(lib, scene, W, H, dirs=eo.pano_dirs(W, H, **PANO))
    assert camera == "lens"
    return eo.oracle_events(lib, scene, W, H, dirs=eo.pinhole_dirs(W, H, eo.lens_scale(LENS_V_FOV)), objects=orient_objects(scene, *YPR))


def marked(before, after):
    """(H, W) bool: the pixels whose RGBA differs."""
    return (np.asarray(before) != np.asarray(after)).any(axis=-1)
