"""The one case of the pass-tally tests — TEST INFRASTRUCTURE shared by tests/test_pass_tallies_model.py (no GPU: it asserts by the
CPU models that every pass has something to count here) and tests/test_gpu_pass_tallies.py (which runs exactly this on the device)."""
import events_oracle as eo
import readout_cases as rc
import stars_cases as sc
from relativitypathtracer_amd import stars

SIZE = rc.SIZES[1]                          # 67 x 41: no multiple of the tile kernels' 64 x 8 either way
AA = (2, 8)                                 # set_adaptive_aa: 2 x 2 samples, threshold 8
OVERLAY = dict(outlines=True, outline_rgba=(255, 255, 255, 200), clock_step=0.5, clock_rgba=(0, 255, 255, 160))
OTHER_OVERLAY = dict(tint=True, tint_alpha=128)       # what the second context draws
STARS = 4096
CAMERA = sc.CAMERAS["pinhole"]


def scene_and_readouts():
    """The `cube` case of readout_cases.scenes()."""
    return eo.scene_from_text(rc.CUBE_TEXT, t=2.0), rc.CUBE_READOUTS


def catalogue():
    return stars.random_catalogue(STARS, sc.SEED)
