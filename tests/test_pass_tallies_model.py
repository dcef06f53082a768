"""The case of tests/test_gpu_pass_tallies.py without a device: by the project's CPU models every one of the five numbers that test reads
back — refined pixels, overlay pixels, readout pixels, stars inside the frame, pixels the stars changed — is above zero on the 67 x 41
cube frame of tests/pass_tallies_case.py, so a tally that reads another's storage, or nothing, cannot pass there by reading zero."""
import pytest

import aa_support
import events_oracle as eo
import oracle_ffi
import pass_tallies_case as case
import readout_cases as rc
import stars_cases as sc
from relativitypathtracer_amd.adaptive import refine_mask
from relativitypathtracer_amd.events import overlay, readout


@pytest.fixture(scope="module")
def events_lib(tmp_path_factory):
    return eo.build_library(tmp_path_factory.mktemp("tallies_events"))


@pytest.fixture(scope="module")
def stars_lib(tmp_path_factory):
    return sc.build_library(tmp_path_factory.mktemp("tallies_stars"))


def test_every_pass_has_something_to_count(events_lib, stars_lib):
    W, H = case.SIZE
    scene, readouts = case.scene_and_readouts()
    interval = scene.params["interval"]
    px, _, _ = oracle_ffi.render(scene, W, H, want_rgb=False)
    ev = rc.cpu_events(events_lib, scene, W, H, "pinhole")
    refined = int(refine_mask(aa_support.rgb8_of(px, W, H), case.AA[1]).sum())
    _, overlay_pixels = overlay(px["rgba"], ev, interval, **case.OVERLAY)
    _, other_overlay_pixels = overlay(px["rgba"], ev, interval, **case.OTHER_OVERLAY)
    _, readout_pixels = readout(px["rgba"], ev, readouts)
    view = sc.view(case.CAMERA, W, H, scene.camera_lorentz()[1], interval, 0, scene.params["white_point"])
    _, (stars_inside, star_pixels) = sc.oracle_pass(stars_lib, view, case.catalogue(), px, ev)
    print(f"{W}x{H}: refined {refined}, overlay {overlay_pixels} (the second context's {other_overlay_pixels}), readouts {readout_pixels}, stars {stars_inside} inside, {star_pixels} pixels")
    assert refined > 0 and overlay_pixels > 0 and readout_pixels > 0 and stars_inside > 0 and star_pixels > 0
    assert 0 < other_overlay_pixels != overlay_pixels      # the second context's pass would be noticed in the first's count
