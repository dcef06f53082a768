"""examples/rpt_render_main.cpp with the free-look options: --yaw --pitch --roll --fov (degrees) reach rpt_set_orientation and
rpt_set_field_of_view before the objects are handed over, and the frame is the one Renderer renders for the same view."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_example_host import ASSETS, build

ARGS = ["--yaw", "180", "--fov", "40", "--pitch", "-10", "--roll", "25"]


def test_an_option_without_its_value_is_an_error(tmp_path):
    exe = build(tmp_path)
    p = subprocess.run([exe, "64", "48", str(tmp_path / "o.ppm"), "--fov"], stdin=subprocess.DEVNULL, capture_output=True, text=True)
    assert p.returncode == 2 and "--fov needs a value" in p.stderr


@pytest.mark.gpu
def test_example_host_with_a_view_matches_the_renderer(tmp_path):
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer
    exe = build(tmp_path)
    out = tmp_path / "shadows.ppm"
    W, H = 320, 184
    with open(os.path.join(ASSETS, "Scenes", "shadows.txt")) as f:
        p = subprocess.run([exe, *ARGS[:4], str(W), str(H), str(out), "0", "0", "0.5", "16", *ARGS[4:]], stdin=f, capture_output=True, text=True,
                           env={**os.environ, "RPT_ASSETS": ASSETS})
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    img = np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)
    s = Scene.from_file("shadows")
    s.set_camera((0, 0, 0.5), 16.0)
    s.update_objects()
    deg = math.pi / 180.0
    r = Renderer(0)
    try:
        r.set_orientation(180 * deg, -10 * deg, 25 * deg)
        r.set_field_of_view(40 * deg)
        r.upload_scene(s)
        r.set_scene_params(s, W, H)
        r.set_output(None)
        r.render()
        assert r.last_variant() == 843
        want = r.read_framebuffer()["rgba"].reshape(H, W, 4)[::-1, :, :3]
    finally:
        r.close()
    assert np.array_equal(img, want)
    # and it is not the un-turned frame
    r = Renderer(0)
    try:
        r.upload_scene(s)
        r.set_scene_params(s, W, H)
        r.set_output(None)
        r.render()
        assert not np.array_equal(img, r.read_framebuffer()["rgba"].reshape(H, W, 4)[::-1, :, :3])
    finally:
        r.close()
