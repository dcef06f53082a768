"""examples/rpt_render_main.cpp with --aa N[:T]: the option reaches rpt_set_adaptive_aa (on the frame ring's slots too), and the frame is
the one Renderer renders with the same setting."""
import os
import re
import subprocess

import numpy as np
import pytest

from test_example_host import ASSETS, build


def test_a_malformed_option_is_an_error(tmp_path):
    exe = build(tmp_path)
    for args, message in ((["--aa"], "--aa needs a value"), (["--aa", "two", "64", "48", "o.ppm"], "--aa takes N or N:T"),
                          (["--aa", "2:x", "64", "48", "o.ppm"], "--aa takes N or N:T")):
        p = subprocess.run([exe, *args], stdin=subprocess.DEVNULL, capture_output=True, text=True, cwd=str(tmp_path))
        assert p.returncode == 2 and message in p.stderr, (args, p.stderr)


@pytest.mark.gpu
@pytest.mark.parametrize("aa, setting, frames", [("3:4", (3, 4), ()), ("2", (2, 8), ()), ("2:-1", (2, -1), ())])
def test_example_host_with_adaptive_aa_matches_the_renderer(tmp_path, aa, setting, frames):
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.adaptive import refine_mask
    from relativitypathtracer_amd.renderer import Renderer
    exe = build(tmp_path)
    out = tmp_path / "shadows.ppm"
    W, H = 320, 184
    with open(os.path.join(ASSETS, "Scenes", "shadows.txt")) as f:
        p = subprocess.run([exe, "--aa", aa, "--fov", "50", str(W), str(H), str(out), "0", "0", "0.5", "16", *frames], stdin=f, capture_output=True, text=True,
                           env={**os.environ, "RPT_ASSETS": ASSETS})
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    img = np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)
    s = Scene.from_file("shadows")
    s.set_camera((0, 0, 0.5), 16.0)
    s.update_objects()
    r = Renderer(0)
    try:
        r.set_field_of_view(np.float32(50 * 3.14159265358979323846 / 180.0))
        r.upload_scene(s)
        r.set_scene_params(s, W, H)
        r.set_output(None)
        r.render()
        coarse = r.read_framebuffer()["rgba"].reshape(H, W, 4)[:, :, :3].copy()
        r.set_adaptive_aa(*setting)
        r.render()
        want = r.read_framebuffer()["rgba"].reshape(H, W, 4)[::-1, :, :3]
        refined, kernel = r.last_aa_refined(), r.last_aa_variant()
    finally:
        r.close()
    assert np.array_equal(img, want)
    assert refined == int(refine_mask(coarse, setting[1]).sum()) and 0 < refined
    m = re.search(r"threshold (-?\d+): (\d+) of (\d+) pixels refined \(kernel (\d+)\)", p.stderr)
    assert m and (int(m.group(1)), int(m.group(2)), int(m.group(3)), int(m.group(4))) == (setting[1], refined, W * H, kernel), p.stderr
    assert not np.array_equal(img, coarse[::-1])
