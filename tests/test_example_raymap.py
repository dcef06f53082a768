"""examples/rpt_render_main.cpp --projection SPEC: the value is read and the map filled on the host before any device is asked for, so a
bad value ends the program with status 2 on every machine; on the GPU the fisheye PPM is the frame Renderer renders through the same map."""
import math
import os
import subprocess

import numpy as np
import pytest

from test_example_host import ASSETS, build


def _run(exe, tmp_path, *args):
    return subprocess.run([exe, *args, str(tmp_path / "o.ppm")], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)


def test_projection_values_are_checked_before_the_device_is_asked_for(tmp_path):
    exe = build(tmp_path)
    p = subprocess.run([exe, "64", "48", str(tmp_path / "o.ppm"), "--projection"], stdin=subprocess.DEVNULL, capture_output=True, text=True, timeout=120)
    assert p.returncode == 2 and "--projection needs a value" in p.stderr
    for spec, size, message in (("gnomonic", ("64", "48"), "unknown projection 'gnomonic'"),
                                ("fisheye:abc", ("64", "48"), "'abc' in 'fisheye:abc' is not a number"),
                                ("fisheye:", ("64", "48"), "is not a number"),
                                ("fisheye:180:0:7", ("64", "48"), "too many values"),
                                ("fisheye:400", ("64", "48"), "out of range"),
                                ("stereographic:360", ("64", "48"), "out of range"),
                                ("equisolid:180:2", ("64", "48"), "out of range"),
                                ("cube_strip:90", ("96", "16"), "too many values"),
                                ("cube_strip", ("64", "48"), "cube_strip needs width = 6 height, not 64 x 48")):
        p = _run(exe, tmp_path, "--projection", spec, *size)
        assert p.returncode == 2 and message in p.stderr, (spec, p.returncode, p.stderr)
        assert "no usable gfx950 device" not in p.stderr


@pytest.mark.gpu
def test_example_host_fisheye_matches_the_renderer(tmp_path):
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import Renderer, raymap
    exe = build(tmp_path)
    out = tmp_path / "shadows.ppm"
    W, H = 100, 52
    with open(os.path.join(ASSETS, "Scenes", "shadows.txt")) as f:
        p = subprocess.run([exe, "--projection", "fisheye:200:1", "--yaw", "30", str(W), str(H), str(out), "0", "0", "0.5", "16"], stdin=f,
                           capture_output=True, text=True, env={**os.environ, "RPT_ASSETS": ASSETS}, timeout=120)
    assert p.returncode == 0, p.stderr
    data = out.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    img = np.frombuffer(data[len(header):], np.uint8).reshape(H, W, 3)
    s = Scene.from_file("shadows")
    s.set_camera((0, 0, 0.5), 16.0)
    s.update_objects()
    r = Renderer(0)
    try:
        r.set_orientation(30 * math.pi / 180.0, 0, 0)
        r.set_raymap(raymap("fisheye", W, H, fov=float(np.float32(200 * math.pi / 180.0)), fit=1))
        r.set_projection("raymap")
        r.upload_scene(s)
        r.set_scene_params(s, W, H)
        r.set_output(None)
        r.render()
        assert r.last_variant() == 1241
        want = r.read_framebuffer()["rgba"].reshape(H, W, 4)[::-1, :, :3]
    finally:
        r.close()
    assert np.array_equal(img, want)
