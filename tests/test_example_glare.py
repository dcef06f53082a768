"""examples/rpt_render_main.cpp --glare W:SIGMA[,W:SIGMA[,W:SIGMA]]: what the flag parses to and what it refuses, decided before the
host looks for a device (the setting is echoed on stderr as soon as it is read; too few positional arguments then end the run at the
usage line)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "relativitypathtracer_amd")


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("example") / "rpt_render")
    cmd = ["g++", "-O2", "-std=c++17", f"-I{ROOT}/include", f"{ROOT}/examples/rpt_render_main.cpp", "-o", path,
           f"-L{PKG}", "-lrpt_hip", "-lrpt_scene", f"-Wl,-rpath,{PKG}", "-L/opt/rocm/lib", "-Wl,-rpath,/opt/rocm/lib"]
    subprocess.run(cmd, check=True, capture_output=True, timeout=300)
    return path


def _run(exe, *args):
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)


@pytest.mark.parametrize("spec,echo", [
    ("0.3:1.2", "glare: 1 layers, weight 0.3 sigma 1.2"),
    ("0.5:0.5,0.5:10.5", "glare: 2 layers, weight 0.5 sigma 0.5; weight 0.5 sigma 10.5"),
    ("0.3:1,0.2:4,0.1:10.6666", "glare: 3 layers, weight 0.3 sigma 1; weight 0.2 sigma 4; weight 0.1 sigma 10.6666"),
])
def test_the_flag_parses_to_the_setting(exe, spec, echo):
    p = _run(exe, "--glare", spec)                 # no positional arguments: the usage line ends the run, after the flag was read
    assert p.returncode == 2 and echo in p.stderr and "[--rocket-temperatures FILE] [--glare SPEC]" in p.stderr


@pytest.mark.parametrize("spec,message", [
    ("0.3", "'0.3' in '0.3' is not W:SIGMA with a weight"),
    ("0.3:", "is not W:SIGMA with a sigma"),
    (":1.0", "is not W:SIGMA with a weight"),
    ("0:1.0", "is not W:SIGMA with a weight"),
    ("-0.2:1.0", "is not W:SIGMA with a weight"),
    ("nan:1.0", "is not W:SIGMA with a weight"),
    ("0.3:0.4", "is not W:SIGMA with a sigma in [0.5, 32/3]"),
    ("0.3:11", "is not W:SIGMA with a sigma in [0.5, 32/3]"),
    ("0.3:nan", "is not W:SIGMA with a sigma"),
    ("0.3:1.0x", "is not W:SIGMA with a sigma"),
    ("0.3:1.0,", "'' in '0.3:1.0,' is not W:SIGMA"),
    ("0.6:1.0,0.5:2.0", "sum to more than 1"),
    ("0.1:1,0.1:2,0.1:3,0.1:4", "more than 3 layers"),
])
def test_a_bad_value_is_refused_before_anything_else(exe, spec, message, tmp_path):
    out = tmp_path / "unused.ppm"
    p = _run(exe, "--glare", spec, "64", "48", str(out))
    assert p.returncode == 2 and p.stderr.startswith("--glare: ") and message in p.stderr
    assert not out.exists()


def test_the_flag_without_a_value_and_the_usage_line(exe):
    p = _run(exe, "--glare")
    assert p.returncode == 2 and "--glare needs a value" in p.stderr and "W:SIGMA[,W:SIGMA[,W:SIGMA]]" in p.stderr
    p = _run(exe, "64", "48")
    assert p.returncode == 2 and "[--glare SPEC]" in p.stderr and "glare:" not in p.stderr


@pytest.mark.gpu
def test_the_host_glares_the_stars_of_a_file(exe, tmp_path):
    """shadows.txt (no textures: the host reads binary PPM only) at 128 x 72 with 200 bright stars and two layers, against the library called from Python."""
    from relativitypathtracer_amd import Scene, stars
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 128, 72
    scene = Scene.from_file("shadows")
    scene.set_camera((0.0, 0.0, 0.0), 16.0)
    scene.update_objects()
    cat = stars.random_catalogue(200, 3).copy()
    cat["rgb"] *= 1e3
    path = tmp_path / "stars.bin"
    cat.tofile(path)
    layers = [(0.3, 1.2), (0.1, 4.0)]
    want, _, _ = render_scene(scene, W, H, stars=cat, glare=layers)
    plain, _, _ = render_scene(scene, W, H, stars=cat)
    assert not np.array_equal(want["rgba"], plain["rgba"])
    out = tmp_path / "out.ppm"
    assets = os.path.join(ROOT, "assets", "reference")
    with open(os.path.join(assets, "Scenes", "shadows.txt")) as f:
        p = subprocess.run([exe, "--stars", str(path), "--glare", "0.3:1.2,0.1:4", str(W), str(H), str(out), "0", "0", "0", "16"], stdin=f,
                           capture_output=True, text=True, timeout=300, env={**os.environ, "RPT_ASSETS": assets})
    assert p.returncode == 0, p.stderr[-2000:]
    assert "glare: 2 layers" in p.stderr and "stars: 0 of" not in p.stderr
    data = out.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    got = np.frombuffer(data[len(header):], dtype=np.uint8).reshape(H, W, 3)
    assert np.array_equal(got, want["rgba"].reshape(H, W, 4)[::-1, :, :3])       # (the PPM's first row is the top row)
