"""examples/rpt_render_main.cpp --segments FILE[:inverse_square][:bias=B][:pieces=N]: what the flag parses to and what it refuses, decided
before the host looks for a device (the setting is echoed on stderr as soon as it is read; too few positional arguments then end the run
at the usage line, and a file that holds no whole records ends it before the scene is read)."""
import os
import subprocess

import numpy as np
import pytest

from relativitypathtracer_amd import segments

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
    ("rods.bin", "segments: file rods.bin, inverse square 0, depth bias 0, pieces 16"),
    ("rods.bin:inverse_square", "segments: file rods.bin, inverse square 1, depth bias 0, pieces 16"),
    ("rods.bin:bias=0.002", "segments: file rods.bin, inverse square 0, depth bias 0.002, pieces 16"),
    ("rods.bin:pieces=64", "segments: file rods.bin, inverse square 0, depth bias 0, pieces 64"),
    ("dir/rods.bin:inverse_square:bias=1e-3:pieces=1", "segments: file dir/rods.bin, inverse square 1, depth bias 0.001, pieces 1"),
    ("rods.bin:pieces=8:bias=0.5:inverse_square", "segments: file rods.bin, inverse square 1, depth bias 0.5, pieces 8"),
])
def test_the_flag_parses_to_the_setting(exe, spec, echo):
    p = _run(exe, "--segments", spec)                 # no positional arguments: the usage line ends the run, after the flag was read
    assert p.returncode == 2 and echo in p.stderr and "[--particles SPEC] [--segments SPEC]" in p.stderr


@pytest.mark.parametrize("spec,message", [
    (":inverse_square", "names no file"),
    ("", "names no file"),
    ("rods.bin:bogus", "unknown option 'bogus'"),
    ("rods.bin:", "unknown option ''"),
    ("rods.bin:bias=", "'' in 'rods.bin:bias=' is not a bias"),
    ("rods.bin:bias=-1", "'-1' in 'rods.bin:bias=-1' is not a bias"),
    ("rods.bin:bias=nan", "is not a bias"),
    ("rods.bin:bias=inf", "is not a bias"),
    ("rods.bin:bias=1x", "'1x' in 'rods.bin:bias=1x' is not a bias"),
    ("rods.bin:pieces=", "'' in 'rods.bin:pieces=' is not a number of pieces"),
    ("rods.bin:pieces=0", "'0' in 'rods.bin:pieces=0' is not a number of pieces"),
    ("rods.bin:pieces=3", "is not a number of pieces"),
    ("rods.bin:pieces=128", "is not a number of pieces"),
    ("rods.bin:pieces=-4", "is not a number of pieces"),
    ("rods.bin:pieces=16x", "is not a number of pieces"),
])
def test_a_bad_value_is_refused_before_anything_else(exe, spec, message, tmp_path):
    out = tmp_path / "unused.ppm"
    p = _run(exe, "--segments", spec, "64", "48", str(out))
    assert p.returncode == 2 and p.stderr.startswith("--segments: ") and message in p.stderr
    assert not out.exists()


def test_the_flag_without_a_value_and_the_usage_line(exe):
    p = _run(exe, "--segments")
    assert p.returncode == 2 and "--segments needs a value" in p.stderr
    p = _run(exe, "64", "48")
    assert p.returncode == 2 and "[--segments SPEC]" in p.stderr and "segments:" not in p.stderr


def test_a_file_that_holds_no_whole_records_is_refused_before_the_scene_is_read(exe, tmp_path):
    out = tmp_path / "unused.ppm"
    missing = tmp_path / "missing.bin"
    p = _run(exe, "--segments", str(missing), "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number (> 0) of 48-byte rpt_segment records" in p.stderr
    ragged = tmp_path / "ragged.bin"
    ragged.write_bytes(b"\0" * 95)
    p = _run(exe, "--segments", f"{ragged}:inverse_square", "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number" in p.stderr
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    p = _run(exe, "--segments", str(empty), "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number" in p.stderr
    assert not out.exists()


@pytest.mark.gpu
def test_the_host_draws_the_rods_of_a_file(exe, tmp_path):
    """shadows.txt at 128 x 72 with a rod lattice riding the first object the frame sees, against the library called from Python."""
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 128, 72
    scene = Scene.from_file("shadows")
    scene.set_camera((0.0, 0.0, 0.0), 16.0)
    scene.update_objects()
    _, _, records = render_scene(scene, W, H, events=True)
    hit = records.reshape(-1)[records.reshape(-1)["object"] >= 0]
    centre = hit["event"][0, 1:4].astype(np.float64)
    rods = segments.rod_lattice(int(hit["object"][0]), centre - 0.4, centre + 0.4, 3, (2.0, 1.5, 0.5))
    path = tmp_path / "rods.bin"
    segments.save(path, rods)
    want, _, _ = render_scene(scene, W, H, segments=rods, segment_options=dict(inverse_square=True, depth_bias=1e-3, pieces=8))
    out = tmp_path / "out.ppm"
    assets = os.path.join(ROOT, "assets", "reference")
    with open(os.path.join(assets, "Scenes", "shadows.txt")) as f:
        p = subprocess.run([exe, "--segments", f"{path}:inverse_square:bias=1e-3:pieces=8", str(W), str(H), str(out), "0", "0", "0", "16"], stdin=f,
                           capture_output=True, text=True, timeout=300, env={**os.environ, "RPT_ASSETS": assets})
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"of {8 * len(rods)} pieces drawn" in p.stderr and "segments: 0 of" not in p.stderr
    data = out.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    got = np.frombuffer(data[len(header):], dtype=np.uint8).reshape(H, W, 3)
    assert np.array_equal(got, want["rgba"].reshape(H, W, 4)[::-1, :, :3])       # (the PPM's first row is the top row)
    plain, _ = render_scene(scene, W, H)
    assert not np.array_equal(want["rgba"], plain["rgba"])
