"""examples/rpt_render_main.cpp --ballistics FILE[:inverse_square][:bias=B] [--ballistic-temperatures FILE]: what the flags parse to and
what they refuse, decided before the host looks for a device (the setting is echoed on stderr as soon as it is read; too few positional
arguments then end the run at the usage line, and a file that holds no whole records ends it before the scene is read)."""
import os
import subprocess

import numpy as np
import pytest

from relativitypathtracer_amd import ballistics

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
    ("jet.bin", "ballistics: file jet.bin, inverse square 0, depth bias 0"),
    ("jet.bin:inverse_square", "ballistics: file jet.bin, inverse square 1, depth bias 0"),
    ("jet.bin:bias=0.002", "ballistics: file jet.bin, inverse square 0, depth bias 0.002"),
    ("dir/jet.bin:inverse_square:bias=1e-3", "ballistics: file dir/jet.bin, inverse square 1, depth bias 0.001"),
    ("jet.bin:bias=0.5:inverse_square", "ballistics: file jet.bin, inverse square 1, depth bias 0.5"),
])
def test_the_flag_parses_to_the_setting(exe, spec, echo):
    p = _run(exe, "--ballistics", spec)               # no positional arguments: the usage line ends the run, after the flag was read
    assert p.returncode == 2 and echo in p.stderr and "[--segments SPEC] [--ballistics SPEC]" in p.stderr and "[--ballistic-temperatures FILE]" in p.stderr


@pytest.mark.parametrize("spec,message", [
    (":inverse_square", "names no file"),
    ("", "names no file"),
    ("jet.bin:bogus", "unknown option 'bogus'"),
    ("jet.bin:", "unknown option ''"),
    ("jet.bin:bias=", "'' in 'jet.bin:bias=' is not a bias"),
    ("jet.bin:bias=-1", "'-1' in 'jet.bin:bias=-1' is not a bias"),
    ("jet.bin:bias=nan", "is not a bias"),
    ("jet.bin:bias=inf", "is not a bias"),
    ("jet.bin:bias=1x", "'1x' in 'jet.bin:bias=1x' is not a bias"),
])
def test_a_bad_value_is_refused_before_anything_else(exe, spec, message, tmp_path):
    out = tmp_path / "unused.ppm"
    p = _run(exe, "--ballistics", spec, "64", "48", str(out))
    assert p.returncode == 2 and p.stderr.startswith("--ballistics: ") and message in p.stderr
    assert not out.exists()


def test_the_flags_without_a_value_and_the_usage_line(exe):
    p = _run(exe, "--ballistics")
    assert p.returncode == 2 and "--ballistics needs a value" in p.stderr and "48-byte rpt_ballistic" in p.stderr
    p = _run(exe, "--ballistic-temperatures")
    assert p.returncode == 2 and "--ballistic-temperatures needs a file name" in p.stderr
    p = _run(exe, "64", "48")
    assert p.returncode == 2 and "[--ballistics SPEC]" in p.stderr and "ballistics:" not in p.stderr


def test_a_file_that_holds_no_whole_records_is_refused_before_the_scene_is_read(exe, tmp_path):
    out = tmp_path / "unused.ppm"
    missing = tmp_path / "missing.bin"
    p = _run(exe, "--ballistics", str(missing), "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number (> 0) of 48-byte rpt_ballistic records" in p.stderr
    ragged = tmp_path / "ragged.bin"
    ragged.write_bytes(b"\0" * 64)          # (a whole number of particle records, not of these)
    p = _run(exe, "--ballistics", f"{ragged}:inverse_square", "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number" in p.stderr
    empty = tmp_path / "empty.bin"
    empty.write_bytes(b"")
    p = _run(exe, "--ballistics", str(empty), "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number" in p.stderr
    assert not out.exists()


def test_temperatures_need_the_set_and_one_value_per_record(exe, tmp_path):
    out = tmp_path / "unused.ppm"
    kelvin = tmp_path / "kelvin.bin"
    np.full(3, 6000.0, dtype=np.float32).tofile(kelvin)
    p = _run(exe, "--ballistic-temperatures", str(kelvin), "64", "48", str(out))
    assert p.returncode == 2 and "--ballistic-temperatures needs --ballistics" in p.stderr
    records = tmp_path / "jet.bin"
    ballistics.save(records, ballistics.jet(0, (0.0, 0.0, 5.0), (1.0, 0.0, 0.0), 0.9, [0.0, 1.0], (1.0, 1.0, 1.0)))
    assert records.stat().st_size == 96
    p = _run(exe, "--ballistics", str(records), "--ballistic-temperatures", str(kelvin), "64", "48", str(out))
    assert p.returncode == 2 and "does not hold 2 float32 temperatures, one per record" in p.stderr
    assert not out.exists()


@pytest.mark.gpu
def test_the_host_draws_the_ballistics_of_a_file(exe, tmp_path):
    """shadows.txt at 128 x 72 with a shell that bursts in front of the first object the frame sees, against the library called from Python."""
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 128, 72
    scene = Scene.from_file("shadows")
    scene.set_camera((0.0, 0.0, 0.0), 16.0)
    scene.update_objects()
    _, _, records = render_scene(scene, W, H, events=True)
    hit = records.reshape(-1)[records.reshape(-1)["object"] >= 0]
    centre, t = hit["event"][0, 1:4].astype(np.float64), float(hit["event"][0, 0])
    bs = ballistics.shell(int(hit["object"][0]), centre, t - 1.0, 0.5, 200, (0.9, 0.8, 0.3))
    path = tmp_path / "shell.bin"
    ballistics.save(path, bs)
    want, _, _ = render_scene(scene, W, H, ballistics=bs, ballistic_options=dict(inverse_square=True, depth_bias=1e-3))
    out = tmp_path / "out.ppm"
    assets = os.path.join(ROOT, "assets", "reference")
    with open(os.path.join(assets, "Scenes", "shadows.txt")) as f:
        p = subprocess.run([exe, "--ballistics", f"{path}:inverse_square:bias=1e-3", str(W), str(H), str(out), "0", "0", "0", "16"], stdin=f,
                           capture_output=True, text=True, timeout=300, env={**os.environ, "RPT_ASSETS": assets})
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"of {len(bs)} seen" in p.stderr and "ballistics: 0 of" not in p.stderr
    data = out.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    got = np.frombuffer(data[len(header):], dtype=np.uint8).reshape(H, W, 3)
    assert np.array_equal(got, want["rgba"].reshape(H, W, 4)[::-1, :, :3])       # (the PPM's first row is the top row)
    plain, _ = render_scene(scene, W, H)
    assert not np.array_equal(want["rgba"], plain["rgba"])
