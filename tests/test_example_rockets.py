"""examples/rpt_render_main.cpp --rockets FILE[:inverse_square][:bias=B] [--rocket-temperatures FILE]: what the flags parse to and what
they refuse, decided before the host looks for a device (the setting is echoed on stderr as soon as it is read; too few positional
arguments then end the run at the usage line, and a file that holds no whole records ends it before the scene is read)."""
import os
import subprocess

import numpy as np
import pytest

from relativitypathtracer_amd import rockets

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
    ("fleet.bin", "rockets: file fleet.bin, inverse square 0, depth bias 0"),
    ("fleet.bin:inverse_square", "rockets: file fleet.bin, inverse square 1, depth bias 0"),
    ("dir/fleet.bin:inverse_square:bias=1e-3", "rockets: file dir/fleet.bin, inverse square 1, depth bias 0.001"),
])
def test_the_flag_parses_to_the_setting(exe, spec, echo):
    p = _run(exe, "--rockets", spec)               # no positional arguments: the usage line ends the run, after the flag was read
    assert p.returncode == 2 and echo in p.stderr and "[--ballistics SPEC] [--rockets SPEC]" in p.stderr and "[--rocket-temperatures FILE]" in p.stderr


@pytest.mark.parametrize("spec,message", [
    (":inverse_square", "names no file"),
    ("fleet.bin:bogus", "unknown option 'bogus'"),
    ("fleet.bin:bias=-1", "'-1' in 'fleet.bin:bias=-1' is not a bias"),
])
def test_a_bad_value_is_refused_before_anything_else(exe, spec, message, tmp_path):
    out = tmp_path / "unused.ppm"
    p = _run(exe, "--rockets", spec, "64", "48", str(out))
    assert p.returncode == 2 and p.stderr.startswith("--rockets: ") and message in p.stderr
    assert not out.exists()


def test_the_flags_without_a_value_and_the_usage_line(exe):
    p = _run(exe, "--rockets")
    assert p.returncode == 2 and "--rockets needs a value" in p.stderr and "64-byte rpt_rocket" in p.stderr
    p = _run(exe, "--rocket-temperatures")
    assert p.returncode == 2 and "--rocket-temperatures needs a file name" in p.stderr
    p = _run(exe, "64", "48")
    assert p.returncode == 2 and "[--rockets SPEC]" in p.stderr and "rockets:" not in p.stderr


def test_a_file_that_holds_no_whole_records_is_refused_before_the_scene_is_read(exe, tmp_path):
    out = tmp_path / "unused.ppm"
    p = _run(exe, "--rockets", str(tmp_path / "missing.bin"), "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number (> 0) of 64-byte rpt_rocket records" in p.stderr
    ragged = tmp_path / "ragged.bin"
    ragged.write_bytes(b"\0" * 96)          # (a whole number of ballistic records, not of these)
    p = _run(exe, "--rockets", f"{ragged}:inverse_square", "64", "48", str(out))
    assert p.returncode == 2 and "does not hold a whole number" in p.stderr
    assert not out.exists()


def test_temperatures_need_the_set_and_one_value_per_record(exe, tmp_path):
    out = tmp_path / "unused.ppm"
    kelvin = tmp_path / "kelvin.bin"
    np.full(3, 6000.0, dtype=np.float32).tofile(kelvin)
    p = _run(exe, "--rocket-temperatures", str(kelvin), "64", "48", str(out))
    assert p.returncode == 2 and "--rocket-temperatures needs --rockets" in p.stderr
    records = tmp_path / "two.bin"
    rockets.save(records, rockets.launch(0, (0.0, 0.0, 5.0), (1.0, 0.0, 0.0), [0.0, 1.0], (1.0, 1.0, 1.0)))
    assert records.stat().st_size == 128
    p = _run(exe, "--rockets", str(records), "--rocket-temperatures", str(kelvin), "64", "48", str(out))
    assert p.returncode == 2 and "does not hold 2 float32 temperatures, one per record" in p.stderr
    assert not out.exists()


@pytest.mark.gpu
def test_the_host_draws_the_rockets_of_a_file(exe, tmp_path):
    """shadows.txt at 128 x 72 with a Bell fleet that starts in front of the first object the frame sees, against the library called from Python."""
    from relativitypathtracer_amd import Scene
    from relativitypathtracer_amd.renderer import render_scene
    W, H = 128, 72
    scene = Scene.from_file("shadows")
    scene.set_camera((0.0, 0.0, 0.0), 16.0)
    scene.update_objects()
    _, _, records = render_scene(scene, W, H, events=True)
    hit = records.reshape(-1)[records.reshape(-1)["object"] >= 0]
    centre, t = hit["event"][0, 1:4].astype(np.float64), float(hit["event"][0, 0])
    spread = np.random.default_rng(5).uniform(-0.5, 0.5, (200, 3))
    rs = rockets.from_arrays(centre + spread, int(hit["object"][0]), (9.0, 8.0, 3.0), acc=(0.0, 0.3, 0.0), epoch=t - 1.0)
    path = tmp_path / "fleet.bin"
    rockets.save(path, rs)
    want, _, _ = render_scene(scene, W, H, rockets=rs, rocket_options=dict(inverse_square=True, depth_bias=1e-3))
    out = tmp_path / "out.ppm"
    assets = os.path.join(ROOT, "assets", "reference")
    with open(os.path.join(assets, "Scenes", "shadows.txt")) as f:
        p = subprocess.run([exe, "--rockets", f"{path}:inverse_square:bias=1e-3", str(W), str(H), str(out), "0", "0", "0", "16"], stdin=f,
                           capture_output=True, text=True, timeout=300, env={**os.environ, "RPT_ASSETS": assets})
    assert p.returncode == 0, p.stderr[-2000:]
    assert f"of {len(rs)} seen" in p.stderr and "rockets: 0 of" not in p.stderr
    data = out.read_bytes()
    header = f"P6\n{W} {H}\n255\n".encode()
    assert data.startswith(header)
    got = np.frombuffer(data[len(header):], dtype=np.uint8).reshape(H, W, 3)
    assert np.array_equal(got, want["rgba"].reshape(H, W, 4)[::-1, :, :3])       # (the PPM's first row is the top row)
    plain, _ = render_scene(scene, W, H)
    assert not np.array_equal(want["rgba"], plain["rgba"])
