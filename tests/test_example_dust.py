"""examples/rpt_render_main.cpp --particle-lighting lit[,shadows][,ambient]: what the flag parses to and what it refuses, decided before
the host looks for a device (the setting is echoed on stderr as soon as it is read; too few positional arguments then end the run at
the usage line).  The grammar of --particles is untouched (tests/test_example_particles.py)."""
import os
import subprocess

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
    ("lit", "particle lighting: lit 1, shadows 0, ambient 0"),
    ("lit,shadows", "particle lighting: lit 1, shadows 1, ambient 0"),
    ("lit,ambient", "particle lighting: lit 1, shadows 0, ambient 1"),
    ("lit,shadows,ambient", "particle lighting: lit 1, shadows 1, ambient 1"),
    ("ambient,shadows,lit", "particle lighting: lit 1, shadows 1, ambient 1"),
    ("shadows", "particle lighting: lit 0, shadows 1, ambient 0"),       # (the library refuses it at the call, with its own message)
])
def test_the_flag_parses_to_the_setting(exe, spec, echo):
    p = _run(exe, "--particle-lighting", spec)        # no positional arguments: the usage line ends the run, after the flag was read
    assert p.returncode == 2 and echo in p.stderr and "[--particle-lighting SPEC]" in p.stderr


@pytest.mark.parametrize("spec,message", [("", "unknown word ''"), ("lit,", "unknown word ''"), ("lit:shadows", "unknown word 'lit:shadows'"),
                                          ("bright", "unknown word 'bright'"), ("lit,inverse_square", "unknown word 'inverse_square'")])
def test_a_bad_value_is_refused_before_anything_else(exe, spec, message, tmp_path):
    out = tmp_path / "unused.ppm"
    p = _run(exe, "--particle-lighting", spec, "64", "48", str(out))
    assert p.returncode == 2 and p.stderr.startswith("--particle-lighting: ") and message in p.stderr
    assert not out.exists()


def test_the_flag_without_a_value_and_without_particles(exe, tmp_path):
    p = _run(exe, "--particle-lighting")
    assert p.returncode == 2 and "--particle-lighting needs a value: lit[,shadows][,ambient]" in p.stderr
    out = tmp_path / "unused.ppm"
    p = _run(exe, "--particle-lighting", "lit", "64", "48", str(out))
    assert p.returncode == 2 and "--particle-lighting needs --particles" in p.stderr and not out.exists()
