"""examples/rpt_render_main.cpp --overlay SPEC: what the flag parses to and what it refuses, decided before the host looks for a device
(the description is echoed on stderr as soon as it is read; too few positional arguments then end the run at the usage line)."""
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
    return subprocess.run([exe, *args], capture_output=True, text=True, timeout=60)


@pytest.mark.parametrize("spec,echo", [
    ("outlines", "overlay: layers 1, clock step 0, delay step 0, lattice steps 0 0 0, tint range 0"),
    ("clock:0.5", "overlay: layers 4, clock step 0.5, delay step 0, lattice steps 0 0 0, tint range 0"),
    ("delay:2", "overlay: layers 2, clock step 0, delay step 2, lattice steps 0 0 0, tint range 0"),
    ("lattice:1:0:0.25", "overlay: layers 8, clock step 0, delay step 0, lattice steps 1 0 0.25, tint range 0"),
    ("tint", "overlay: layers 16, clock step 0, delay step 0, lattice steps 0 0 0, tint range 0"),
    ("tint:30", "overlay: layers 16, clock step 0, delay step 0, lattice steps 0 0 0, tint range 30"),
    ("tint:7.5,lattice:4:4:4,delay:2,clock:0.5,outlines", "overlay: layers 31, clock step 0.5, delay step 2, lattice steps 4 4 4, tint range 7.5"),
])
def test_the_flag_parses_to_the_description(exe, spec, echo):
    p = _run(exe, "--overlay", spec)                  # no positional arguments: the usage line ends the run, after the flag was read
    assert p.returncode == 2 and echo in p.stderr and "[--overlay SPEC]" in p.stderr


@pytest.mark.parametrize("spec,message", [
    ("bogus", "unknown layer 'bogus'"),
    ("", "unknown layer ''"),
    ("outlines,", "unknown layer ''"),
    ("outlines:3", "'outlines' takes no value"),
    ("clock", "'clock' takes one step"),
    ("delay:1:2", "'delay' takes one step"),
    ("lattice:1:2", "'lattice' takes three steps"),
    ("tint:1:2", "'tint' takes at most one value"),
    ("clock:fast", "'fast' in 'clock:fast' is not a number"),
    ("clock:", "'' in 'clock:' is not a number"),
    ("delay:inf", "'inf' in 'delay:inf' is not a number"),
])
def test_a_bad_value_is_refused_before_anything_else(exe, spec, message):
    p = _run(exe, "--overlay", spec, "64", "48", "unused.ppm")
    assert p.returncode == 2 and p.stderr.startswith("--overlay: ") and message in p.stderr
    assert not os.path.exists("unused.ppm")


def test_the_flag_without_a_value_and_the_usage_line(exe):
    p = _run(exe, "--overlay")
    assert p.returncode == 2 and "--overlay needs a value" in p.stderr
    p = _run(exe, "64", "48")
    assert p.returncode == 2 and "[--events FILE] [--overlay SPEC]" in p.stderr and "overlay:" not in p.stderr
