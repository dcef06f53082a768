"""The host side of the lit particles that needs no device (relativitypathtracer_amd/csrc/rpt_dust_host.hpp: the flags' validation, the
launch's refusals as predicates, the choice of the splat kernel) in a stand-alone program (tests/native/dust_host_main.cpp) built with
g++, plain and under the address and undefined-behaviour sanitizers, and run directly.  The sanitizer build is skipped only where g++ says
it has no sanitizer runtime; any other failure to build under those flags fails the test."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "dust_host_main.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *extra, "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    return exe, p


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_flags_launch_refusals_and_kernel_choice(tmp_path):
    exe, p = _build(tmp_path, "dust_host", ["-O2", "-ffp-contract=off"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert "warning" not in p.stderr, p.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr[-2000:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_address_and_undefined_behaviour_sanitizers_find_nothing(tmp_path):
    exe, p = _build(tmp_path, "dust_host_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if p.returncode != 0:
        # a skip only where the compiler has no sanitizer runtime to link; anything else the flags bring out of the header is a failure
        missing = any(w in p.stderr for w in ("cannot find -lasan", "cannot find -lubsan", "libasan", "libubsan", "unrecognized command-line option", "unsupported option"))
        assert missing, p.stderr[-3000:]
        pytest.skip("g++ has no sanitizer runtime to link here: " + p.stderr[-300:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
