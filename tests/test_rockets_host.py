"""The host side of the rocket pass that needs no device (relativitypathtracer_amd/csrc/rpt_rockets_host.hpp: the set's validation, its
largest object index and the copy the device reads; the options are the particle pass's) in a stand-alone program
(tests/native/rockets_host_main.cpp) built with g++, plain and under the address and undefined-behaviour sanitizers."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "rockets_host_main.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *extra, "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    return exe, p


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_validation_largest_index_copy_and_options(tmp_path):
    exe, p = _build(tmp_path, "rockets_host", ["-O2", "-ffp-contract=off"])
    assert p.returncode == 0, p.stderr[-2000:]
    assert "warning" not in p.stderr, p.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and r.stdout.startswith("ok "), (r.stdout, r.stderr[-2000:])


@pytest.mark.skipif(shutil.which("g++") is None, reason="no g++")
def test_address_and_undefined_behaviour_sanitizers_find_nothing(tmp_path):
    exe, p = _build(tmp_path, "rockets_host_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    if p.returncode != 0:
        pytest.skip("g++ cannot link -fsanitize=address,undefined here: " + p.stderr[-300:])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and r.stdout.startswith("ok ") and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, (r.stdout, r.stderr[-3000:])
