"""The host side of the thermal point sources that needs no device (relativitypathtracer_amd/csrc/rpt_thermal_host.hpp: the temperature
array's validation — every refusal, both ends of the range — and the conversion T -> x_G) in a stand-alone program
(tests/native/thermal_host_main.cpp) built with g++, plain and under the address and undefined-behaviour sanitizers.  The x_G the program
prints are held against Python's double arithmetic, rounded to float once."""
import os
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "native", "thermal_host_main.cpp")


def _build(tmp_path, name, extra):
    exe = str(tmp_path / name)
    p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", *extra, "-o", exe, SRC], capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "warning" not in p.stderr, p.stderr[-2000:]
    return exe


def _run(exe):
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    lines = r.stdout.splitlines()
    assert r.returncode == 0 and lines and lines[-1].startswith("ok "), (r.stdout[-2000:], r.stderr[-2000:])
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
    return [tuple(float.fromhex(v) for v in line.split()[1:]) for line in lines if line.startswith("x ")]


def _check_conversion(pairs):
    assert len(pairs) > 5000
    T = np.array([p[0] for p in pairs])
    assert T.min() == 500.0 and T.max() == 1e8
    for t, x in pairs:
        assert np.float32(t) == t and np.float32(x) == x
        assert np.float32(1.438776877e7 / (546.1 * t)) == np.float32(x), (t, x)


def test_validation_refusals_range_ends_and_the_conversion(tmp_path):
    _check_conversion(_run(_build(tmp_path, "thermal_host", ["-O2", "-ffp-contract=off"])))


def test_address_and_undefined_behaviour_sanitizers_find_nothing(tmp_path):
    _check_conversion(_run(_build(tmp_path, "thermal_host_asan", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])))
