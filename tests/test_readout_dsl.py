"""The scene DSL's `dRATE,OFFSET,DIGITS,DECIMALS[,U0,V0,U1,V1]` command and Scene.readouts() (DESIGN.md "Readout pass").  No GPU."""
import glob
import os

import numpy as np

from relativitypathtracer_amd import Scene

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def test_a_scene_without_d_has_no_readouts():
    s = Scene()
    s.inputScene("Os p0,0,5,0,0,1,0,1,1,1\nOc p2,0,5,0,0,1,0,1,1,1 w0,1\nR\n")
    assert s.readouts() is None
    assert Scene.from_file("ladder_paradox").readouts() is None


def test_no_shipped_scene_has_a_token_that_starts_with_d():
    files = glob.glob(os.path.join(ROOT, "assets", "reference", "Scenes", "*.txt"))
    assert len(files) >= 8
    for path in files:
        assert not [tok for tok in open(path).read().split() if tok.startswith("d")], path


def test_the_d_command_sets_the_current_objects_display_with_its_defaults():
    s = Scene()
    text = "Os p0,0,5,0,0,1,0,1,1,1 d1,0,4,2\nOc p2,0,5,0,0,1,0,1,1,1\nOc d-0.5,12.25,9,6,0.9,0.2,0.1,0.8 p1,1,5,0,0,1,0,1,1,1\nOs d2,3,1,0 d1,-1e3,3,1\nR\n"
    assert s.inputScene(text) == ""
    r = s.readouts()
    assert len(r) == 4 and r[1] is None
    assert r[0] == dict(rate=F(1), offset=F(0), digits=4, decimals=2, rect=(F(0.1), F(0.25), F(0.9), F(0.75)), on_rgba=(255, 0, 0, 255), off_rgba=(0, 0, 0, 160))
    assert r[2] == dict(rate=F(-0.5), offset=F(12.25), digits=9, decimals=6, rect=(F(0.9), F(0.2), F(0.1), F(0.8)), on_rgba=(255, 0, 0, 255), off_rgba=(0, 0, 0, 160))
    assert (r[3]["rate"], r[3]["offset"], r[3]["digits"], r[3]["decimals"]) == (1, -1000, 3, 1)          # the later command wins
    assert r is s.readouts()                                    # cached per parse
    assert len(s.objects()) == 4 and s.objects().dtype.itemsize == 320         # the object record is the reference's


def test_a_malformed_d_is_a_warning_and_is_ignored():
    s = Scene()
    assert "d1,0,4,2" in s.inputScene("d1,0,4,2\nOs p0,0,5,0,0,1,0,1,1,1\nR\n")       # before any object
    assert s.readouts() is None
    for bad in ("d", "d1", "d1,0,4", "d1,0,4,2,0.1", "d1,0,4,2,0.1,0.2,0.9", "d1,0,4,2,0.1,0.2,0.9,0.8,7", "d1,0,0,0", "d1,0,10,0", "d1,0,4,4", "d1,0,9,7",
                "d1,0,4.5,2", "d1,0,4,-1", "dx,0,4,2", "d1,,4,2", "d1,0,4,2,", "dnan,0,4,2", "d1,inf,4,2", "d1e39,0,4,2", "d1,0,4,2,0.5,0.2,0.5,0.8",
                "d1,0,4,2,0.1,0.3,0.9,0.3"):
        s = Scene()
        diagnostics = s.inputScene(f"Os p0,0,5,0,0,1,0,1,1,1 {bad}\nR\n")
        assert s.readouts() is None, bad
        assert f'"{bad}"' in diagnostics, (bad, diagnostics)
    s = Scene()                                                 # ignored: the display set before stays
    s.inputScene("Os p0,0,5,0,0,1,0,1,1,1 d1,0,4,2 d1,0,44,2\nR\n")
    assert s.readouts()[0]["digits"] == 4
