"""The domain check of the triangle test's exact reciprocal (rpt_scene_exact_rcp, host code: no device needed).  Kernels 41 / 43
take 1 / det through rcp_exact only for scenes whose triangles all have |e1| |e2| <= 2^60; every other scene gets the IEEE division."""
import ctypes as C
import os

import pytest

from relativitypathtracer_amd import _ffi
from relativitypathtracer_amd.scene import Scene

SHIPPED = ["bunny", "shadows", "arch", "cube", "cubes", "ladder_paradox", "rulers", "soccer"]


def exact_rcp(scene):
    d = scene.desc()
    return _ffi.hip().rpt_scene_exact_rcp(C.byref(d))


def obj_scene(tmp_path, name, text):
    path = os.path.join(str(tmp_path), name)
    with open(path, "w") as f:
        f.write(text)
    s = Scene()
    s.ReadOBJ(path)
    return s


@pytest.mark.parametrize("name", SHIPPED)
def test_shipped_scenes_select_the_exact_reciprocal(name):
    assert exact_rcp(Scene.from_file(name)) == 1


def test_models_select_the_exact_reciprocal(tmp_path):
    root = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "assets", "reference", "Models")
    for m in sorted(os.listdir(root)):
        s = Scene()
        s.ReadOBJ(os.path.join(root, m))
        assert exact_rcp(s) == 1, m


def test_flat_mesh_is_in_the_domain(tmp_path):
    """A mesh with zero extent on one axis: its triangles are ordinary, the reciprocal's domain holds (only |e1| |e2| matters)."""
    text = "v 0 0 0\nv 1 0 0\nv 0 1 0\nv 1 1 0\nf 1 2 3\nf 2 4 3\n"
    assert exact_rcp(obj_scene(tmp_path, "flat.obj", text)) == 1


def test_huge_mesh_takes_the_ieee_division(tmp_path):
    """|e1| |e2| = 2^62 > 2^60: |det| could leave the range on which rcp_exact equals 1 / det."""
    text = "v 0 0 0\nv 2147483648 0 0\nv 0 2147483648 0\nf 1 2 3\n"
    assert exact_rcp(obj_scene(tmp_path, "huge.obj", text)) == 0


def test_boundary_mesh(tmp_path):
    """|e1| |e2| = 2^60 exactly is inside, the next float of an edge outside."""
    inside = "v 0 0 0\nv 1073741824 0 0\nv 0 1073741824 0\nf 1 2 3\n"
    outside = "v 0 0 0\nv 1073741952 0 0\nv 0 1073741824 0\nf 1 2 3\n"
    assert exact_rcp(obj_scene(tmp_path, "edge_in.obj", inside)) == 1
    assert exact_rcp(obj_scene(tmp_path, "edge_out.obj", outside)) == 0


def test_bad_arguments():
    assert _ffi.hip().rpt_scene_exact_rcp(None) < 0
