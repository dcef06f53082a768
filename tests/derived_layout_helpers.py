"""The derived layouts of a scene on the host (rpt_derived_layout_host) as numpy records, and the soup the exit-record tests share —
TEST INFRASTRUCTURE (a helper, no tests in it)."""
import ctypes as C

import numpy as np

NODES, EXITS, HITS, NODE_INDEX = 0, 1, 2, 3          # RPT_LAYOUT_* of include/rpt.h
EXIT_INNER = 0x01FFFFFF                              # RPT_EXIT_INNER
BEGIN_MASK = 0x00FFFFFF

DNODE = np.dtype([("min", "<f4", 3), ("link", "<i4"), ("max", "<f4", 3), ("begin", "<u4"), ("leafCount", "<i4"), ("nb", "<i4", 6), ("pad", "<i4")])
DEXIT = np.dtype([("min", "<f4", 3), ("a", "<i4"), ("max", "<f4", 3), ("b", "<u4")])
DHIT = np.dtype([("normal", "<f4", (3, 3)), ("uv", "<f4", (3, 2)), ("spare", "<i4")])
assert (DNODE.itemsize, DEXIT.itemsize, DHIT.itemsize) == (64, 32, 64)

SOUP_SEED = 14       # tests/mesh_soups.py: half of the vertices in one spot — 481 nodes, nine leaves with 255 to 603 records, 47 exits into them


def layout(scene, which):
    """One array of the scene's derived layouts, or None where the scene has none."""
    from relativitypathtracer_amd import _ffi
    lib = _ffi.hip()
    desc = scene.desc()
    need = C.c_size_t(0)
    rc = lib.rpt_derived_layout_host(C.byref(desc), which, None, 0, C.byref(need))
    if rc == 0:
        return None
    assert rc == 1, rc
    dtype = {NODES: DNODE, EXITS: DEXIT, HITS: DHIT, NODE_INDEX: np.dtype("<i4")}[which]
    assert need.value % dtype.itemsize == 0
    out = np.zeros(need.value // dtype.itemsize, dtype=dtype)
    rc = lib.rpt_derived_layout_host(C.byref(desc), which, out.ctypes.data, out.nbytes, None)
    assert rc == 1, rc
    return out


def soup_scene(tmp_dir, seed=SOUP_SEED):
    """A one-object scene of tests/mesh_soups.py's soup `seed` (the object's pose is mesh_truth.load_case's)."""
    from mesh_soups import write_soup
    from relativitypathtracer_amd import Scene
    write_soup(tmp_dir, seed)
    scene = Scene(asset_root=str(tmp_dir))
    scene.inputScene(f"MModels/soup{seed}.obj\nOm0\n p0.5,-1,6,0.6,0.2,1,0.1,2,1.5,2.5\n c0.8,0.5,0.3\nA0.2\nR\n")
    scene.update_objects()
    return scene


def exits_into_long_lists(nodes, exits):
    """How many exit records lead to a leaf whose list has 255 records or more (whose count the walk reads from the leaf's own DNode)."""
    long_leaves = np.flatnonzero((nodes["link"] == -1) & (nodes["leafCount"] >= 255))
    to_leaf = exits[exits["b"] != EXIT_INNER]
    return int(np.isin(to_leaf["a"], long_leaves).sum())
