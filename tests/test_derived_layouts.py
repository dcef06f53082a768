"""The exit records and the hit records of the derived layouts (csrc/rpt_kernels.hip.h: DExit, DHit), built on the host alone
(rpt_derived_layout_host: what rpt_upload_scene puts on the device): every (node, side) record holds the fields of the DNode that
nb[side] names, "none" is the sentinel, every hit record the fifteen floats that triangles[] names in normals[] / uvs[].  No GPU."""
import numpy as np
import pytest

import derived_layout_helpers as dl
import mesh_truth as mt

MESHES = ("triangle", "cube", "pear", "bunny")
_scenes = {}


def _scene(name, tmp_path_factory):
    if name not in _scenes:
        if name == "soup":
            _scenes[name] = dl.soup_scene(tmp_path_factory.mktemp("soup"))
        else:
            _scenes[name] = mt.load_case(name, tmp_path_factory.mktemp(name))[0]
    return _scenes[name]


def _bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _check_exits(nodes, exits):
    n = len(nodes)
    assert len(exits) == 6 * n
    ex = exits.reshape(n, 6)
    nb = nodes["nb"]
    assert ((nb >= -1) & (nb < n)).all()
    none = nb == -1
    # "none": the sentinel, and nothing else in the record
    assert (ex["a"][none] == -1).all() and (ex["b"][none] == dl.EXIT_INNER).all()
    assert not _bits(ex["min"][none]).any() and not _bits(ex["max"][none]).any()
    # a neighbour: its DNode's very floats, and its index and begin word (a leaf) or its link (inner)
    d = nodes[np.where(none, 0, nb)]
    some = ~none
    assert np.array_equal(_bits(ex["min"][some]), _bits(d["min"][some])) and np.array_equal(_bits(ex["max"][some]), _bits(d["max"][some]))
    leaf = some & (d["link"] == -1)
    inner = some & (d["link"] != -1)
    assert np.array_equal(ex["a"][leaf], nb[leaf]) and np.array_equal(ex["b"][leaf], d["begin"][leaf])
    assert np.array_equal(ex["a"][inner], d["link"][inner]) and (ex["b"][inner] == dl.EXIT_INNER).all()
    # the three cases can be told apart by what the walk tests: a == -1 is "none" alone, b == RPT_EXIT_INNER is no leaf's word
    assert (ex["a"][some] != -1).all() and (ex["b"][leaf] != dl.EXIT_INNER).all()
    assert (nodes["begin"][nodes["link"] == -1] != dl.EXIT_INNER).all()
    return int(none.sum()), int(leaf.sum()), int(inner.sum())


@pytest.mark.parametrize("name", MESHES + ("soup",))
def test_exit_records_hold_the_neighbours_node(name, tmp_path_factory):
    scene = _scene(name, tmp_path_factory)
    a = mt.arrays(scene)
    nodes, exits, index = dl.layout(scene, dl.NODES), dl.layout(scene, dl.EXITS), dl.layout(scene, dl.NODE_INDEX)
    oc = a["octrees"]
    assert len(nodes) == len(oc) == len(index) and sorted(index.tolist()) == list(range(len(oc)))
    # the DNodes themselves against the reference's nodes (so that "the DNode nb[side] names" is anchored outside the library)
    d = nodes[index]
    assert np.array_equal(_bits(d["min"]), _bits(oc["min"][:, :3])) and np.array_equal(_bits(d["max"]), _bits(oc["max"][:, :3]))
    ref_nb = np.asarray(oc["neighbors"])
    assert np.array_equal(d["nb"], np.where(ref_nb == -1, -1, index[np.where(ref_nb == -1, 0, ref_nb)]))
    is_leaf = np.asarray(oc["children"])[:, 0] == -1
    assert np.array_equal(d["link"] == -1, is_leaf)
    assert np.array_equal(d["leafCount"][is_leaf], np.asarray(oc["trisCount"])[is_leaf])
    assert np.array_equal(d["begin"][is_leaf] >> 24, np.minimum(d["leafCount"][is_leaf], 255).astype(np.uint32))
    none, leaf, inner = _check_exits(nodes, exits)
    print(f"\n{name}: {len(nodes)} nodes, exits: {none} none, {leaf} to a leaf, {inner} to an inner node")
    roots = index[np.asarray(scene.mesh_roots(), dtype=np.int64)]
    assert (exits.reshape(-1, 6)["a"][roots] == -1).all()       # a root has no neighbour: its six exits are "none"
    assert leaf > 0 and none > 0
    if name == "triangle":
        # (the builder splits the flat root once: eight leaves under it, and no exit of this mesh leads to an inner node)
        assert len(nodes) == 9 and inner == 0
    if name in ("pear", "bunny"):
        assert inner > 0                                        # cells of unequal depth side by side
    if name == "soup":
        assert dl.exits_into_long_lists(nodes, exits) > 0              # the full count is read through such an exit


@pytest.mark.parametrize("name", MESHES + ("soup",))
def test_hit_records_hold_the_triangles_normals_and_uvs(name, tmp_path_factory):
    scene = _scene(name, tmp_path_factory)
    a = mt.arrays(scene)
    hits = dl.layout(scene, dl.HITS)
    words = np.asarray(a["triangles"]).astype(np.int64).reshape(-1, 3, 3)          # [triangle][corner] = vertex, uv, normal
    assert len(hits) == len(words) > 0
    normals, uvs = np.asarray(a["normals"]), np.asarray(a["uvs"])
    assert np.array_equal(_bits(hits["normal"]), _bits(normals[words[:, :, 2]][:, :, :3]))
    assert np.array_equal(_bits(hits["uv"]), _bits(uvs[words[:, :, 1]][:, :, :2]))
    assert not hits["spare"].any()


def test_a_scene_without_meshes_has_no_layout_to_hand_out():
    from conftest import load_config
    assert dl.layout(load_config("cubes"), dl.NODES) is None
