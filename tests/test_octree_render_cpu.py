"""Host side of the K14 first-hit render: the float64 restatement (tests/octree_render_reference.py)
against the paths the reference itself recorded (tests/golden/octree_walk.npz) and against answers
worked out by hand, the C ABI's argument checks, and what ``OcTree.render`` / ``render_image`` and
``scripts/render_octree.py`` refuse or default to without a GPU.

First-leaf agreement with the recorded paths follows from the full-path agreement of
tests/test_octree_walk_cpu.py; the rays left out are its GRAZING rays (restatement margin below the
fixture's own threshold) and those whose first leaf lies beyond the recorded length, together at
most its 10 %."""

import ctypes
import os
import sys

import numpy as np
import pytest

from tests import octree_render_reference as rref
from tests import octree_walk_reference as wref
from tests.octree_walk_helpers import two_level_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
TREES = ["shell", "planes", "nodata"]


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in ("octree.npz", "octree_walk.npz"):
        with np.load(os.path.join(HERE, "golden", name)) as g:
            out[name] = {k: g[k] for k in g.files}
    return out


@pytest.mark.parametrize("name", TREES)
def test_first_leaf_equals_the_reference_paths(golden, name):
    tree = {k: golden["octree.npz"][name + "/" + k] for k in ("scale", "node_index", "leaf_index")}
    g = golden["octree_walk.npz"]
    starts, directions = g[name + "/starts"], g[name + "/directions"]
    recorded = g[name + "/leaves_64"]
    w = wref.walk(tree["scale"], tree["node_index"], tree["leaf_index"], starts, directions)
    # along the whole chord: no t_min
    want = rref.first_hit(w, tree["scale"], tree["leaf_index"], starts, directions, -np.inf)
    stop = want["crossing"] - w["offsets"][:-1]              # which stop of its ray
    beyond = (want["crossing"] >= 0) & (stop >= recorded.shape[1] - 1)
    grazing = w["margin"] < float(g["grazing"])
    ok = ~grazing & ~beyond
    print("%s: %d grazing, %d beyond the recorded length, of %d" %
          (name, grazing.sum(), beyond.sum(), len(ok)))
    assert 1.0 - ok.mean() <= 0.10
    has = (recorded >= 0).any(1)
    first = np.where(has, recorded[np.arange(len(recorded)), (recorded >= 0).argmax(1)], -1)
    assert np.array_equal(want["leaf"][ok], first[ok])
    assert (want["leaf"][ok] >= 0).sum() >= 100
    assert not want["clamped"].any() and (want["face"][want["leaf"] >= 0] < 6).all()


def test_known_answers_on_a_hand_built_tree():
    scale, nodes, leaves = two_level_tree()
    starts = np.float32([[-2, -0.5, -0.5], [0.25, 0.3, -3], [0.2, 0.3, 0.1]])
    dirs = np.float32([[2, 0, 0], [0, 0, 1], [0, 0, -0.5]])
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    hit = rref.first_hit(w, scale, leaves, starts, dirs, 0.0)
    assert list(hit["leaf"]) == [0, 1, 1]
    assert np.allclose(hit["t"], [0.5, 3.0, 0.0]) and hit["t"][2] == 0.0
    assert list(hit["face"]) == [0, 4, 6]
    assert list(hit["clamped"]) == [False, False, True]
    # the third ray leaves leaf 1 at t = 0.2: nothing ends after 0.5
    late = rref.first_hit(w, scale, leaves, starts, dirs, 0.5)
    assert late["leaf"][2] == -1 and late["t"][2] == 0 and late["face"][2] == -1
    assert late["crossing"][2] == -1 and np.isinf(late["edge_gap"][2])
    # ray 0 enters leaf 0 at t = 0.5 exactly: not before t_min, so a face, and max() is t_min
    assert late["leaf"][0] == 0 and late["face"][0] == 0 and late["t"][0] == 0.5
    # towards -x from beyond the cube: the +x face of leaf 2
    w2 = wref.walk(scale, nodes, leaves, np.float32([[3, 0.75, 0.8]]), np.float32([[-1, 0, 0]]))
    back = rref.first_hit(w2, scale, leaves, np.float32([[3, 0.75, 0.8]]),
                          np.float32([[-1, 0, 0]]), 0.0)
    assert back["leaf"][0] == 2 and back["face"][0] == 1 and np.isclose(back["t"][0], 2.0)
    # the main diagonal enters leaf 0 through a corner of the cube: no gap between the axes
    w3 = wref.walk(scale, nodes, leaves, np.float32([[-2, -2, -2]]), np.float32([[1, 1, 1]]))
    corner = rref.first_hit(w3, scale, leaves, np.float32([[-2, -2, -2]]),
                            np.float32([[1, 1, 1]]), 0.0)
    assert corner["leaf"][0] == 0 and corner["edge_gap"][0] == 0.0
    assert hit["edge_gap"][0] == np.inf        # two zero components: one axis only


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_render_symbols_are_declared_and_exported():
    _lib, lib = library()
    assert {"ffn_octree_first_hit", "ffn_octree_render"} <= set(_lib.declared_symbols())
    assert lib.ffn_octree_first_hit and lib.ffn_octree_render
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "octree.py:418-501" in header and "voxelize_model.py:90-110" in header
    # the table of "faces" shading: declared in the header, seven factors, pairs, 1 for face 6
    table = (ctypes.c_float * 7)()
    lib.ffn_octree_face_shade.restype = None
    lib.ffn_octree_face_shade(table)
    k = list(table)
    assert "FFN_OCTREE_FACE_SHADE" in header
    assert k[0] == k[1] and k[2] == k[3] and k[4] == k[5] and k[6] == 1.0
    assert all(0.0 < v <= 1.0 for v in k) and len({k[0], k[2], k[4]}) == 3


def test_bad_arguments_return_nonzero_without_a_device():
    """Every pointer is null in every call, so nothing can be launched; which check refused is
    read from the library's error string."""
    _, lib = library()
    lib.ffn_octree_first_hit.restype = ctypes.c_int
    lib.ffn_octree_render.restype = ctypes.c_int
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    f, i64 = ctypes.c_float, ctypes.c_int64

    def first_hit(n=4, depth=3, num_leaves=1, t_min=0.0):
        status = lib.ffn_octree_first_hit(None, None, i64(n), f(1.0), depth, None, i64(0), None,
                                          i64(num_leaves), f(t_min), None, None, None, None)
        return status, lib.ffn_last_error_string().decode()

    def render(n=4, depth=3, t_min=0.0, channels=3, shading=0):
        status = lib.ffn_octree_render(None, None, i64(n), f(1.0), depth, None, i64(0), None,
                                       i64(1), f(t_min), None, channels, f(0), f(0), f(0),
                                       shading, None, None, None, None, None, None, None)
        return status, lib.ffn_last_error_string().decode()

    for call, who in ((first_hit, "ffn_octree_first_hit"), (render, "ffn_octree_render")):
        for kwargs, why in (({}, "null argument"), ({"n": 0}, "shape"), ({"depth": 30}, "shape"),
                            ({"depth": 0}, "shape"), ({"t_min": float("nan")}, "t_min")):
            status, text = call(**kwargs)
            assert status != 0 and who in text and why in text, (kwargs, text)
    status, text = first_hit(num_leaves=0)
    assert status != 0 and "shape" in text
    for kwargs, why in (({"channels": 2}, "channels"), ({"channels": 0}, "channels"),
                        ({"shading": 2}, "shading"), ({"shading": -1}, "shading")):
        status, text = render(**kwargs)
        assert status != 0 and why in text, (kwargs, text)


def test_render_refuses_trees_without_colours_and_images_without_a_centre():
    import fourier_feature_nets as ffn
    from fourier_feature_nets.octree import Hit
    assert Hit._fields == ("leaves", "t", "faces")
    scale, nodes, leaves = two_level_tree()
    rays = np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    bare = ffn.OcTree(float(scale), nodes, leaves)
    with pytest.raises(ValueError, match="leaf_data"):
        bare.render(*rays)
    two = ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 2), np.float32))
    with pytest.raises(ValueError, match="leaf_data"):
        two.render(*rays)
    full = ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="shading"):
        full.render(*rays, shading="phong")
    assert full.center is None
    with pytest.raises(ValueError, match="cent"):
        full.render_image(None, 0)
    with pytest.raises(NotImplementedError, match="intersect"):
        full.intersect(rays[0], rays[1], 4)
    with pytest.raises(NotImplementedError):
        ffn.OcTree.build_from_mesh("mesh.ply", 4, 1)
    # the device copy of leaf_data is dropped when the tree's state changes
    full._cache[("leaf_data_f32", "cuda")] = "stale"
    full.load_state(full.state_dict)
    assert not full._cache


def test_render_octree_parser_defaults():
    sys.path.insert(0, ROOT)
    from scripts import render_octree
    parser = render_octree.build_parser()
    args = parser.parse_args(["tree.npz", "data.npz", "out"])
    assert (args.tree_path, args.data_path, args.output_dir) == ("tree.npz", "data.npz", "out")
    assert args.split == "val" and args.resolution is None and args.num_cameras == 10
    assert args.center == [0.0, 0.0, 0.0] and args.background == [0.0, 0.0, 0.0]
    assert args.shading == "flat" and args.device == "cuda"
    args = parser.parse_args(["t", "d", "o", "--center", "0.25", "-0.5", "-0.0001", "--shading",
                              "faces", "--background", "1", "1", "1", "--split", "train",
                              "--resolution", "32", "--num-cameras", "2", "--device", "cuda:0"])
    assert args.center == [0.25, -0.5, -0.0001] and args.shading == "faces"
    assert args.background == [1.0, 1.0, 1.0] and args.split == "train"
    assert args.resolution == 32 and args.num_cameras == 2
    with pytest.raises(SystemExit):
        parser.parse_args(["t", "d", "o", "--shading", "smooth"])
