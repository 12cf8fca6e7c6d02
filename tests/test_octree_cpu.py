"""Host side of the octree: the numpy restatement (tests/octree_reference.py) against trees the
reference itself built (tests/golden/octree.npz from tests/golden/make_octree.py), the
voxelize_model.py parser against the reference's, the host-only load / state_dict / prune path of
``OcTree`` and the K12 ABI symbols."""

import ctypes
import json
import os

import numpy as np
import pytest

from tests import octree_reference as oref

HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def golden():
    with np.load(os.path.join(HERE, "golden", "octree.npz")) as g:
        return {k: g[k] for k in g.files}


def cloud_names(g):
    return [str(n) for n in g["names"]]


def mean_bound(data, point_leaf, leaf_index, counts):
    """(n + 1) * 2^-24 * mean|x| per leaf and component: first-order bound of an f32 sum of n
    terms in any order, plus the division."""
    keep = point_leaf >= 0
    slot = np.searchsorted(leaf_index, point_leaf[keep])
    mag = np.zeros((len(leaf_index), data.shape[1]), np.float64)
    np.add.at(mag, slot, np.abs(np.asarray(data, np.float64)[keep]))
    return (counts[:, None] + 1) * 2.0 ** -24 * (mag / counts[:, None])


def test_fixture_covers_the_cases(golden):
    names = cloud_names(golden)
    assert set(names) == {"shell", "planes", "tiny", "depth1", "nodata"}
    assert len(np.unique(golden["shell/leaf_depths"])) >= 2
    assert len(golden["tiny/node_index"]) == 0 and list(golden["tiny/leaf_index"]) == [0]
    assert int(golden["depth1/depth"]) == 1 and "nodata/data" not in golden


@pytest.mark.parametrize("name", ["shell", "planes", "tiny", "depth1", "nodata"])
def test_restatement_reproduces_the_reference_trees(golden, name):
    g = {k.split("/", 1)[1]: v for k, v in golden.items() if k.startswith(name + "/")}
    mine = oref.build(g["positions"], int(g["depth"]), int(g["min_leaf_size"]), g.get("data"))
    assert np.array_equal(mine["node_index"], g["node_index"])
    assert np.array_equal(mine["leaf_index"], g["leaf_index"])
    assert np.float32(mine["scale"]).tobytes() == np.float32(g["scale"]).tobytes()
    if "data" in g:
        # the reference's own f32 means pass the bound the GPU means are held to
        bound = mean_bound(g["data"], mine["point_leaf"], mine["leaf_index"], mine["leaf_count"])
        assert g["leaf_data"].dtype == np.float32
        assert (np.abs(g["leaf_data"].astype(np.float64) - mine["leaf_data"]) <= bound).all()
    if "leaf_centers" in g:
        centers, depths = oref.leaf_geometry(g["scale"], g["leaf_index"])
        assert centers.tobytes() == g["leaf_centers"].tobytes()
        assert np.array_equal(depths, g["leaf_depths"])
    if "query" in g:
        assert len(g["query"]) >= 3000
        answers = oref.query(g["scale"], g["node_index"], g["leaf_index"], g["query"])
        assert np.array_equal(answers, g["query_result"])
        assert (answers >= 0).any() and (answers < 0).any()


def test_voxelize_parser_equals_the_reference():
    from scripts import _cli
    with open(os.path.join(HERE, "golden", "cli_defaults_voxelize.json")) as f:
        ref = json.load(f)["voxelize_model"]
    from tests.golden.make_octree import CLI_ARGV
    mine = vars(_cli.build_parser("t", _cli.VOXELIZE).parse_args(CLI_ARGV))
    assert mine == ref
    assert isinstance(_cli.build_parser("t", _cli.VOXELIZE).parse_args(
        CLI_ARGV + ["--num-cameras", "7"]).num_cameras, float)


@pytest.mark.parametrize("name", ["shell", "planes", "tiny", "nodata"])
def test_load_then_state_dict_returns_the_same_arrays(golden, name, tmp_path):
    import fourier_feature_nets as ffn
    from fourier_feature_nets.octree import OcTree
    assert OcTree is ffn.OcTree
    state = {"node_index": golden[name + "/node_index"], "leaf_index": golden[name + "/leaf_index"],
             "scale": float(golden[name + "/scale"])}        # the reference stores a Python float
    if name + "/leaf_data" in golden:
        state["leaf_data"] = golden[name + "/leaf_data"]
    tree = ffn.OcTree.load(state)
    back = tree.state_dict
    assert sorted(back) == sorted(state)
    for key in ("node_index", "leaf_index"):
        assert back[key].dtype == np.int64 and np.array_equal(back[key], state[key])
    assert back["scale"].dtype == np.float32
    assert back["scale"].tobytes() == golden[name + "/scale"].tobytes()
    if "leaf_data" in state:
        assert back["leaf_data"].tobytes() == state["leaf_data"].tobytes()
    assert len(tree) == len(state["node_index"]) + len(state["leaf_index"])
    assert tree.num_leaves == len(state["leaf_index"]) and tree.scale == state["scale"]
    assert tree.depth == (1 if name == "tiny" else int(golden[name + "/leaf_depths"].max()) + 1)
    # through a file, and through load_state
    path = str(tmp_path / "tree.npz")
    tree.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == sorted(state)
        assert f["node_index"].dtype == np.int64 and f["leaf_index"].dtype == np.int64
    again = ffn.OcTree.load(path)
    assert np.array_equal(again.state_dict["leaf_index"], state["leaf_index"])
    other = ffn.OcTree(1.0, set(), {0})
    other.load_state(state)
    assert np.array_equal(other.state_dict["node_index"], state["node_index"])
    assert ffn.OcTree.load(str(tmp_path / "missing.npz")) is None


@pytest.mark.parametrize("name", ["shell", "planes", "nodata"])
def test_prune_equals_the_reference(golden, name):
    import fourier_feature_nets as ffn
    state = {k: golden[name + "/" + k] for k in ("node_index", "leaf_index", "scale")}
    if name + "/leaf_data" in golden:
        state["leaf_data"] = golden[name + "/leaf_data"]
    pruned = ffn.OcTree.load(state).prune()
    assert np.array_equal(pruned.state_dict["node_index"], golden[name + "/pruned_node_index"])
    assert np.array_equal(pruned.state_dict["leaf_index"], golden[name + "/pruned_leaf_index"])
    if "leaf_data" in state:
        assert pruned.leaf_data().tobytes() == golden[name + "/pruned_leaf_data"].tobytes()
    else:
        assert pruned.leaf_data() is None


def test_parts_outside_this_path_say_so():
    import fourier_feature_nets as ffn
    tree = ffn.OcTree(1.0, {0}, {1, 2})
    with pytest.raises(NotImplementedError, match="intersect"):
        tree.intersect(np.zeros((1, 3)), np.ones((1, 3)), 4)
    with pytest.raises(NotImplementedError, match="build_from_mesh"):
        ffn.OcTree.build_from_mesh("mesh.obj", 4, 2)
    with pytest.raises(ValueError, match="leaf"):
        ffn.OcTree(1.0, {0}, set())


def test_octree_symbols_are_declared_and_exported():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    names = [n for n in _lib.declared_symbols() if n.startswith("ffn_octree_")]
    assert set(names) >= {"ffn_octree_surface_points", "ffn_octree_path_codes",
                          "ffn_octree_structure", "ffn_octree_interior_nodes",
                          "ffn_octree_leaf_means", "ffn_octree_query",
                          "ffn_octree_leaf_geometry", "ffn_octree_scan_tiles",
                          "ffn_octree_max_depth"}
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in names:
        assert hasattr(lib, name), name
    lib.ffn_octree_max_depth.restype = ctypes.c_int
    assert lib.ffn_octree_max_depth() >= 10
    # argument checks refuse before any launch: no GPU is touched
    lib.ffn_octree_query.restype = ctypes.c_int
    assert lib.ffn_octree_query(None, ctypes.c_int64(4), ctypes.c_float(1.0), None,
                                ctypes.c_int64(0), None, ctypes.c_int64(1), None, None) != 0
