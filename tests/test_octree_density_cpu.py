"""Host side of the K16 density-octree build: the numpy restatement
(tests/octree_density_reference.py) on trees worked out by hand, the C ABI's argument checks, and
what ``OcTree.build_from_model`` and ``scripts/voxelize_density.py`` refuse or default to without
a GPU."""

import ctypes
import os
import sys

import numpy as np
import pytest

from tests import octree_density_reference as dref
from tests.octree_density_helpers import EXACT_TOL, ROW, blob_field, hand_cases
from tests.octree_walk_helpers import two_level_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SYMBOLS = ("ffn_octree_cell_centers", "ffn_octree_density_select", "ffn_octree_merge_level")


def run_case(case):
    depth = case["depth"]
    codes = np.asarray(case["codes"], np.int32)
    levels = np.full(len(codes), depth - 1, np.int32)
    codes, levels, data = dref.merge(codes, levels, case["data"], depth, *case["tol"])
    return dref.tree(codes, levels, data, depth)


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_hand_worked_merges(name):
    case = hand_cases()[name]
    nodes, leaves, data = run_case(case)
    assert leaves.tolist() == case["leaves"] and nodes.tolist() == case["nodes"]
    assert data.shape == (len(leaves), 4) and data.dtype == F
    if "mean" in case:
        assert np.array_equal(data[0].view(np.uint32), F(case["mean"]).view(np.uint32))


def test_the_two_level_geometry():
    """The merged octant and the two corners are the tree of ``two_level_tree``; the centres of
    its finest cells are those of the chain."""
    scale, want_nodes, want_leaves = two_level_tree()
    nodes, leaves, data = run_case(hand_cases()["two_level"])
    assert np.array_equal(nodes, want_nodes) and np.array_equal(leaves, want_leaves)
    assert np.array_equal(data[0], ROW) and data[1, 3] == 9 and data[2, 3] == 7
    centers = dref.cell_centers(56, 8, (0, 0, 0), scale, 3)
    assert np.array_equal(centers[0], F([0.25, 0.25, 0.25]))
    assert np.array_equal(centers[7], F([0.75, 0.75, 0.75]))
    assert np.array_equal(dref.cell_centers(0, 1, (0, 0, 0), scale, 3)[0], F([-0.75] * 3))
    # child index 4 [x] + 2 [y] + [z]: code 1 differs from code 0 in z
    assert np.array_equal(dref.cell_centers(1, 1, (0, 0, 0), scale, 3)[0], F([-0.75, -0.75, -0.25]))
    # depth 1: the one cell is the cube; the centre is added in f32
    assert np.array_equal(dref.cell_centers(0, 1, (0.3, -0.2, 0.1), 0.7, 1)[0], F([0.3, -0.2, 0.1]))
    moved = dref.cell_centers(0, 8, (0.3, -0.2, 0.1), 0.7, 2)
    half = F(F(0.7) * F(0.5))
    assert np.array_equal(moved[7], (F([half] * 3) + F([0.3, -0.2, 0.1])).astype(F))
    assert np.array_equal(moved[0], (F([-half] * 3) + F([0.3, -0.2, 0.1])).astype(F))


def test_the_occupancy_rule():
    tau, side = dref.tau_of(0.01), dref.side_of(1.0, 5)
    assert side == F(0.125) and tau == F(-np.log1p(-0.01)) and dref.tau_of(0.0) == 0
    edge = F(tau / side)                       # a power-of-two side: edge * side == tau exactly
    assert F(edge * side) == tau
    data = np.zeros((5, 4), F)
    data[:, 3] = [edge, np.nextafter(edge, F(np.inf)), np.nan, 0.0, 100.0]
    codes, kept = dref.select(data, 40, tau, side)
    assert codes.tolist() == [41, 44] and codes.dtype == np.int32       # strict, NaN not kept
    assert np.array_equal(kept[:, 3], data[[1, 4], 3])
    # with alpha_threshold 0 any positive density is a leaf, zero is not
    codes, _ = dref.select(data, 0, dref.tau_of(0.0), side)
    assert codes.tolist() == [0, 1, 4]
    # the activations: sigmoid(0) = 1/2, softplus above the threshold is the identity
    out = dref.activate(F([[0, 0, 0, 25], [0, 0, 0, 0]]))
    assert np.array_equal(out[0], F([0.5, 0.5, 0.5, 25])) and abs(out[1, 3] - np.log(2)) < 1e-7


def test_the_blob_field_merges_at_several_levels():
    depth = 5
    data = blob_field(depth)
    assert data.shape == (8 ** (depth - 1), 4)
    nodes, leaves, merged = dref.build(data, depth, 1.0, 0.01, (0.01, 0.01))
    _, fine, _ = dref.build(data, depth, 1.0, 0.01)
    assert len(leaves) < len(fine) and len(np.intersect1d(nodes, leaves)) == 0
    levels = np.searchsorted([dref.first_id(k) for k in range(1, depth + 1)], leaves, side="right")
    assert set(levels.tolist()) == {1, 2, 3, 4}
    assert leaves[0] == 1 and np.array_equal(merged[0], F([0.125, 0.25, 0.375, 5.0]))
    # every leaf's parent chain is in the node index
    for leaf in leaves[:: max(1, len(leaves) // 50)]:
        up = int(leaf)
        while up > 0:
            up = (up - 1) >> 3
            assert up in nodes


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_density_symbols_are_declared_and_exported():
    _lib, lib = library()
    assert set(SYMBOLS) <= set(_lib.declared_symbols())
    for name in SYMBOLS:
        assert getattr(lib, name)
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert all(k in header for k in ("K16a", "K16b", "K16c", "ffn_octree_bake"))
    lib.ffn_abi_version.restype = ctypes.c_int
    assert lib.ffn_abi_version() == _lib.ABI_VERSION == 3


def test_bad_arguments_return_nonzero_without_a_device():
    """Nothing can be launched: a scalar is out of range, a pointer is null or misaligned, in every
    call.  Pointers that would be checked later get a host buffer nobody reads."""
    _, lib = library()
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    for name in SYMBOLS:
        getattr(lib, name).restype = ctypes.c_int
    f, i64, i = ctypes.c_float, ctypes.c_int64, ctypes.c_int
    buffer = (ctypes.c_float * 64)()
    base = ctypes.addressof(buffer)
    base += (-base) % 16
    host, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def refused(name, args, why):
        status = getattr(lib, name)(*args)
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and name in text and why in text, (name, why, text)

    def centers(first=0, count=8, depth=2, out=host):
        return (i64(first), i64(count), f(0), f(0), f(0), f(1), i(depth), out, None)

    for kwargs, why in (({"out": None}, "null argument"), ({"count": 0}, "shape"),
                        ({"count": -3}, "shape"), ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
                        ({"first": -1}, "shape"), ({"first": 1}, "shape"),      # 1 + 8 > 8^1
                        ({"count": 1 << 31, "depth": 11}, "shape")):
        refused("ffn_octree_cell_centers", centers(**kwargs), why)

    def select(logits=host, first=0, count=8, depth=2, activated=host, out=host, total=host):
        return (logits, i64(first), i64(count), f(0.01), f(1.0), i(depth), host, host, host,
                activated, host, out, total, None)

    for kwargs, why in (({"logits": None}, "null argument"), ({"total": None}, "null argument"),
                        ({"logits": odd}, "aligned"), ({"activated": odd}, "aligned"),
                        ({"out": odd}, "aligned"), ({"count": 0}, "shape"),
                        ({"first": 60, "count": 8, "depth": 3}, "shape"),
                        ({"depth": 0}, "depth"), ({"depth": 12}, "depth")):
        refused("ffn_octree_density_select", select(**kwargs), why)

    def merge(codes=host, data=host, n=8, level=1, depth=2, rgb=0.0, sigma=0.0, out=host):
        return (codes, host, data, i64(n), i(level), i(depth), f(rgb), f(sigma), host, host, host,
                host, host, host, out, host, None)

    for kwargs, why in (({"codes": None}, "null argument"), ({"out": None}, "null argument"),
                        ({"data": odd}, "aligned"), ({"out": odd}, "aligned"),
                        ({"n": 0}, "shape"), ({"level": 0}, "shape"), ({"level": 2}, "shape"),
                        ({"depth": 1}, "shape"), ({"depth": 12, "level": 3}, "shape"),
                        ({"rgb": -1.0}, "tolerances"), ({"sigma": float("nan")}, "tolerances")):
        refused("ffn_octree_merge_level", merge(**kwargs), why)


class NoDevice:
    """A model whose device must not be asked for."""
    use_view = False
    training = False

    def parameters(self):
        raise AssertionError("build_from_model touched the model before checking its arguments")


def test_build_from_model_refuses_bad_arguments_before_any_device():
    import fourier_feature_nets as ffn
    build = ffn.OcTree.build_from_model
    for depth in (0, -1, 12):
        with pytest.raises(ValueError, match="depth"):
            build(NoDevice(), depth)
    for value in (1.0, -0.01, 2.0, float("nan")):
        with pytest.raises(ValueError, match="alpha_threshold"):
            build(NoDevice(), 4, alpha_threshold=value)
    for value in (-1.0, float("nan"), (0.1, -0.1), (0.1, 0.2, 0.3), ()):
        with pytest.raises(ValueError, match="merge_tolerance"):
            build(NoDevice(), 4, merge_tolerance=value)
    for kwargs in ({"center": (0, 0)}, {"view": (0, 1)}, {"batch_size": 0}):
        with pytest.raises(ValueError, match="three components"):
            build(NoDevice(), 4, **kwargs)
    for value in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            build(NoDevice(), 4, scale=value)
    with pytest.raises(AssertionError, match="touched the model"):     # all checks passed
        build(NoDevice(), 4, alpha_threshold=0.0, merge_tolerance=(0.0, 1e9))
    assert float(EXACT_TOL) == 7 / 1024


def test_program_parser_defaults():
    sys.path.insert(0, ROOT)
    from scripts import voxelize_density
    parser = voxelize_density.build_parser()
    args = parser.parse_args(["model.pt", "tree.npz"])
    assert (args.model_path, args.output_path) == ("model.pt", "tree.npz")
    assert args.voxel_depth == 8 and args.center == [0.0, 0.0, 0.0] and args.scale == 1.0
    assert args.alpha_threshold == 0.01 and args.merge_tolerance is None
    assert args.view == [0.0, 0.0, 1.0] and args.batch_size == 1 << 20 and args.device == "cuda"
    args = parser.parse_args(["m", "t", "--voxel-depth", "10", "--center", "0.25", "-0.5", "0",
                              "--scale", "1.5", "--alpha-threshold", "0.05", "--merge-tolerance",
                              "0.01", "0.5", "--view", "1", "0", "0", "--batch-size", "4096",
                              "--device", "cuda:0"])
    assert args.voxel_depth == 10 and args.center == [0.25, -0.5, 0.0] and args.scale == 1.5
    assert args.alpha_threshold == 0.05 and args.merge_tolerance == [0.01, 0.5]
    assert args.view == [1.0, 0.0, 0.0] and args.batch_size == 4096 and args.device == "cuda:0"
    with pytest.raises(SystemExit):
        parser.parse_args(["m"])
    with pytest.raises(SystemExit):
        parser.parse_args(["m", "t", "--merge-tolerance", "0.1"])
