"""Host side of K18 (spherical-harmonic leaves): the basis and the view set of ``bake_sh``, what an
``OcTree`` does with ``sh_degree`` without a GPU (state, ``prune``, refusals), the C ABI's argument
checks, the program's new flags, and the inputs of tests/test_octree_sh_gpu.py (the share of rays
its cases leave out, in the float64 walk)."""

import ctypes
import os
import sys

import numpy as np
import pytest

from tests import octree_sh_reference as shref
from tests.octree_render_helpers import LEFT_OUT_CAP
from tests.octree_sh_helpers import DEGREES, SIZES, TREES, case, prefix, sh_leaf_data
from tests.octree_walk_helpers import two_level_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def sh_tree(degree, dtype=np.float32):
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    data = sh_leaf_data(scale, leaves, degree).astype(dtype)
    return ffn.OcTree(float(scale), nodes, leaves, data, sh_degree=degree), data


def test_basis_closed_forms_and_quadrature():
    from fourier_feature_nets_amd.octree import sh_basis, sh_view_directions
    c0, c1 = 0.28209479177387814, 0.4886025119029199
    c2, c3, c4 = 1.0925484305920792, 0.31539156525252005, 0.5462742152960396
    root = np.sqrt(0.5)
    want = {(1, 0, 0): [c0, 0, 0, -c1, 0, 0, -c3, 0, c4],
            (0, 1, 0): [c0, -c1, 0, 0, 0, 0, -c3, 0, -c4],
            (0, 0, 1): [c0, 0, c1, 0, 0, 0, 2 * c3, 0, 0],
            (0, 0, -1): [c0, 0, -c1, 0, 0, 0, 2 * c3, 0, 0],
            (root, root, 0): [c0, -c1 * root, 0, -c1 * root, c2 / 2, 0, -c3, 0, 0],
            (0, root, -root): [c0, -c1 * root, -c1 * root, 0, 0, c2 / 2, c3 / 2, 0, -c4 / 2],
            (-root, 0, root): [c0, 0, c1 * root, c1 * root, 0, 0, c3 / 2, c2 / 2, c4 / 2]}
    for u, row in want.items():
        assert np.allclose(sh_basis(np.array(u), 2)[0], row, rtol=0, atol=1e-15), u
        assert np.allclose(sh_basis(np.array([u]), 1)[0], row[:4], rtol=0, atol=1e-15), u
        # the restatement of the tests is a second writing of the same table
        assert np.allclose(shref.basis(np.float32([u]) * 3, 2)[0], row, rtol=0, atol=1e-7), u
    assert sh_basis(np.zeros((5, 3)), 1).shape == (5, 4) and sh_basis(np.zeros(3), 2).shape == (1, 9)
    views = sh_view_directions(4096)
    assert views.shape == (4096, 3) and views.dtype == np.float64
    assert np.allclose(np.linalg.norm(views, axis=1), 1.0, rtol=0, atol=1e-15)
    assert np.array_equal(views, sh_view_directions(4096))
    gram = 4 * np.pi / 4096 * sh_basis(views, 2).T @ sh_basis(views, 2)
    worst = np.abs(gram - np.eye(9)).max()
    print("Fibonacci quadrature, 4096 points: |(4 pi / V) Y^T Y - I| <= %.3g" % worst)
    # measured for this point set: 2.07e-5.  The bound is the order of a lattice rule on the
    # sphere, 1 / V: the z midpoints integrate polynomials in z far better, the golden-angle
    # azimuths leave O(1 / V)
    assert worst <= 1.0 / 4096


@pytest.mark.parametrize("degree", DEGREES)
def test_projection_is_a_left_inverse(degree):
    from fourier_feature_nets_amd.octree import sh_basis, sh_view_directions
    bases = (degree + 1) ** 2
    for num_views in (2 * bases, 64):
        y = sh_basis(sh_view_directions(num_views), degree)
        assert y.shape == (num_views, bases)
        assert np.abs(np.linalg.pinv(y) @ y - np.eye(bases)).max() <= 1e-10
        print("degree %d, %d views: cond(Y) = %.4f" % (degree, num_views, np.linalg.cond(y)))


@pytest.mark.parametrize("degree", DEGREES)
def test_state_round_trip(degree, tmp_path):
    import fourier_feature_nets as ffn
    tree, data = sh_tree(degree)
    assert tree.sh_degree == degree
    state = tree.state_dict
    assert state["sh_degree"].dtype == np.int32 and state["sh_degree"].shape == ()
    assert int(state["sh_degree"]) == degree
    again = ffn.OcTree.load(state)
    assert again.sh_degree == degree and np.array_equal(again.leaf_data(), data)
    path = str(tmp_path / "sh.npz")
    tree.save(path)
    with np.load(path) as f:
        assert set(f.files) == {"node_index", "leaf_index", "scale", "leaf_data", "sh_degree"}
    loaded = ffn.OcTree.load(path)
    assert loaded.sh_degree == degree and np.array_equal(loaded.leaf_data(), data)
    assert np.array_equal(loaded.state_dict["leaf_index"], state["leaf_index"])
    # without the key: a plain tree, whatever the channel count -- nothing is inferred
    del state["sh_degree"]
    plain = ffn.OcTree.load(state)
    assert plain.sh_degree is None and "sh_degree" not in plain.state_dict
    scale, nodes, leaves = two_level_tree()
    assert ffn.OcTree(float(scale), nodes, leaves, data).sh_degree is None
    assert ffn.OcTree(float(scale), nodes, leaves).sh_degree is None
    # a degree that does not fit the channels
    state["sh_degree"] = np.int32(3 - degree)
    with pytest.raises(ValueError, match="sh_degree"):
        ffn.OcTree.load(state)
    state["sh_degree"] = np.int32(3)
    with pytest.raises(ValueError, match="sh_degree"):
        ffn.OcTree.load(state)
    state["sh_degree"] = np.int32(degree)
    state["leaf_data"] = data[:, :4]
    with pytest.raises(ValueError, match="sh_degree"):
        ffn.OcTree.load(state)
    del state["leaf_data"]
    with pytest.raises(ValueError, match="sh_degree"):
        ffn.OcTree.load(state)


def test_prune_keeps_the_degree():
    tree, data = sh_tree(2, np.float64)
    pruned = tree.prune()
    assert pruned.sh_degree == 2 and pruned.leaf_data().shape == (2, 28)
    # leaves 1 and 2 (ids 65 and 72) merge into node 8: the mean of their coefficient vectors
    assert np.array_equal(pruned.leaf_data()[0], data[0])
    assert np.allclose(pruned.leaf_data()[1], data[1:].mean(0), rtol=0, atol=1e-15)
    assert tree.sh_degree == 2 and tree.leaf_data().shape == (3, 28)
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    assert ffn.OcTree(float(scale), nodes, leaves).prune().sh_degree is None


def test_refusals_before_any_device():
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd.octree import sh_basis
    tree, data = sh_tree(2)
    rays = np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    for degree in (0, 3, -1, 1.5, True):
        with pytest.raises(ValueError, match="degree"):
            tree.bake_sh(None, degree=degree, center=(0, 0, 0))
        with pytest.raises(ValueError, match="degree"):
            sh_basis(np.zeros((1, 3)), degree)
        with pytest.raises(ValueError, match="degree"):
            ffn.OcTree(1.0, [0], [1], data[:1], sh_degree=degree)
    for degree, views in ((1, 7), (2, 17), (2, 0)):
        with pytest.raises(ValueError, match="num_views"):
            tree.bake_sh(None, degree=degree, num_views=views, center=(0, 0, 0))
    # a loaded tree does not know its centre: the error of bake
    assert tree.center is None
    with pytest.raises(ValueError, match="cent") as sh_error:
        tree.bake_sh(None)
    with pytest.raises(ValueError, match="cent") as bake_error:
        tree.bake(None)
    assert str(sh_error.value) == str(bake_error.value)
    for who in (lambda: ffn.OctreeField(tree, center=(0, 0, 0)),
                lambda: ffn.fit_octree(tree, None, center=(0, 0, 0))):
        with pytest.raises(ValueError, match="fitting SH leaves is not built"):
            who()
    # render_volume validates an SH tree as _check_volume does: before any device
    for value in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="min_transmittance"):
            tree.render_volume(*rays, min_transmittance=value)
        with pytest.raises(ValueError, match="min_transmittance"):
            tree.render_image(None, 0, center=(0, 0, 0), mode="volume", min_transmittance=value)
    with pytest.raises(ValueError, match="cent"):
        tree.render_image(None, 0, mode="volume")
    tree._leaf_data = data[:, :13]                      # tampered with after construction
    with pytest.raises(ValueError, match="sh_degree"):
        tree.render_volume(*rays)


def test_device_layout():
    from fourier_feature_nets_amd import ops
    for degree, stride in ((1, 16), (2, 28)):
        _, data = sh_tree(degree, np.float64)
        rows = ops.octree_sh_device_layout(data, degree)
        assert rows.shape == (3, stride) and rows.dtype == np.float32 and rows.flags.c_contiguous
        channels = data.shape[1]
        assert np.array_equal(rows[:, 0], data[:, -1].astype(np.float32))
        assert np.array_equal(rows[:, 1:channels], data[:, :-1].astype(np.float32))
        assert (rows[:, channels:] == 0).all()
        with pytest.raises(ValueError, match="leaf_data"):
            ops.octree_sh_device_layout(data[:, :-1], degree)
    with pytest.raises(ValueError, match="degree"):
        ops.octree_sh_device_layout(data, 3)


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_sh_symbols_and_bad_arguments_without_a_device():
    _lib, lib = library()
    names = {"ffn_octree_render_volume_sh", "ffn_octree_sh_accumulate"}
    assert names <= set(_lib.declared_symbols())
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "K18a" in header and "K18b" in header and "row_stride" in header
    lib.ffn_octree_render_volume_sh.restype = ctypes.c_int
    lib.ffn_octree_sh_accumulate.restype = ctypes.c_int
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    f, i64 = ctypes.c_float, ctypes.c_int64
    host = (ctypes.c_float * 64)()

    def render(n=4, depth=3, t_min=0.0, channels=28, min_t=0.0, own=None, degree=2, stride=28):
        status = lib.ffn_octree_render_volume_sh(None, None, i64(n), f(1.0), depth, None, i64(0),
                                                 None, i64(1), f(t_min), own, channels, f(0), f(0),
                                                 f(0), f(min_t), own, own, own, degree, stride,
                                                 None)
        return status, lib.ffn_last_error_string().decode()

    for kwargs, why in (({}, "null argument"), ({"own": host}, "null argument"),
                        ({"n": 0, "own": host}, "shape"), ({"depth": 30, "own": host}, "shape"),
                        ({"degree": 0}, "degree"), ({"degree": 3}, "degree"),
                        ({"channels": 13}, "channels"), ({"degree": 1}, "channels"),
                        ({"stride": 24}, "row_stride"), ({"stride": 30}, "row_stride"),
                        ({"degree": 1, "channels": 13, "stride": 13}, "row_stride"),
                        ({"stride": 68}, "row_stride"),
                        ({"t_min": float("nan")}, "t_min"), ({"min_t": 1.0}, "min_transmittance"),
                        ({"min_t": float("nan")}, "min_transmittance"),
                        ({"degree": 1, "channels": 13, "stride": 16}, "null argument")):
        status, text = render(**kwargs)
        assert status != 0 and "ffn_octree_render_volume_sh" in text and why in text, (kwargs, text)
    for args, why in (((None, i64(4), 2, host, f(1), host, None), "null argument"),
                      ((host, i64(4), 2, None, f(1), host, None), "null argument"),
                      ((host, i64(4), 2, host, f(1), None, None), "null argument"),
                      ((host, i64(0), 2, host, f(1), host, None), "shape"),
                      ((host, i64(1 << 31), 1, host, f(1), host, None), "shape"),
                      ((host, i64(4), 0, host, f(1), host, None), "degree"),
                      ((host, i64(4), 3, host, f(1), host, None), "degree")):
        status = lib.ffn_octree_sh_accumulate(*args)
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and "ffn_octree_sh_accumulate" in text and why in text, text


def test_bake_program_flags():
    sys.path.insert(0, ROOT)
    from scripts import bake_octree
    parser = bake_octree.build_parser()
    args = parser.parse_args(["tree.npz", "model.pt", "out.npz"])
    assert args.sh_degree is None and args.num_views == 64
    args = parser.parse_args(["t", "m", "o", "--sh-degree", "1", "--num-views", "12"])
    assert args.sh_degree == 1 and args.num_views == 12
    with pytest.raises(SystemExit):
        parser.parse_args(["t", "m", "o", "--sh-degree", "3"])


@pytest.mark.parametrize("name", sorted(TREES))
def test_the_gpu_cases_leave_out_few_rays(name):
    """What tests/test_octree_sh_gpu.py relies on, decided in the float64 walk alone: every prefix
    of the ray set keeps at least 98 % of its rays, hits and misses are both there, and the rays
    end across the range of transmittance."""
    scale, nodes, leaves, starts, directions, w, ok = case(name)
    depths = {"eight": 2, "mixed4": 4}
    import fourier_feature_nets as ffn
    tree = ffn.OcTree(float(scale), nodes, leaves)
    assert tree.depth == depths[name]
    if name == "eight":
        assert tree.num_leaves == 8
    for n in SIZES:
        assert 1.0 - ok[:n].mean() <= LEFT_OUT_CAP, (n, 1.0 - ok[:n].mean())
    assert w["hit"].sum() > 500 and (~w["hit"]).sum() > 20
    for degree in DEGREES:
        data = sh_leaf_data(scale, leaves, degree)
        assert np.abs(data[:, :-1]).max() <= 4.0 and (data[:, -1] >= 0).all()
        v = shref.composite(w, scale, starts, directions, data, degree, 0.0, (0.25, 0.5, 0.125))
        took = v["count"] > 0
        mid = took & (v["trans"] > 0.05) & (v["trans"] < 0.95)
        print("%s degree %d: %d of 1000 rays take a leaf (at most %d), %d end with 0.05 < T < 0.95;"
              " colour budget %.3g .. %.3g, of which the colour's own term at most %.3g"
              % (name, degree, took.sum(), v["count"].max(), mid.sum(), v["budget_c"].min(),
                 v["budget_c"].max(), v["own"].max()))
        assert mid.sum() >= 0.3 * took.sum()
        # the restatement on a prefix is the restatement of the prefix
        small = shref.composite(prefix(w, 65), scale, starts[:65], directions[:65], data, degree,
                                0.0, (0.25, 0.5, 0.125))
        assert np.array_equal(small["color"], v["color"][:65])
        assert np.array_equal(small["budget_c"], v["budget_c"][:65])
    # opposite directions see different colours at degree 1, the same band-0 and band-2 terms
    y = shref.basis(np.float32([[1, 2, 3], [-1, -2, -3]]), 2)
    assert np.allclose(y[0, 1:4], -y[1, 1:4]) and np.allclose(y[0, 4:], y[1, 4:])
