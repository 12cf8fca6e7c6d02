"""Host side of K24, colouring leaves from the cameras that can see them: the numpy restatement
(tests/visible_reference.py) on scenes whose answer is known by hand and on the seeded scenes the
GPU tests use, ``cameras.projection_matrices(origin=...)`` / ``eye_positions`` against float64, what
the C ABI refuses without a GPU, the programs' arguments, and the routing of
``build_from_silhouettes(color=...)``."""

import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from tests import visible_reference as vref
from tests.carve_helpers import AXIS_EYES, OBLIQUE_EYES, Scene, rig, turned_away
from tests.octree_lattice_helpers import grid_tree
from tests.visible_helpers import (camera_arrays, constant_images, densities, depth_of, grid_scene,
                                   mixed_scene, two_in_a_row)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SYMBOL = "ffn_octree_visible_votes"


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


# ------------------------------------------------------------------------------- hand cases
def test_a_root_only_tree_is_seen_by_every_camera_in_front():
    cameras = rig(AXIS_EYES[:3], 4.0, 8, 8)
    cameras[1] = turned_away(cameras[1])
    proj, eyes = camera_arrays(cameras, (0, 0, 0))
    images = constant_images([[10, 20, 30], [1, 1, 1], [200, 100, 50]], 8, 8)
    out = vref.visible(1.0, np.zeros(0, np.int64), np.zeros(1, np.int64), [50.0], images, proj, eyes,
                       128, 0.3)
    assert out["votes"].tolist() == [[210, 120, 80, 2]]
    assert out["candidate"].tolist() == [[True, False, True]] and not out["undecided"].any()
    # the colour: one f32 division of two exact integers per channel
    want = (F([210, 120, 80]) / F(255 * 2)).astype(F)
    assert np.array_equal(bits(vref.colors(out["votes"], np.zeros((1, 3), F))), bits(want[None]))


@pytest.mark.parametrize("front,occludes", [(50.0, True), (0.0, False), (-3.0, False),
                                            (float("nan"), False)])
def test_two_leaves_in_a_row(front, occludes):
    """An opaque leaf in front hides the one behind it; a transparent one, one of negative density
    and one of NaN density hide nothing (``sigma = fmaxf(density, 0)``).  The front leaf sees the
    camera whatever it holds."""
    scale, nodes, ids, density, cameras = two_in_a_row(front)
    proj, eyes = camera_arrays(cameras, (0, 0, 0))
    images = constant_images([[7, 8, 9]], 16, 16)
    out = vref.visible(scale, nodes, ids, density, images, proj, eyes, 1, 0.3)
    assert out["candidate"].all() and not out["undecided"].any()
    assert out["votes"][0].tolist() == [7, 8, 9, 1]
    assert out["votes"][1].tolist() == ([0, 0, 0, 0] if occludes else [7, 8, 9, 1])
    # the chord in front is (2/9) |d| = 1.012: density 1 leaves T = 0.363, above 0.3 and below 0.5
    density[0] = 1.0
    for tau, seen in ((0.3, True), (0.5, False), (0.0, True)):
        out = vref.visible(scale, nodes, ids, density, images, proj, eyes, 1, tau)
        assert bool(out["visible"][1, 0]) == seen and not out["undecided"].any()
    # and with tau = 0 only a cell opaque enough for f32's a to be exactly 1 occludes
    density[0] = 50.0
    assert not vref.visible(scale, nodes, ids, density, images, proj, eyes, 1, 0.0)["visible"][1, 0]


def test_an_eye_inside_the_cube_and_inside_the_target_leaf():
    """The eye at (-0.9, -0.9, -0.9) lies inside leaf 0, looking at the origin with a wide lens.  Its
    own leaf's centre lies ahead on the optical axis: visible however dense the leaf is (the walk
    meets the target first).  The +x neighbour's centre lies behind 0.97 of opaque leaf 0."""
    scale, nodes, ids, density, _ = two_in_a_row(50.0)
    cameras = rig([(-1, -1, -1)], 0.9 * np.sqrt(3.0), 32, 32, fov_deg=100.0)
    proj, eyes = camera_arrays(cameras, (0, 0, 0))
    images = constant_images([[40, 50, 60]], 32, 32)
    out = vref.visible(scale, nodes, ids, density, images, proj, eyes, 255, 0.3)
    assert out["candidate"].all() and not out["undecided"].any()
    assert out["votes"].tolist() == [[40, 50, 60, 1], [0, 0, 0, 0]]
    density[0] = 0.0
    out = vref.visible(scale, nodes, ids, density, images, proj, eyes, 255, 0.3)
    assert out["votes"].tolist() == [[40, 50, 60, 1], [40, 50, 60, 1]]


def test_a_camera_turned_away_and_a_background_pixel_do_not_vote():
    scale, nodes, ids, density, cameras = two_in_a_row(0.0)
    proj, eyes = camera_arrays([turned_away(cameras[0])], (0, 0, 0))
    images = constant_images([[7, 8, 9]], 16, 16)
    out = vref.visible(scale, nodes, ids, density, images, proj, eyes, 1, 0.3)
    assert not out["candidate"].any() and not out["votes"].any()
    proj, eyes = camera_arrays(cameras, (0, 0, 0))
    out = vref.visible(scale, nodes, ids, density, constant_images([[7, 8, 9]], 16, 16, alpha=100),
                       proj, eyes, 101, 0.3)
    assert not out["candidate"].any() and not out["votes"].any()
    out = vref.visible(scale, nodes, ids, density, constant_images([[7, 8, 9]], 16, 16, alpha=100),
                       proj, eyes, 100, 0.3)
    assert out["votes"][:, 3].tolist() == [1, 1]


# ------------------------------------------------------------------------------- seeded scenes
@pytest.mark.parametrize("name,eyes,distance", [("mixed", OBLIQUE_EYES, 6.0),
                                                ("mixed", AXIS_EYES, 6.0),
                                                ("grid", OBLIQUE_EYES, 4.0),
                                                ("grid", AXIS_EYES, 4.0)])
def test_the_seeded_scenes_are_decided_and_exercise_both_outcomes(name, eyes, distance):
    """The scenes of the GPU tests, reference alone: no pair sits on the threshold, and a good share
    of the pairs ends either way."""
    scale, nodes, ids = mixed_scene() if name == "mixed" else grid_scene()
    density = densities(scale, depth_of(ids), len(ids), 3)
    cameras = rig(eyes, distance, 32, 32, fov_deg=90.0)      # the whole cube in view
    proj, cam_eyes = camera_arrays(cameras, (0, 0, 0))
    images = constant_images([[k, 2 * k, 3 * k] for k in range(1, len(cameras) + 1)], 32, 32)
    out = vref.visible(scale, nodes, ids, density, images, proj, cam_eyes, 128, 0.3)
    pairs, undecided = out["pairs"], int(out["undecided"].sum())
    share = out["visible"].sum() / pairs
    print("%s, %d eyes: %d undecided of %d pairs, %.1f %% visible"
          % (name, len(eyes), undecided, pairs, 100 * share))
    assert pairs == len(ids) * len(eyes) and out["candidate"].all()
    assert undecided == 0
    assert 0.2 < share < 0.8
    assert (out["votes"][:, 3] == out["visible"].sum(1)).all()


# ------------------------------------------------------------------------------- cameras
def test_projection_matrices_with_an_origin_and_eye_positions_against_float64():
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES + OBLIQUE_EYES, 4.0, 40, 30)
    plain = ffn.projection_matrices(cameras)
    assert np.array_equal(bits(plain), bits(ffn.projection_matrices(cameras, origin=None)))
    for cam, matrix in zip(cameras, plain):           # today's result: the float64 product, rounded
        big = np.eye(4)
        big[:3, :3] = cam.intrinsics
        exact = (big @ np.linalg.inv(np.asarray(cam.extrinsics, np.float64)))[:3]
        assert np.array_equal(bits(matrix), bits(exact.astype(F)))
    center = (0.25, -1.5, 0.125)
    want_proj, want_eyes = camera_arrays(cameras, center)
    got = ffn.projection_matrices(cameras, origin=center)
    assert got.shape == (9, 3, 4) and got.dtype == F
    assert np.array_equal(bits(got), bits(want_proj))
    eyes = ffn.eye_positions(cameras, center)
    assert eyes.shape == (9, 3) and eyes.dtype == F
    assert np.array_equal(bits(eyes), bits(want_eyes))
    # a point relative to the origin through P' is the point itself through P, to rounding
    point = np.array([0.3, -0.2, 0.4])
    a = plain.astype(np.float64) @ np.append(point + center, 1.0)
    b = got.astype(np.float64) @ np.append(point, 1.0)
    assert np.allclose(a, b, rtol=0, atol=1e-4 * np.abs(a).max())
    assert np.array_equal(bits(ffn.projection_matrices(cameras, origin=(0, 0, 0))), bits(plain))


# ------------------------------------------------------------------------------- the C ABI
def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_the_symbol_is_declared_exported_and_documented():
    _lib, lib = library()
    assert SYMBOL in _lib.declared_symbols()
    assert getattr(lib, SYMBOL)
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    assert "K24" in text and "No counterpart in the reference" in text[text.index("K24"):]


def test_bad_arguments_return_nonzero_without_a_device():
    _, lib = library()
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    fn = getattr(lib, SYMBOL)
    fn.restype = ctypes.c_int
    f, i64, i = ctypes.c_float, ctypes.c_int64, ctypes.c_int
    buffer = (ctypes.c_float * 64)()
    base = ctypes.addressof(buffer)
    base += (-base) % 16
    host, odd, byte = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 1)

    def call(centers=host, leaves=8, depth=2, nodes=host, num_nodes=1, ids=host, data=host,
             stride=4, offset=3, images=host, blocks=host, cameras=2, height=4, width=4, alpha=128,
             tau=0.3, votes=host):
        return (centers, i64(leaves), f(1), i(depth), nodes, i64(num_nodes), ids, data, i(stride),
                i(offset), images, blocks, i(cameras), i(height), i(width), i(alpha), f(tau), votes,
                None)

    for kwargs, why in (({"centers": None}, "null argument"), ({"ids": None}, "null argument"),
                        ({"nodes": None}, "null argument"), ({"data": None}, "null argument"),
                        ({"images": None}, "null argument"), ({"blocks": None}, "null argument"),
                        ({"votes": None}, "null argument"),
                        ({"images": byte}, "images must be 4-byte aligned"),
                        ({"votes": odd}, "votes 16-byte aligned"),
                        ({"leaves": 0}, "num_leaves"), ({"leaves": 2 ** 31 + 1}, "num_leaves"),
                        ({"num_nodes": -1}, "num_nodes"),
                        ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
                        ({"cameras": 0}, "cameras >= 1"), ({"cameras": -3}, "cameras >= 1"),
                        ({"height": 0}, "height"), ({"width": 0}, "width"),
                        ({"height": (1 << 24) + 1}, "height"), ({"width": (1 << 24) + 1}, "width"),
                        ({"alpha": 0}, "alpha_u8"), ({"alpha": 256}, "alpha_u8"),
                        ({"tau": float("nan")}, "min_transmittance"),
                        ({"tau": -0.1}, "min_transmittance"), ({"tau": 1.0}, "min_transmittance"),
                        ({"stride": 0}, "stride"), ({"offset": -1}, "sigma_offset"),
                        ({"offset": 4}, "sigma_offset")):
        status = fn(*call(**kwargs))
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and SYMBOL in text and why in text, (kwargs, text)


def good():
    return dict(leaf_centers=torch.zeros((8, 3)), leaf_index=torch.arange(1, 9),
                rows=torch.zeros((8, 4)), stride=4, sigma_offset=3,
                images_u8=torch.zeros((3, 5, 7, 4), dtype=torch.uint8),
                proj=torch.ones((3, 3, 4)), eyes=torch.ones((3, 3)), depth=2, alpha_u8=128,
                min_transmittance=0.3)


def test_octree_visible_check_refuses_what_needs_no_device():
    from fourier_feature_nets_amd import ops
    assert ops.octree_visible_check(**good()) == (8, 3, 5, 7)
    nan = torch.ones((3, 3))
    nan[1, 2] = float("nan")
    for change, why in (
            ({"leaf_centers": torch.zeros((7, 3))}, "leaf_centers must be"),
            ({"leaf_centers": torch.zeros((8, 3), dtype=torch.float64)}, "leaf_centers must be a"),
            ({"leaf_index": torch.arange(1, 9, dtype=torch.int32)}, "leaf_index must be a"),
            ({"rows": torch.zeros((8, 5))}, "rows must be"),
            ({"stride": 0}, "stride"), ({"sigma_offset": 4}, "sigma_offset"),
            ({"images_u8": torch.zeros((3, 5, 7, 3), dtype=torch.uint8)}, "images_u8 must be"),
            ({"images_u8": torch.zeros((3, 5, 7, 4))}, "images_u8 must be a"),
            ({"images_u8": torch.zeros((0, 5, 7, 4), dtype=torch.uint8),
              "proj": torch.ones((0, 3, 4)), "eyes": torch.ones((0, 3))}, "0 cameras"),
            ({"proj": torch.ones((2, 3, 4))}, "proj must be"),
            ({"eyes": torch.ones((3, 4))}, "eyes must be"),
            ({"eyes": nan}, "NaN or an infinity"),
            ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
            ({"alpha_u8": 0}, "alpha_u8"), ({"alpha_u8": 256}, "alpha_u8"),
            ({"min_transmittance": 1.0}, "min_transmittance"),
            ({"min_transmittance": float("nan")}, "min_transmittance"),
            ({"out": torch.zeros((8, 4), dtype=torch.int32)}, "out must be a"),
            ({"out": torch.zeros((7, 4), dtype=torch.uint32)}, "out must be")):
        with pytest.raises(ValueError, match=why):
            ops.octree_visible_check(**{**good(), **change})
    # the check comes first: host tensors never reach a launch
    with pytest.raises(ValueError, match="alpha_u8"):
        ops.octree_visible_votes(scale=1.0, node_index=torch.zeros(1, dtype=torch.int64),
                                 **{**good(), "alpha_u8": 0})


# ------------------------------------------------------------------------------- the methods
class Untouched(Scene):
    """A dataset whose sampler (and with it the device) must not be asked for."""

    @property
    def sampler(self):
        raise AssertionError("went to the device before checking")


def test_the_methods_refuse_bad_arguments_before_any_device():
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES[:2], 4.0, 8, 8)
    images = np.zeros((2, 8, 8, 4), np.uint8)
    scene = Scene(images, cameras)
    nodes, ids = grid_tree(2, [(1, 0, 0, 0), (1, 1, 0, 0)])
    tree = ffn.OcTree(1.0, nodes, ids, np.zeros((2, 4), F))
    for method in (tree.visible_votes, tree.color_from_images):
        with pytest.raises(ValueError, match="pass center"):           # a loaded tree has none
            method(scene)
        with pytest.raises(ValueError, match="alpha_threshold"):
            method(scene, (0, 0, 0), alpha_threshold=1.5)
        for value in (1.0, -0.1, float("nan")):
            with pytest.raises(ValueError, match="min_transmittance"):
                method(scene, (0, 0, 0), min_transmittance=value)
        with pytest.raises(ValueError, match="alpha channel"):
            method(Scene(images[..., :3], cameras), (0, 0, 0))
        with pytest.raises(ValueError, match="color_space must be RGB"):
            method(Scene(images, cameras, "YCrCb"), (0, 0, 0))
        with pytest.raises(ValueError, match="1 cameras for 2 images"):
            method(Scene(images, cameras[:1]), (0, 0, 0))
    with pytest.raises(ValueError, match="leaf_data"):
        ffn.OcTree(1.0, nodes, ids).visible_votes(scene, (0, 0, 0))
    sh = ffn.OcTree(1.0, nodes, ids, np.zeros((2, 13), F), sh_degree=1)
    with pytest.raises(ValueError, match="OcTree.visible_votes"):       # names the way out
        sh.color_from_images(scene, (0, 0, 0))
    doc = ffn.OcTree.color_from_images.__doc__
    assert "one ray per" in doc.lower() and "untuned" in doc
    sig = inspect.signature(ffn.OcTree.color_from_images).parameters
    assert sig["min_transmittance"].default == 0.3 and sig["alpha_threshold"].default == 0.5
    assert inspect.signature(ffn.OcTree.visible_votes).parameters["min_transmittance"].default == 0.3


def test_build_from_silhouettes_routes_by_color(monkeypatch):
    """``color="mean"`` hands K23's cells straight to ``_from_cells`` and never asks for votes;
    ``color="visible"`` builds the unmerged hull, asks for its votes, and hands the recoloured rows,
    in code order, to ``_from_cells`` with the caller's tolerances.  (Host tensors, stubs for the
    kernels: the routing alone.)"""
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import octree as octree_module
    cameras = rig(AXIS_EYES[:2], 4.0, 8, 8)
    scene = Scene(np.full((2, 8, 8, 4), 255, np.uint8), cameras)
    scene.sampler = type("S", (), {"device": "cpu"})()
    codes = torch.tensor([3, 9, 12], dtype=torch.int32)
    data = torch.tensor([[.1, .2, .3, 5.], [.4, .5, .6, 5.], [.7, .8, .9, 5.]])
    calls = []

    def carve(*args, **kwargs):
        return codes.clone(), data.clone()

    def from_cells(codes_in, data_in, depth, scale, center, tolerances, device):
        calls.append((codes_in.clone(), data_in.clone(), tolerances))
        return "tree"

    asked = []

    class Hull:
        def _visible_votes_on_device(self, images, cams, alpha_u8, center, tau):
            asked.append((alpha_u8, center, tau, len(cams)))
            return torch.from_numpy(np.array([[255, 0, 510, 2], [0, 0, 0, 0], [51, 102, 153, 1]],
                                             np.uint32))

    monkeypatch.setattr(octree_module.ops, "octree_carve_select", carve)
    monkeypatch.setattr(ffn.OcTree, "_from_cells", staticmethod(from_cells))
    build = ffn.OcTree.build_from_silhouettes
    with pytest.raises(ValueError, match="color is 'mean' or 'visible'"):
        build(Untouched(scene.images, cameras), 3, color="front")
    with pytest.raises(ValueError, match="visible_transmittance"):
        build(Untouched(scene.images, cameras), 3, color="visible", visible_transmittance=1.0)
    # mean: one call, K23's rows untouched, no votes
    assert build(scene, 3, merge_tolerance=0.25) == "tree" and len(calls) == 1 and not asked
    assert torch.equal(calls[0][0], codes) and torch.equal(calls[0][1], data)
    assert calls[0][2] == (0.25, 0.25)
    assert build(scene, 3, merge_tolerance=0.25, color="mean") == "tree" and len(calls) == 2
    assert torch.equal(calls[1][1], data) and not asked
    # visible: the hull unmerged, then the recoloured rows with the tolerances
    calls.clear()
    monkeypatch.setattr(ffn.OcTree, "_from_cells",
                        staticmethod(lambda *a: (calls.append((a[0].clone(), a[1].clone(), a[5])),
                                                 Hull() if a[5] is None else "tree")[1]))
    assert build(scene, 3, center=(0.5, 0, 0), alpha_threshold=0.25, merge_tolerance=0.25,
                 color="visible", visible_transmittance=0.1) == "tree"
    assert asked == [(64, (0.5, 0.0, 0.0), 0.1, 2)]
    assert len(calls) == 2 and calls[0][2] is None and calls[1][2] == (0.25, 0.25)
    assert torch.equal(calls[0][1], data) and torch.equal(calls[1][0], codes)
    want = data.numpy().copy()
    want[0, :3] = F([255, 0, 510]) / F(510)
    want[2, :3] = F([51, 102, 153]) / F(255)
    assert np.array_equal(bits(calls[1][1].numpy()), bits(want))       # leaf 1: no vote, kept
    sig = inspect.signature(build).parameters
    assert sig["color"].default == "mean" and sig["visible_transmittance"].default == 0.3


# ------------------------------------------------------------------------------- the programs
def test_program_parsers():
    sys.path.insert(0, ROOT)
    import fourier_feature_nets as ffn
    from scripts import carve_octree, color_octree
    args = carve_octree.build_parser().parse_args(["d", "t"])
    assert args.color == "mean" and args.visible_transmittance == 0.3
    args = carve_octree.build_parser().parse_args(["d", "t", "--color", "visible",
                                                   "--visible-transmittance", "0.1"])
    assert args.color == "visible" and args.visible_transmittance == 0.1
    with pytest.raises(SystemExit):
        carve_octree.build_parser().parse_args(["d", "t", "--color", "front"])
    parser = color_octree.build_parser()
    args = parser.parse_args(["tree.npz", "data.npz", "out.npz"])
    assert (args.tree_path, args.data_path, args.output_path) == ("tree.npz", "data.npz", "out.npz")
    assert args.center == [0.0, 0.0, 0.0] and args.split == "train"
    sig = inspect.signature(ffn.OcTree.color_from_images).parameters
    assert args.alpha_threshold == sig["alpha_threshold"].default
    assert args.min_transmittance == sig["min_transmittance"].default
    args = parser.parse_args(["a", "b", "c", "--center", "0.5", "-1", "2", "--split", "val",
                              "--alpha-threshold", "0.25", "--min-transmittance", "0.1"])
    assert args.center == [0.5, -1.0, 2.0] and args.split == "val"
    assert args.alpha_threshold == 0.25 and args.min_transmittance == 0.1
    with pytest.raises(SystemExit):
        parser.parse_args(["a", "b"])
