"""K30 without a GPU: the dense numpy restatement of the mesh contract
(tests/octree_mesh_reference.py) against closed forms, that its budgets tell a wrong answer from a
right one on every case of the GPU tests, the argument checks of ``OcTree.extract_mesh``, of
``mesh.save_obj`` and of the C ABI, and an OBJ written and read back."""

import ctypes
import os

import numpy as np
import pytest

from tests import octree_mesh_reference as mref
from tests.octree_lattice_helpers import grid_tree, level_cells
from tests.octree_mesh_cases import CASES, CUBOID, case, parse_obj, reference


def test_lone_cell():
    ref = reference("lone")
    c = case("lone")
    assert len(ref.corners) == 8 and len(ref.triangles) == 12
    assert ref.cells == 4 and ref.side == 0.5
    # every vertex is pulled a third of a cell from its corner towards the cell's centre
    centre_corner = np.array([1, 2, 1]) + 0.5
    np.testing.assert_allclose(ref.offsets, np.sign(centre_corner - ref.corners) / 3, atol=1e-15)
    centre = (centre_corner - ref.cells / 2) * ref.side
    np.testing.assert_allclose(np.abs(ref.vertices - centre), ref.side / 6, atol=1e-15)
    volume = mref.six_volumes(ref.vertices, ref.triangles) / 6
    assert abs(volume - ref.side ** 3 / 27) <= 1e-15
    np.testing.assert_allclose(ref.colors, np.tile(c.leaf_data.astype(np.float64), (8, 1)))
    # the normals point away from the cell, along the diagonals
    np.testing.assert_allclose(ref.normals, -np.sign(centre_corner - ref.corners) / np.sqrt(3),
                               atol=1e-15)
    assert mref.euler_characteristic(8, ref.triangles) == 2


def test_lone_cell_one_level_up():
    """One level-1 leaf in a depth-3 tree spans 2^3 finest cells: a 2 x 2 x 2 cuboid."""
    ref = reference("lone_coarse")
    assert ref.cells == 4 and ref.solid_cells == 8
    assert len(ref.corners) == 27 - 1 and len(ref.triangles) == 4 * 12
    assert ref.corners.min(0).tolist() == [0, 2, 0] and ref.corners.max(0).tolist() == [2, 4, 2]
    assert mref.edges_pair_up(ref.triangles)
    block = reference("lone_coarse", "corners")
    assert mref.six_volumes(block.corners, block.triangles) == 6 * 8
    # the eight corners of the block move as the lone cell's do
    at_corner = ((ref.corners == ref.corners.min(0)) | (ref.corners == ref.corners.max(0))).all(1)
    assert at_corner.sum() == 8
    alpha = ref.alpha.max()
    # one solid sample of opacity a, three cut edges: t = 0.5 / a from the empty side
    np.testing.assert_allclose(np.abs(ref.offsets[at_corner]), (0.5 + 0.5 / alpha) / 3, atol=1e-12)


def test_cuboid_counts_and_euler():
    p, q, r = CUBOID
    ref = reference("cuboid")
    assert len(ref.corners) == (p + 1) * (q + 1) * (r + 1) - (p - 1) * (q - 1) * (r - 1)
    assert len(ref.triangles) == 4 * (p * q + q * r + r * p)
    assert mref.euler_characteristic(len(ref.corners), ref.triangles) == 2
    assert mref.edges_pair_up(ref.triangles)
    assert mref.six_volumes(ref.vertices, ref.triangles) > 0


def test_ring_is_a_torus():
    ref = reference("ring")
    assert ref.solid_cells == 8 and ref.colors is None
    assert mref.euler_characteristic(len(ref.corners), ref.triangles) == 0
    assert mref.edges_pair_up(ref.triangles)


def test_root_leaf_closes_at_the_cube():
    ref = reference("root")
    assert ref.cells == 1 and len(ref.corners) == 8 and len(ref.triangles) == 12
    assert sorted(map(tuple, ref.corners.tolist())) == [(i, j, k) for i in (0, 1) for j in (0, 1)
                                                        for k in (0, 1)]
    block = reference("root", "corners")
    np.testing.assert_array_equal(np.abs(block.vertices), 0.5)
    assert mref.six_volumes(block.corners, block.triangles) == 6
    full = reference("full")
    assert len(full.corners) == 5 ** 3 - 3 ** 3 and len(full.triangles) == 4 * 3 * 16
    assert ((full.corners == 0) | (full.corners == 4)).any(1).all()


def test_no_solid_leaf_is_an_empty_mesh():
    ref = reference("none_solid")
    assert ref.corners.shape == (0, 3) and ref.triangles.shape == (0, 3)
    assert ref.vertices.shape == (0, 3) and ref.colors.shape == (0, 3)


@pytest.mark.parametrize("seed", range(6))
def test_random_fields_are_closed_oriented_and_hold_their_volume(seed):
    rng = np.random.default_rng(seed)
    cells = level_cells(2, rng, int(rng.integers(1, 60)))
    nodes, leaves = grid_tree(3, cells)
    block = mref.extract(1.0, leaves, placement="corners")
    assert block.solid_cells == len(cells)
    assert mref.edges_pair_up(block.triangles)
    assert mref.six_volumes(block.corners, block.triangles) == 6 * len(cells)
    nets = mref.extract(1.0, leaves)
    np.testing.assert_array_equal(nets.triangles, block.triangles)
    assert mref.six_volumes(nets.vertices, nets.triangles) > 0
    # keys ascend
    key = (nets.corners[:, 0] * 5 + nets.corners[:, 1]) * 5 + nets.corners[:, 2]
    assert (np.diff(key) > 0).all()


@pytest.mark.parametrize("name", CASES)
def test_every_case_keeps_the_invariants_and_its_margin(name):
    ref = reference(name)
    block = reference(name, "corners")
    assert ref.margin >= 1e-3
    assert mref.edges_pair_up(ref.triangles)
    assert mref.six_volumes(block.corners, block.triangles) == 6 * ref.solid_cells
    np.testing.assert_array_equal(ref.triangles, block.triangles)
    if case(name).euler is not None:
        assert mref.euler_characteristic(len(ref.corners), ref.triangles) == case(name).euler
    assert (np.abs(ref.offsets) <= 0.5).all()


@pytest.mark.parametrize("name", [n for n in CASES if n != "none_solid"])
def test_the_budgets_tell_a_wrong_answer_from_a_right_one(name):
    """The offset of a neighbouring vertex, or a ``t`` computed with its pair swapped, misses the
    budget; so do a neighbour's colour and normal where the tree has more than one of either."""
    ref = reference(name)
    assert np.isfinite(ref.offset_budget).all() and ref.offset_budget.max() < 1e-3
    edges = np.concatenate([ref.triangles[:, [0, 1]], ref.triangles[:, [1, 2]]])
    u, v = edges[:, 0], edges[:, 1]
    budget = ref.offset_budget
    neighbour = np.abs(ref.offsets[u] - ref.offsets[v]).max(1) > 4 * np.maximum(budget[u], budget[v])
    swapped = np.abs(ref.swapped_offsets - ref.offsets).max(1) > 4 * budget
    assert neighbour.any() or swapped.any()
    if ((ref.alpha > 0.01) & (ref.alpha < 0.99)).any():
        assert swapped.any()                     # graded opacities: the pair's order matters
    # positions: a neighbouring vertex is a cell away
    assert ref.vertex_budget.max() < 1e-3 * ref.side
    # normals: of neighbouring vertices that do not share theirs, some differ by more than both budgets
    differ = np.abs(ref.normals[u] - ref.normals[v]).max(1)
    assert (differ > 4 * np.maximum(ref.normal_budget[u], ref.normal_budget[v])).any()
    assert np.median(ref.normal_budget) < 1e-3
    if ref.colors is not None and len(np.unique(ref.colors, axis=0)) > 1:
        assert ref.color_budget < 1e-4
        assert (np.abs(ref.colors[u] - ref.colors[v]).max(1) > 4 * ref.color_budget).any()


# ------------------------------------------------------------------------------ the layers
def tree_of(name):
    from fourier_feature_nets_amd.octree import OcTree
    c = case(name)
    return OcTree(c.scale, c.nodes, c.leaves, c.leaf_data, c.sh_degree)


def test_extract_mesh_refuses_bad_arguments_before_any_device():
    tree = tree_of("mixed")
    for bad in (0.0, 1.0, -0.5, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha_threshold"):
            tree.extract_mesh(alpha_threshold=bad)
    with pytest.raises(ValueError, match="placement"):
        tree.extract_mesh(placement="marching_cubes")
    with pytest.raises(ValueError, match="solid"):
        tree.extract_mesh(solid=np.zeros(tree.num_leaves + 1, bool))
    with pytest.raises(TypeError, match="solid"):
        tree.extract_mesh(solid=np.zeros(tree.num_leaves, np.uint8))
    with pytest.raises(ValueError, match="batch_size"):
        tree.extract_mesh(batch_size=0)
    with pytest.raises(ValueError, match="center"):
        tree.extract_mesh(center=(0.0, float("nan"), 0.0))
    from fourier_feature_nets_amd.octree import OcTree
    c = case("lone")
    with pytest.raises(ValueError, match="leaf_data"):
        OcTree(c.scale, c.nodes, c.leaves, np.zeros((1, 2), np.float32)).extract_mesh()


def test_ops_refuse_cpu_tensors_and_bad_arguments():
    import torch
    from fourier_feature_nets_amd import ops
    with pytest.raises(ValueError, match="placement"):
        ops.octree_mesh_check(0.5, "dual")
    with pytest.raises(ValueError, match="alpha_threshold"):
        ops.octree_mesh_check(float("nan"), "corners")
    assert ops.octree_mesh_check(0.25, "corners") == (0.25, False)
    keys = torch.zeros(4, dtype=torch.int64)
    masks = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="GPU"):
        ops.octree_mesh_faces(keys, masks, 3)
    with pytest.raises(ValueError, match="disagree"):
        ops.octree_mesh_faces(keys, masks[:3], 3)
    with pytest.raises(ValueError, match="disagree"):
        ops.octree_mesh_vertices(keys, masks, torch.zeros((4, 7), dtype=torch.int32),
                                 torch.zeros(2), None, None, 3, 1.0, (0, 0, 0), 0.5, True)
    with pytest.raises(ValueError, match="solid"):
        ops.octree_mesh_solid(None, 0, torch.zeros(3, dtype=torch.uint8), 4, 0.5, 0.5, "cpu")
    with pytest.raises(ValueError, match="cand_offsets"):
        ops.octree_mesh_candidates(keys[:0], keys, masks, keys, 0, 8, 3)


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_the_abi_declares_and_refuses_by_name_without_a_device():
    _lib, lib = library()
    names = {"ffn_octree_mesh_max_depth", "ffn_octree_mesh_solid", "ffn_octree_mesh_candidates",
             "ffn_octree_mesh_vertices", "ffn_octree_mesh_face_flags", "ffn_octree_mesh_faces"}
    assert names <= set(_lib.declared_symbols())
    assert lib.ffn_octree_mesh_max_depth() == 21
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    f, i64 = ctypes.c_float, ctypes.c_int64
    host = (ctypes.c_float * 64)()
    good = ctypes.c_void_p(ctypes.addressof(host))

    def refused(status, who, why):
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and who in text and why in text, (who, why, text)

    def solid(rows=good, stride=4, offset=3, n=4, side=0.5, thr=0.5, out=good):
        return lib.ffn_octree_mesh_solid(rows, stride, offset, None, i64(n), f(side), f(thr), out,
                                         out, None)

    for kwargs, why in (({"n": 0}, "shape"), ({"out": None}, "null argument"),
                        ({"thr": 0.0}, "threshold"), ({"thr": 1.0}, "threshold"),
                        ({"thr": float("nan")}, "threshold"), ({"side": 0.0}, "side"),
                        ({"side": float("inf")}, "side"), ({"stride": 0}, "sigma_offset"),
                        ({"offset": 4}, "sigma_offset"), ({"offset": -1}, "sigma_offset")):
        refused(solid(**kwargs), "ffn_octree_mesh_solid", why)

    def candidates(leaves=1, depth=3, first=0, count=8, p=good, nodes=0):
        return lib.ffn_octree_mesh_candidates(None, i64(nodes), p, i64(leaves), p, p, i64(first),
                                              i64(count), depth, p, p, p, p, p, p, p, p, p, p, None)

    for kwargs, why in (({"leaves": 0}, "shape"), ({"depth": 0}, "depth"), ({"depth": 22}, "depth"),
                        ({"first": -1}, "count"), ({"count": 0}, "count"),
                        ({"count": 1 << 31}, "count"), ({"p": None}, "null argument"),
                        ({"nodes": 3}, "null argument")):
        refused(candidates(**kwargs), "ffn_octree_mesh_candidates", why)

    def vertices(count=4, leaves=2, depth=3, rows=good, colors=good, stride=4, offset=0, step=1,
                 scale=1.0, thr=0.5, cx=0.0, p=good):
        return lib.ffn_octree_mesh_vertices(p, p, p, i64(count), p, rows, i64(leaves), stride,
                                            offset, step, 0, depth, f(scale), f(cx), f(0), f(0),
                                            f(thr), 1, p, colors, p, p, None)

    for kwargs, why in (({"count": 0}, "shape"), ({"leaves": 0}, "shape"), ({"depth": 22}, "depth"),
                        ({"p": None}, "null argument"), ({"rows": None}, "go together"),
                        ({"colors": None}, "go together"), ({"offset": 2}, "colour columns"),
                        ({"step": 2}, "colour columns"), ({"step": 0}, "colour columns"),
                        ({"thr": 1.0}, "threshold"), ({"scale": 0.0}, "scale"),
                        ({"cx": float("nan")}, "centre")):
        refused(vertices(**kwargs), "ffn_octree_mesh_vertices", why)

    refused(lib.ffn_octree_mesh_face_flags(good, i64(0), good, good, good, good, None),
            "ffn_octree_mesh_face_flags", "shape")
    refused(lib.ffn_octree_mesh_face_flags(good, i64(4), good, None, good, good, None),
            "ffn_octree_mesh_face_flags", "null argument")
    for args, why in (((i64(0), 3, i64(1)), "shape"), ((i64(4), 3, i64(13)), "shape"),
                      ((i64(4), 3, i64(0)), "shape"), ((i64(4), 0, i64(2)), "depth")):
        refused(lib.ffn_octree_mesh_faces(good, good, good, good, args[0], args[1], args[2], good,
                                          good, None), "ffn_octree_mesh_faces", why)
    refused(lib.ffn_octree_mesh_faces(good, good, good, good, i64(4), 3, i64(2), None, good, None),
            "ffn_octree_mesh_faces", "null argument")


def test_save_obj_keeps_every_bit(tmp_path):
    from fourier_feature_nets_amd import mesh
    ref = reference("levels")
    rng = np.random.default_rng(3)
    # awkward floats: every exponent, denormals, values that need all nine digits
    vertices = ref.vertices.astype(np.float32)
    vertices[:8] = rng.integers(1, 2 ** 31 - 2 ** 23, (8, 3)).astype(np.uint32).view(np.float32)
    vertices[8] = [np.float32(1e-45), np.float32(-0.0), np.float32(16777217.0)]
    colors = ref.colors.astype(np.float32)
    normals = ref.normals.astype(np.float32)
    triangles = ref.triangles.astype(np.int32)
    path = str(tmp_path / "levels.obj")
    mesh.save_obj(path, vertices, triangles, colors, normals)
    v, c, n, f, paired = parse_obj(path)
    assert paired
    np.testing.assert_array_equal(v.view(np.uint32), vertices.view(np.uint32))
    np.testing.assert_array_equal(c.view(np.uint32), colors.view(np.uint32))
    np.testing.assert_array_equal(n.view(np.uint32), normals.view(np.uint32))
    np.testing.assert_array_equal(f, triangles)
    # no colours, no normals: plain v and f records
    mesh.save_obj(path, vertices, triangles)
    v, c, n, f, paired = parse_obj(path)
    assert c is None and n is None and not paired
    np.testing.assert_array_equal(v.view(np.uint32), vertices.view(np.uint32))
    np.testing.assert_array_equal(f, triangles)
    with open(path) as text:
        assert all("/" not in line for line in text if line.startswith("f "))
    # an empty mesh is a file without records
    mesh.save_obj(path, np.zeros((0, 3), np.float32), np.zeros((0, 3), np.int32))
    assert parse_obj(path)[3].shape == (0, 3)


def test_save_obj_refuses_bad_arguments(tmp_path):
    from fourier_feature_nets_amd import mesh
    path = str(tmp_path / "bad.obj")
    vertices = np.zeros((4, 3), np.float32)
    triangles = np.array([[0, 1, 2]], np.int32)
    with pytest.raises(ValueError, match="vertices"):
        mesh.save_obj(path, np.zeros((4, 2)), triangles)
    with pytest.raises(ValueError, match="triangles"):
        mesh.save_obj(path, vertices, np.zeros((1, 3), np.float32))
    with pytest.raises(ValueError, match="triangles"):
        mesh.save_obj(path, vertices, np.zeros((3,), np.int32))
    with pytest.raises(ValueError, match="outside"):
        mesh.save_obj(path, vertices, np.array([[0, 1, 4]]))
    with pytest.raises(ValueError, match="colors"):
        mesh.save_obj(path, vertices, triangles, colors=np.zeros((3, 3)))
    with pytest.raises(ValueError, match="normals"):
        mesh.save_obj(path, vertices, triangles, normals=np.zeros((4, 2)))
    assert not os.path.exists(path)
