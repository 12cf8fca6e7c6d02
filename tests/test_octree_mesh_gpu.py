"""K30 on the GPU: ``OcTree.extract_mesh`` against the dense numpy restatement of its contract
(tests/octree_mesh_reference.py).  Corners, masks and triangles bit for bit; the block surface bit
for bit against its own f32 expression; surface-nets positions, colours and normals within the
budgets the reference derives; the invariants on the device output itself; the same bits on a second
call and over several chunks; the script in a fresh process."""

import os
import subprocess
import sys

import numpy as np
import pytest

from tests import octree_mesh_reference as mref
from tests.octree_mesh_cases import CASES, case, parse_obj, reference

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_MESHES = {}


def tree_of(name):
    from fourier_feature_nets_amd.octree import OcTree
    c = case(name)
    return OcTree(c.scale, c.nodes, c.leaves, c.leaf_data, c.sh_degree)


def mesh_of(name, placement="surface_nets"):
    """The device mesh of a case, extracted once and shared: do not write into it."""
    key = (name, placement)
    if key not in _MESHES:
        _MESHES[key] = tree_of(name).extract_mesh(placement=placement, **case(name).kwargs)
    return _MESHES[key]


def same_bits(a, b):
    for x, y in zip(a, b):
        if x is None or y is None:
            assert x is None and y is None
            continue
        assert x.dtype == y.dtype and x.shape == y.shape
        np.testing.assert_array_equal(x.view(np.uint8), y.view(np.uint8))


def check_types(mesh, colours):
    count, faces = len(mesh.vertices), len(mesh.triangles)
    assert mesh.vertices.dtype == np.float32 and mesh.vertices.shape == (count, 3)
    assert mesh.triangles.dtype == np.int32 and mesh.triangles.shape == (faces, 3)
    assert mesh.normals.dtype == np.float32 and mesh.normals.shape == (count, 3)
    assert mesh.corners.dtype == np.int32 and mesh.corners.shape == (count, 3)
    assert mesh.masks.dtype == np.uint8 and mesh.masks.shape == (count,)
    if colours:
        assert mesh.colors.dtype == np.float32 and mesh.colors.shape == (count, 3)
    else:
        assert mesh.colors is None


@pytest.mark.parametrize("name", CASES)
def test_the_mesh_is_the_contracts(name):
    ref = reference(name)
    assert ref.margin >= 1e-3                # no leaf's solidity hangs on the last bit of expm1f
    mesh = mesh_of(name)
    check_types(mesh, case(name).leaf_data is not None)
    # integers: exactly
    np.testing.assert_array_equal(mesh.corners, ref.corners)
    np.testing.assert_array_equal(mesh.masks, ref.masks)
    np.testing.assert_array_equal(mesh.triangles, ref.triangles)
    # floats: within the budgets the reference derives
    error = np.abs(mesh.vertices.astype(np.float64) - ref.vertices).max(1)
    print(name, "positions: worst error / budget",
          (error / ref.vertex_budget).max() if len(error) else 0.0)
    assert (error <= ref.vertex_budget).all()
    error = np.abs(mesh.normals.astype(np.float64) - ref.normals).max(1)
    print(name, "normals: worst error / budget",
          (error / np.maximum(ref.normal_budget, 1e-300)).max() if len(error) else 0.0)
    assert (error <= ref.normal_budget).all()
    if ref.colors is not None:
        error = np.abs(mesh.colors.astype(np.float64) - ref.colors)
        print(name, "colours: worst error / budget",
              error.max() / ref.color_budget if error.size else 0.0)
        assert (error <= ref.color_budget).all()
    # a second call gives the same bits in every output
    again = tree_of(name).extract_mesh(**case(name).kwargs)
    same_bits(mesh, again)


@pytest.mark.parametrize("name", CASES)
def test_the_block_surface_is_exact_and_the_invariants_hold_on_the_device_output(name):
    c, ref = case(name), reference(name, "corners")
    block = mesh_of(name, "corners")
    nets = mesh_of(name)
    np.testing.assert_array_equal(block.corners, ref.corners)
    np.testing.assert_array_equal(block.triangles, ref.triangles)
    np.testing.assert_array_equal(block.masks, nets.masks)
    # center + (c - n/2) * side, in f32, in that order
    center = np.float32(c.kwargs.get("center", (0.0, 0.0, 0.0)))
    cells = block.corners.astype(np.float32) - np.float32(ref.cells / 2)
    expected = center + cells * np.float32(ref.side)
    assert expected.dtype == np.float32
    np.testing.assert_array_equal(block.vertices.view(np.uint32), expected.view(np.uint32))
    # colours and normals do not depend on the placement
    same_bits((block.colors, block.normals), (nets.colors, nets.normals))
    for mesh in (block, nets):
        assert mref.edges_pair_up(mesh.triangles)
        if c.euler is not None:
            assert mref.euler_characteristic(len(mesh.vertices), mesh.triangles) == c.euler
    assert mref.six_volumes(block.corners, block.triangles) == 6 * ref.solid_cells
    if len(nets.vertices):
        assert mref.six_volumes(nets.vertices, nets.triangles) > 0
        assert (mesh.triangles.min() >= 0) and mesh.triangles.max() < len(mesh.vertices)


def test_closed_forms_on_the_device():
    lone = mesh_of("lone")
    assert len(lone.vertices) == 8 and len(lone.triangles) == 12
    ref = reference("lone")
    centre = (np.array([1, 2, 1]) + 0.5 - ref.cells / 2) * ref.side
    np.testing.assert_allclose(np.abs(lone.vertices - centre), ref.side / 6, rtol=1e-6)
    volume = mref.six_volumes(lone.vertices, lone.triangles) / 6
    assert abs(volume - ref.side ** 3 / 27) <= 1e-6 * ref.side ** 3
    coarse = mesh_of("lone_coarse")
    assert len(coarse.vertices) == 26 and len(coarse.triangles) == 48
    empty = mesh_of("none_solid")
    assert len(empty.vertices) == 0 and len(empty.triangles) == 0
    assert empty.colors.shape == (0, 3)
    root = mesh_of("root", "corners")
    np.testing.assert_array_equal(np.abs(root.vertices), np.float32(0.5))


@pytest.mark.parametrize("name,batch", [("lone_coarse", 7), ("levels", 100), ("mixed", 1000),
                                        ("random_sh2", 333), ("root", 1)])
def test_several_chunks_give_the_bits_of_one(name, batch):
    """The chunk boundaries fall inside the candidates of single leaves: the level-1 leaf of
    ``lone_coarse`` has 26 candidates, that of ``levels`` 386."""
    from fourier_feature_nets_amd import ops
    import torch
    tree = tree_of(name)
    chunked = tree.extract_mesh(batch_size=batch, **case(name).kwargs)
    same_bits(mesh_of(name), chunked)
    ref = reference(name)
    flags = torch.from_numpy((ref.alpha > ref.threshold).astype(np.uint8)).cuda()
    offsets, total, _ = ops.octree_mesh_candidate_offsets(
        torch.from_numpy(case(name).leaves).cuda(), flags, mref.tree_depth(case(name).leaves))
    offsets = offsets.cpu().numpy()
    assert total > batch
    cuts = np.arange(batch, total, batch)
    inside = np.searchsorted(offsets, cuts, side="right") - 1
    assert (offsets[inside] < cuts).any()            # a cut strictly inside a leaf's candidates


def test_a_solid_mask_as_a_device_tensor_and_thresholds_that_do_not_count():
    import torch
    c = case("mixed_solid")
    tree = tree_of("mixed_solid")
    mesh = tree.extract_mesh(solid=torch.from_numpy(c.kwargs["solid"]).cuda())
    same_bits(mesh_of("mixed_solid"), mesh)
    # the threshold is 0.5 whatever was passed
    same_bits(mesh, tree.extract_mesh(alpha_threshold=0.9, solid=c.kwargs["solid"]))
    colours = tree_of("random_colors")
    same_bits(mesh_of("random_colors"), colours.extract_mesh(alpha_threshold=0.123))


def test_the_faces_entry_refuses_keys_that_are_not_there():
    import torch
    from fourier_feature_nets_amd import ops
    from fourier_feature_nets_amd._lib import FfnError
    mesh = mesh_of("lone")
    n1 = reference("lone").cells + 1
    corners = torch.from_numpy(mesh.corners.astype(np.int64)).cuda()
    keys = (corners[:, 0] * n1 + corners[:, 1]) * n1 + corners[:, 2]
    masks = torch.from_numpy(mesh.masks).cuda()
    triangles = ops.octree_mesh_faces(keys, masks, 3)
    np.testing.assert_array_equal(triangles.cpu().numpy(), mesh.triangles)
    with pytest.raises(FfnError, match="not among the vertices"):
        ops.octree_mesh_faces(keys[:-1].contiguous(), masks[:-1].contiguous(), 3)


def test_the_script_writes_the_mesh_in_a_fresh_process(tmp_path):
    c = case("lone_coarse")
    tree = tree_of("lone_coarse")
    tree_path, obj_path = str(tmp_path / "tree.npz"), str(tmp_path / "tree.obj")
    tree.save(tree_path)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "octree_to_mesh.py"),
                          tree_path, obj_path, "--center", "0.25", "-1", "3"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    mesh = tree.extract_mesh(center=(0.25, -1.0, 3.0))
    assert "%d vertices, %d triangles" % (len(mesh.vertices), len(mesh.triangles)) in out.stdout
    vertices, colors, normals, faces, paired = parse_obj(obj_path)
    assert paired and c.leaf_data is not None
    np.testing.assert_array_equal(vertices.view(np.uint32), mesh.vertices.view(np.uint32))
    np.testing.assert_array_equal(colors.view(np.uint32), mesh.colors.view(np.uint32))
    np.testing.assert_array_equal(normals.view(np.uint32), mesh.normals.view(np.uint32))
    np.testing.assert_array_equal(faces, mesh.triangles)
