"""K30 at depths 11, 12, 16 and 21 on the GPU, where leaf ids and corner keys pass 2^31 and reach
2^60: ``OcTree.extract_mesh`` on sparse deep trees (tests/octree_deep_cases.py) against the sparse
restatement of its contract (tests/octree_mesh_sparse_reference.py) and against the device's own
mesh of the shallow tree that each deep tree embeds.

A shallow case under one cell of a deep tree has the shallow mesh, moved: the same masks and
triangles, corners shifted by the cell's offset, and -- the finest side keeps its bits -- the same
bits in every normal and colour.  Block-surface positions have the bits of ``center + (c - n/2)
side`` in f32; surface-nets positions lie within the per-vertex budget of the sparse reference,
which is the dense module's derivation with the vertex's own ``|c - n/2|``.

NO TREE HERE HAS A SOLID LEAF OF MORE THAN 8^3 FINEST CELLS: see ``deep_mesh``."""

import functools

import numpy as np
import pytest

from tests import octree_deep_cases as deep
from tests import octree_mesh_reference as mref
from tests import octree_mesh_sparse_reference as sref
from tests.octree_lattice_helpers import cell_id, grid_tree
from tests.octree_mesh_cases import case, reference
from tests.test_octree_mesh_gpu import check_types, mesh_of, same_bits

pytestmark = pytest.mark.gpu


def tree_of(m):
    from fourier_feature_nets_amd.octree import OcTree
    return OcTree(m.scale, m.nodes, m.leaves, m.leaf_data, m.sh_degree)


@functools.lru_cache(maxsize=None)
def deep_reference(name, depth, place):
    m = deep.deep_mesh(name, depth, place)
    return sref.extract(m.scale, m.leaves, m.leaf_data, m.sh_degree)


def candidate_counts(leaves, flags, depth):
    import torch
    from fourier_feature_nets_amd import ops
    offsets, total, _ = ops.octree_mesh_candidate_offsets(
        torch.from_numpy(leaves).cuda(), torch.from_numpy(flags.astype(np.uint8)).cuda(), depth)
    offsets = offsets.cpu().numpy()
    assert offsets.dtype == np.int64 and offsets[-1] == total
    return np.diff(offsets), total, offsets


@pytest.mark.parametrize("place", deep.MESH_PLACES)
@pytest.mark.parametrize("name", deep.MESH_NAMES)
@pytest.mark.parametrize("depth", deep.MESH_DEPTHS)
def test_a_deep_tree_has_the_shallow_mesh_moved(depth, name, place):
    m = deep.deep_mesh(name, depth, place)
    ref = deep_reference(name, depth, place)
    shallow = mesh_of(name)
    tree = tree_of(m)
    assert tree.depth == depth
    nets = tree.extract_mesh()
    block = tree.extract_mesh(placement="corners")
    for mesh in (nets, block):
        check_types(mesh, True)
        sref.check_integers(mesh.corners, mesh.masks, mesh.triangles, ref)
        np.testing.assert_array_equal(mesh.corners, shallow.corners.astype(np.int64) + m.shift)
        np.testing.assert_array_equal(mesh.masks, shallow.masks)
        np.testing.assert_array_equal(mesh.triangles, shallow.triangles)
        # the finest side has the shallow case's bits, and with it every opacity
        same_bits((mesh.normals, mesh.colors), (shallow.normals, shallow.colors))
        assert mref.edges_pair_up(mesh.triangles)
        euler = mref.euler_characteristic(len(mesh.vertices), mesh.triangles)
        assert euler == mref.euler_characteristic(len(shallow.vertices), shallow.triangles)
        assert case(name).euler in (None, euler)
    assert ref.corners.max() == ref.cells or place != "ones"       # vertices on the + faces
    assert mref.six_volumes(block.corners - m.shift, block.triangles) == 6 * ref.solid_cells
    # center + (c - n/2) * side, in f32, in that order
    cells = block.corners.astype(np.float32) - np.float32(ref.cells / 2)
    assert np.array_equal(cells.astype(np.int64), ref.corners - ref.cells // 2)
    expected = np.float32(0.0) + cells * np.float32(ref.side)
    assert expected.dtype == np.float32
    np.testing.assert_array_equal(block.vertices.view(np.uint32), expected.view(np.uint32))
    error = np.abs(nets.vertices.astype(np.float64) - ref.vertices).max(1)
    print("%s D=%d %s: %d vertices, largest key %.3g; positions: worst error / budget %.3f, "
          "budgets %.3g .. %.3g of a cell"
          % (name, depth, place, len(error), float(ref.cells + 1) ** 3,
             (error / ref.vertex_budget).max(), ref.vertex_budget.min() / ref.side,
             ref.vertex_budget.max() / ref.side))
    assert (error <= ref.vertex_budget).all()
    error = np.abs(nets.normals.astype(np.float64) - ref.normals).max(1)
    assert (error <= ref.normal_budget).all()
    assert (np.abs(nets.colors.astype(np.float64) - ref.colors) <= ref.color_budget).all()
    # the level-1 leaf of density 0 (2^(D-2) cells a side) has no candidates
    counts, total, _ = candidate_counts(m.leaves, ref.alpha > ref.threshold, depth)
    zero = np.searchsorted(m.leaves, cell_id(*deep.ZERO_LEAF))
    assert counts[zero] == 0 and ref.alpha[zero] == 0
    c, shallow_ref = case(name), reference(name)
    shallow_counts, shallow_total, _ = candidate_counts(
        c.leaves, shallow_ref.alpha > shallow_ref.threshold, mref.tree_depth(c.leaves))
    assert total == shallow_total and np.array_equal(counts[m.slots], shallow_counts)


@pytest.mark.parametrize("place", deep.MESH_PLACES)
@pytest.mark.parametrize("name", deep.MESH_NAMES)
@pytest.mark.parametrize("depth", deep.MESH_DEPTHS)
def test_a_callers_mask_empties_a_level_one_leaf(depth, name, place):
    """The masked leaf would be solid by its density (6 * 4^(D-2) + 2 candidates): it is only ever
    extracted with the mask."""
    from fourier_feature_nets_amd.octree import OcTree
    m = deep.deep_mesh(name, depth, place, masked=True)
    assert m.solid is not None and m.solid.dtype == bool
    c = case(name)
    under = OcTree(c.scale, c.nodes, c.leaves, c.leaf_data, c.sh_degree).extract_mesh(
        solid=m.solid[m.slots])
    ref = sref.extract(m.scale, m.leaves, m.leaf_data, m.sh_degree, solid=m.solid)
    counts, total, _ = candidate_counts(m.leaves, m.solid, depth)
    level_one = np.searchsorted(m.leaves, [cell_id(*deep.ZERO_LEAF), cell_id(*deep.MASKED_LEAF)])
    assert (counts[level_one] == 0).all() and total == counts[m.slots].sum() > 0
    for placement in ("corners", "surface_nets"):
        mesh = tree_of(m).extract_mesh(solid=m.solid, placement=placement)
        check_types(mesh, True)
        sref.check_integers(mesh.corners, mesh.masks, mesh.triangles, ref)
        np.testing.assert_array_equal(mesh.corners, under.corners.astype(np.int64) + m.shift)
        np.testing.assert_array_equal(mesh.triangles, under.triangles)
        same_bits((mesh.masks, mesh.normals, mesh.colors),
                  (under.masks, under.normals, under.colors))
        assert mref.edges_pair_up(mesh.triangles)
    # the surface-nets mesh (the last of the two) against the reference's positions
    error = np.abs(mesh.vertices.astype(np.float64) - ref.vertices).max(1)
    print("masked %s D=%d %s: %d vertices; positions: worst error / budget %.3f"
          % (name, depth, place, len(error), (error / ref.vertex_budget).max()))
    assert (error <= ref.vertex_budget).all()
    assert (np.abs(mesh.colors.astype(np.float64) - ref.colors) <= ref.color_budget).all()


CENTER = (30000.5, -1.7, 290000.25)     # of the size of the depth-21 cube (scale 2^17), and small


@pytest.mark.parametrize("place", deep.MESH_PLACES)
def test_a_cube_that_is_not_at_the_origin_at_depth_21(place):
    """``center + (c - n/2) side``: the centre is added last, and its size enters the budget."""
    m = deep.deep_mesh("levels", 21, place)
    tree = tree_of(m)
    ref = sref.extract(m.scale, m.leaves, m.leaf_data, m.sh_degree, center=CENTER)
    plain = deep_reference("levels", 21, place)
    assert (ref.vertex_budget > plain.vertex_budget).all()
    block = tree.extract_mesh(placement="corners", center=CENTER)
    nets = tree.extract_mesh(center=CENTER)
    for mesh in (block, nets):
        sref.check_integers(mesh.corners, mesh.masks, mesh.triangles, ref)
    cells = block.corners.astype(np.float32) - np.float32(ref.cells / 2)
    product = cells * np.float32(ref.side)                 # a power of two: exact
    assert np.array_equal(product.astype(np.float64),
                          (ref.corners - ref.cells // 2) * ref.side)
    expected = np.float32(CENTER)[None, :] + product
    assert expected.dtype == np.float32
    np.testing.assert_array_equal(block.vertices.view(np.uint32), expected.view(np.uint32))
    assert (expected != product).all()                     # the centre moved every coordinate
    error = np.abs(nets.vertices.astype(np.float64) - ref.vertices).max(1)
    print("levels D=21 %s, centre %s: positions: worst error / budget %.3f, budgets %.3g .. %.3g of "
          "a cell" % (place, CENTER, (error / ref.vertex_budget).max(),
                      ref.vertex_budget.min() / ref.side, ref.vertex_budget.max() / ref.side))
    assert (error <= ref.vertex_budget).all()
    same_bits((nets.normals, nets.colors), (mesh_of("levels").normals, mesh_of("levels").colors))


@pytest.mark.parametrize("name,batch", [("levels", 100), ("lone_coarse", 7)])
def test_chunks_that_cut_inside_a_leaf_at_depth_21_give_the_bits_of_one(name, batch):
    m = deep.deep_mesh(name, 21, "ones")
    ref = deep_reference(name, 21, "ones")
    tree = tree_of(m)
    same_bits(tree.extract_mesh(), tree.extract_mesh(batch_size=batch))
    _, total, offsets = candidate_counts(m.leaves, ref.alpha > ref.threshold, 21)
    assert total > batch
    cuts = np.arange(batch, total, batch)
    inside = np.searchsorted(offsets, cuts, side="right") - 1
    assert (offsets[inside] < cuts).any()            # a cut strictly inside a leaf's candidates


def test_every_entry_point_on_one_finest_cell_at_the_far_corner_of_depth_21():
    import torch
    from fourier_feature_nets_amd import ops
    from fourier_feature_nets_amd._lib import FfnError
    depth = 21
    n = 1 << (depth - 1)
    nodes, leaves = grid_tree(depth, [(depth - 1, n - 1, n - 1, n - 1)])
    assert len(nodes) == 20 and int(leaves[0]) == (8 ** 21 - 1) // 7 - 1     # the largest id there is
    dev_nodes, dev_leaves = torch.from_numpy(nodes).cuda(), torch.from_numpy(leaves).cuda()
    flags = torch.ones(1, dtype=torch.uint8, device="cuda")
    offsets, total, top = ops.octree_mesh_candidate_offsets(dev_leaves, flags, depth)
    assert offsets.cpu().tolist() == [0, 8] and total == 8 and top == depth - 1
    keys, masks, samples = ops.octree_mesh_candidates(dev_nodes, dev_leaves, flags, offsets, 0, 8,
                                                      depth)
    corners = [(n - 1 + dx, n - 1 + dy, n - 1 + dz) for dx in (0, 1) for dy in (0, 1) for dz in (0, 1)]
    want = [(i * (n + 1) + j) * (n + 1) + k for i, j, k in corners]         # Python integers
    assert want[-1] == (n + 1) ** 3 - 1 and want[-1] > 2 ** 60
    assert keys.dtype == torch.int64 and keys.cpu().tolist() == want
    # the cell is sample (1 - dx, 1 - dy, 1 - dz) of its corner cell + (dx, dy, dz)
    assert masks.cpu().tolist() == [1 << (7 - b) for b in range(8)]
    picked = samples.cpu().numpy()
    assert ((picked == 0).sum(1) == 1).all() and ((picked == -1).sum(1) == 7).all()
    alpha = torch.ones(1, device="cuda")
    for nets in (False, True):
        vertices, colors, normals, got = ops.octree_mesh_vertices(
            keys, masks, samples, alpha, None, None, depth, 1.0, (0.0, 0.0, 0.0), 0.5, nets)
        assert colors is None and got.dtype == torch.int32 and got.cpu().tolist() == \
            [list(c) for c in corners]
        side = np.float32(2.0) / np.float32(n)
        expected = (np.float32(corners) - np.float32(n / 2)) * side
        if nets:                                     # threshold 0.5 between 1 and 0: a third in
            assert np.abs(vertices.cpu().numpy() - expected).max() <= 0.5 * side
        else:
            np.testing.assert_array_equal(vertices.cpu().numpy().view(np.uint32),
                                          expected.view(np.uint32))
    triangles = ops.octree_mesh_faces(keys, masks, depth)
    assert triangles.shape == (12, 3) and triangles.dtype == torch.int32
    assert mref.edges_pair_up(triangles.cpu().numpy())
    assert mref.six_volumes(np.array(corners) - (n - 1), triangles.cpu().numpy()) == 6
    with pytest.raises(FfnError, match="not among the vertices"):
        ops.octree_mesh_faces(keys[:-1].contiguous(), masks[:-1].contiguous(), depth)


def test_a_tree_of_depth_22_is_refused_before_any_launch(monkeypatch):
    from fourier_feature_nets_amd import ops
    from fourier_feature_nets_amd.octree import OcTree
    nodes, leaves = grid_tree(22, [(21, 0, 0, 0)])
    tree = OcTree(1.0, nodes, leaves)
    assert tree.depth == 22 == ops.octree_mesh_max_depth() + 1

    def launched(*args, **kwargs):
        raise AssertionError("a kernel entry point was called: %r" % (args[:1],))
    monkeypatch.setattr(ops, "_call", launched)
    for placement in mref.PLACEMENTS:
        with pytest.raises(ValueError, match="deeper than the corner keys hold"):
            tree.extract_mesh(placement=placement)
