"""K20 without a GPU: the float64 / pure-Python restatement (tests/octree_tv_reference.py) against
known answers, and the argument refusals of the host wrappers that need no device."""

import numpy as np
import pytest

from tests import octree_tv_reference as tref
from tests.octree_lattice_helpers import cell_id, grid_tree, level_cells, mixed_tree
from tests.octree_sh_helpers import mixed_depth4
from tests.octree_walk_helpers import two_level_tree


@pytest.mark.parametrize("k", [1, 2, 3])
def test_full_grid_edge_count(k):
    nodes, leaves = grid_tree(k + 1, level_cells(k))
    nb, edge_list = tref.tree_edges(nodes, leaves)
    side = 1 << k
    assert len(edge_list) == 3 * 4 ** k * (side - 1)
    # an interior cell has six neighbours, a corner three; every neighbour relation is mutual
    assert (nb >= 0).sum() == 2 * len(edge_list)
    for i in range(len(nb)):
        for d in range(6):
            if nb[i, d] >= 0:
                assert nb[nb[i, d], d ^ 1] == i
    # the + x neighbour of cell (ix, iy, iz) is cell (ix + 1, iy, iz)
    number = {int(v): n for n, v in enumerate(leaves)}
    assert nb[number[cell_id(k, 0, 0, 0)], 1] == number[cell_id(k, 1, 0, 0)]
    assert nb[number[cell_id(k, 0, 0, 0)], 0] == -1


def test_root_only_tree_has_no_neighbours():
    nb, edge_list = tref.tree_edges(np.zeros(0, np.int64), np.array([0], np.int64))
    assert nb.shape == (1, 6) and (nb == -1).all() and len(edge_list) == 0
    out = tref.total_variation(np.ones((1, 4), np.float32), edge_list, np.ones(4), 0.01)
    assert out["value"] == 0.0 and not out["grad"].any()


def test_two_level_tree_by_listing():
    """Leaves 1 (octant ---), 65 and 72 (the --- and +++ corners of octant +++): leaf 1 touches
    octant +++ in a corner only, 65 and 72 are diagonal inside it: no faces at all; 65's -x, -y, -z
    neighbours are the empty octants, 72's + sides the cube's boundary."""
    _, nodes, leaves = two_level_tree()
    nb, edge_list = tref.tree_edges(nodes, leaves)
    assert (nb == -1).all() and len(edge_list) == 0
    assert tref.touching_pairs(leaves) == set()
    # with octant +-- (id 5) a leaf as well, leaf 1 touches it across +x and nothing else changes:
    # 65 lies at the --- corner of +++, whose -x, -y and -z sides face the empty -++, +-+ and ++-
    # octants
    nodes2, leaves2 = grid_tree(3, [(1, 0, 0, 0), (1, 1, 0, 0), (2, 2, 2, 2), (2, 3, 3, 3)])
    assert leaves2.tolist() == [1, 5, 65, 72]
    nb2, edges2 = tref.tree_edges(nodes2, leaves2)
    want = np.full((4, 6), -1)
    want[0, 1], want[1, 0] = 1, 0
    assert np.array_equal(nb2, want) and edges2.tolist() == [[0, 1]]
    # a fine leaf beside a coarse one: octant +-+ (id 6) is what 65 sees across its -y face
    nodes3, leaves3 = grid_tree(3, [(1, 1, 0, 1), (2, 2, 2, 2)])       # +-+ (id 6) and 65
    nb3, edges3 = tref.tree_edges(nodes3, leaves3)
    assert leaves3.tolist() == [6, 65]
    want = np.full((2, 6), -1)
    want[1, 2] = 0                      # 65's -y neighbour is the coarse leaf; the coarse side is -1
    assert np.array_equal(nb3, want) and edges3.tolist() == [[1, 0]]


def test_mixed_depth4_by_listing():
    """Every entry of the table re-derived from the leaves' boxes: the neighbour across a face is the
    one leaf whose box holds the cell on the other side, if it is of the leaf's size or larger."""
    _, nodes, leaves = mixed_depth4()
    nb, edge_list = tref.tree_edges(nodes, leaves)
    level = tref.levels(leaves)
    top = int(level.max())
    lo, hi = tref.boxes(leaves, top)
    assert set(level.tolist()) == {1, 2, 3}
    for i in range(len(leaves)):
        side = hi[i, 0] - lo[i, 0]
        for d, (axis, step) in enumerate(tref.DIRECTIONS):
            probe = lo[i].copy()                         # the - corner of the cell on the other side
            probe[axis] += step * side
            holder = np.nonzero(((lo <= probe) & (probe < hi)).all(1))[0]
            want = int(holder[0]) if len(holder) and hi[holder[0], 0] - lo[holder[0], 0] >= side else -1
            assert nb[i, d] == want, (i, d)
    pairs = [(min(a, b), max(a, b)) for a, b in edge_list.tolist()]
    assert len(set(pairs)) == len(pairs) and set(pairs) == tref.touching_pairs(leaves)
    assert len(pairs) > 20 and (level[edge_list[:, 0]] != level[edge_list[:, 1]]).any()


def test_every_touching_pair_of_a_random_mixed_tree_is_an_edge_once():
    _, nodes, leaves = mixed_tree()                     # depth 5: levels 2, 3, 4, empty regions
    _, edge_list = tref.tree_edges(nodes, leaves)
    pairs = [(min(a, b), max(a, b)) for a, b in edge_list.tolist()]
    assert len(set(pairs)) == len(pairs)
    assert set(pairs) == tref.touching_pairs(leaves)
    level = tref.levels(leaves)
    # the finer leaf holds a mixed edge, and an equal-level edge points in a + direction
    assert (level[edge_list[:, 0]] >= level[edge_list[:, 1]]).all()
    assert (level[edge_list[:, 0]] > level[edge_list[:, 1]]).any()


def test_skew_tree_hand_count():
    """Octant 0 a level-1 leaf, octants 4, 2, 1 (its +x, +y, +z neighbours) full level-3 grids: the
    hand count of the GPU test's level-5 case at a size brute force can check."""
    sub = 3
    side = 1 << (sub - 1)                                # cells per axis inside an octant
    codes = [(1, 0, 0, 0)]
    for ox, oy, oz in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        codes += [(sub, ox * side + x, oy * side + y, oz * side + z)
                  for x in range(side) for y in range(side) for z in range(side)]
    nodes, leaves = grid_tree(sub + 1, codes)
    _, edge_list = tref.tree_edges(nodes, leaves)
    inside = 3 * side * side * (side - 1)
    assert len(edge_list) == 3 * inside + 3 * side * side
    out = tref.total_variation(np.zeros((len(leaves), 4), np.float32), edge_list, np.ones(4), 0.1)
    assert out["incidences"][0] == 3 * side * side and leaves[0] == 1
    pairs = set((min(a, b), max(a, b)) for a, b in edge_list.tolist())
    assert pairs == tref.touching_pairs(leaves)


@pytest.mark.parametrize("eps", [1e-3, 1e-1])
def test_gradient_is_the_central_difference_of_the_energy(eps):
    _, nodes, leaves = mixed_depth4()
    _, edge_list = tref.tree_edges(nodes, leaves)
    rng = np.random.default_rng(5)
    rows = rng.normal(size=(len(leaves), 4)).astype(np.float32)
    lam = np.float32([1.0, 0.5, 0.0, 2.0])
    out = tref.total_variation(rows, edge_list, lam, eps)
    eps32 = float(np.float32(eps))
    base = rows.astype(np.float64)
    assert abs(out["value"] - tref.energy(base, edge_list, lam.astype(np.float64), eps32)) < 1e-14
    h = 1e-6
    for leaf, col in [(0, 0), (3, 1), (7, 2), (len(leaves) - 1, 3), (len(leaves) // 2, 0)]:
        up, down = base.copy(), base.copy()
        up[leaf, col] += h
        down[leaf, col] -= h
        numeric = (tref.energy(up, edge_list, lam.astype(np.float64), eps32)
                   - tref.energy(down, edge_list, lam.astype(np.float64), eps32)) / (2 * h)
        assert abs(numeric - out["grad"][leaf, col]) < 2e-8, (leaf, col)
    assert not out["grad"][:, 2].any() and not out["budget"][:, 2].any()
    # the sum of every column's gradient over the leaves is 0: + for i, - for j
    assert np.abs(out["grad"].sum(0)).max() < 1e-12
    assert (out["budget"][out["incidences"] > 0][:, [0, 1, 3]] > 0).all()
    assert out["budget"].max() < 1e-5                   # a few dozen steps of 2^-24 of O(1 / E) sums


def test_host_wrappers_refuse_without_a_gpu():
    import torch
    from fourier_feature_nets_amd import OcTree, ops
    assert ops.octree_tv_weights(None, 4).tolist() == [1, 1, 1, 1]
    assert ops.octree_tv_weights((2, 3), 4).tolist() == [2, 2, 2, 3]
    sh1 = ops.octree_tv_weights((1, 2, 3), 16, 1)
    assert sh1.tolist() == [3, 1, 2, 2, 2, 1, 2, 2, 2, 1, 2, 2, 2, 0, 0, 0]
    sh2 = ops.octree_tv_weights((1, 2, 3), 28, 2)
    assert sh2[0] == 3 and sh2[[1, 10, 19]].tolist() == [1, 1, 1] and sh2.sum() == 3 + 3 + 24 * 2
    for bad in [(1,), (1, 2, 3), (1, float("nan")), (-1, 1), (1, float("inf")), 5]:
        with pytest.raises(ValueError, match="weights"):
            ops.octree_tv_weights(bad, 4)
    with pytest.raises(ValueError, match="weights"):
        ops.octree_tv_weights((1, 1), 28, 2)
    with pytest.raises(ValueError, match="stride"):
        ops.octree_tv_weights((1, 1, 1), 12, 1)
    for bad in [0.0, -1.0, float("nan"), float("inf")]:
        with pytest.raises(ValueError, match="eps"):
            ops.octree_tv_check_eps(bad)
    with pytest.raises(TypeError, match="plan"):
        ops.octree_tv(torch.zeros((2, 4)), None, np.ones(4, np.float32), 0.01)
    with pytest.raises(ValueError, match="neighbors"):
        ops.octree_tv_plan(torch.zeros((3, 5), dtype=torch.int32), torch.zeros(3, dtype=torch.int64))
    _, nodes, leaves = two_level_tree()
    bare = OcTree(1.0, nodes, leaves)
    with pytest.raises(ValueError, match="leaf_data"):
        bare.total_variation()
    with pytest.raises(ValueError, match="eps"):
        OcTree(1.0, nodes, leaves, np.zeros((3, 4), np.float32)).total_variation(eps=0)
    with pytest.raises(ValueError, match="weights"):
        OcTree(1.0, nodes, leaves, np.zeros((3, 4), np.float32)).total_variation((1, 2, 3))


def test_build_and_abi_list_the_new_file():
    from fourier_feature_nets_amd import _lib, build
    assert build.SOURCES["octree_tv.hip"] == ["-ffp-contract=off"]
    names = _lib.declared_symbols()
    for name in ("ffn_octree_neighbors", "ffn_octree_tv_workspace_bytes", "ffn_octree_tv"):
        assert name in names
    # refused before any launch (no device is touched: the checks come first)
    import ctypes
    lib = _lib.load()
    lib.ffn_octree_tv_workspace_bytes.restype = ctypes.c_int64
    size = lib.ffn_octree_tv_workspace_bytes
    assert size(ctypes.c_int64(10), ctypes.c_int64(20), ctypes.c_int(4)) > 0
    assert size(ctypes.c_int64(10), ctypes.c_int64(61), ctypes.c_int(4)) == -1      # E > 6 L
    assert size(ctypes.c_int64(10), ctypes.c_int64(20), ctypes.c_int(6)) == -1      # stride % 4
    assert size(ctypes.c_int64(1 << 30), ctypes.c_int64(1 << 30), ctypes.c_int(4)) == -1   # 2 E
    fake = ctypes.c_void_p(4096)                       # aligned, never dereferenced
    odd = ctypes.c_void_p(4100)
    lam = (ctypes.c_float * 4)(1, 1, 1, 1)
    nan = (ctypes.c_float * 4)(1, float("nan"), 1, 1)
    neg = (ctypes.c_float * 4)(1, 1, -1, 1)

    def tv(rows=fake, stride=4, weights=lam, eps=0.01, value=fake, d_rows=fake, accumulate=0):
        lib.ffn_octree_tv.restype = ctypes.c_int
        return lib.ffn_octree_tv(rows, ctypes.c_int64(10), ctypes.c_int(stride), fake, fake,
                                 ctypes.c_int64(20), fake, fake, fake, fake, fake,
                                 ctypes.c_int64(6), weights, ctypes.c_float(eps), value, d_rows,
                                 ctypes.c_int(accumulate), fake, ctypes.c_int64(0), None)

    for kwargs in (dict(stride=6), dict(rows=odd), dict(d_rows=odd), dict(eps=0.0), dict(eps=-1.0),
                   dict(eps=float("nan")), dict(weights=nan), dict(weights=neg), dict(rows=None),
                   dict(value=None), dict(d_rows=None, accumulate=1), dict()):   # (): no workspace
        assert tv(**kwargs) != 0, kwargs
        assert b"ffn_octree_tv" in lib.ffn_last_error_string()
