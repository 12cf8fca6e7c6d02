"""K21 without a GPU: the threshold policy ``refine_actions``, the numpy restatement of the rebuild
(tests/octree_refine_reference.py) on hand-made trees, the float64 invariance of the volume render
under a split that the GPU tests lean on, and the argument refusals that need no device."""

import numpy as np
import pytest

from tests import octree_refine_reference as rref
from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import grid_tree, lattice_rays, level_cells, mixed_tree
from tests.octree_sh_helpers import mixed_depth4
from tests.octree_volume_helpers import hand_case, random_leaf_data
from tests.octree_walk_helpers import two_level_tree


# ------------------------------------------------------------------------------- policy
def test_refine_actions_policy():
    from fourier_feature_nets import refine_actions
    # dyadic weights and thresholds: a float32 weight equals its threshold exactly
    lo, hi = 2.0 ** -6, 2.0 ** -3
    weights = np.float32([0.0, 2.0 ** -8, lo, 2.0 ** -4, hi, 0.5, 0.5, np.nan])
    depths = np.int32([3, 3, 3, 3, 3, 3, 10, 3])
    got = refine_actions(weights, depths, lo, hi)
    assert got.dtype == np.uint8 and got.shape == (8,)
    #                        < prune  < prune  == prune  between  == split  above  capped  NaN
    assert got.tolist() == [0, 0, 1, 1, 2, 2, 1, 1]
    # the defaults are 1e-2 and 1e-1
    assert refine_actions(np.float32([0.005, 0.02, 0.09, 0.11]), np.int32([1, 1, 1, 1])).tolist() \
        == [0, 1, 1, 2]
    # never split
    assert refine_actions(weights, depths, lo, None).tolist() == [0, 0, 1, 1, 1, 1, 1, 1]
    # prune_below == split_above: no leaf is only kept, but the depth cap and a NaN still keep
    mid = 2.0 ** -4
    assert refine_actions(weights, depths, mid, mid).tolist() == [0, 0, 0, 2, 2, 2, 1, 1]
    # the depth cap: a leaf at level max_depth - 1 stays
    assert refine_actions(weights, depths, lo, hi, max_depth=4).tolist() == \
        [0, 0, 1, 1, 1, 1, 1, 1]
    assert refine_actions(weights, depths, lo, hi, max_depth=5).tolist() == \
        [0, 0, 1, 1, 2, 2, 1, 1]
    # nothing pruned at 0: no weight is below it
    assert refine_actions(weights, depths, 0.0, None).tolist() == [1] * 8
    assert refine_actions(np.zeros(0), np.zeros(0, np.int32)).shape == (0,)


def test_refine_actions_refusals():
    from fourier_feature_nets import refine_actions
    weights, depths = np.float32([0.5, 0.0]), np.int32([1, 1])
    with pytest.raises(ValueError, match="prune_below"):
        refine_actions(weights, depths, 0.2, 0.1)
    with pytest.raises(ValueError, match="prune_below"):
        refine_actions(weights, depths, float("nan"), 0.1)
    with pytest.raises(ValueError, match="one entry per leaf"):
        refine_actions(weights, depths[:1])
    for bad in (0, 12):
        with pytest.raises(ValueError, match="max_depth"):
            refine_actions(weights, depths, max_depth=bad)


# ------------------------------------------------------------------------------- numpy refine
def test_numpy_refine_on_the_two_level_tree():
    _, nodes, leaves = two_level_tree()                     # nodes {0, 8}, leaves {1, 65, 72}
    rows = np.float32([[1, 2], [3, 4], [5, 6]])
    ids, new_nodes, new_rows, parent = rref.refine(leaves, rows, [1, 1, 1])
    assert np.array_equal(ids, leaves) and np.array_equal(new_nodes, nodes)
    assert np.array_equal(new_rows, rows) and parent.tolist() == [0, 1, 2]
    # split leaf 1 (node 1): children 9 .. 16; node 1 becomes interior
    ids, new_nodes, new_rows, parent = rref.refine(leaves, rows, [2, 1, 0])
    assert ids.tolist() == list(range(9, 17)) + [65]
    assert new_nodes.tolist() == [0, 1, 8]
    assert parent.tolist() == [0] * 8 + [1]
    assert np.array_equal(new_rows, rows[parent])
    # dropping both children of node 8 removes node 8
    ids, new_nodes, _, parent = rref.refine(leaves, None, [1, 0, 0])
    assert ids.tolist() == [1] and new_nodes.tolist() == [0] and parent.tolist() == [0]
    # split a deep leaf: ids 8 * 72 + 1 + k
    ids, new_nodes, _, parent = rref.refine(leaves, None, [0, 0, 2])
    assert ids.tolist() == [577 + k for k in range(8)] and new_nodes.tolist() == [0, 8, 72]
    assert parent.tolist() == [2] * 8


def test_numpy_refine_root_only():
    ids, nodes, rows, parent = rref.refine([0], np.float32([[7.0]]), [2])
    assert ids.tolist() == list(range(1, 9)) and nodes.tolist() == [0]
    assert rows.tolist() == [[7.0]] * 8 and parent.tolist() == [0] * 8
    ids, nodes, rows, parent = rref.refine([0], None, [1])
    assert ids.tolist() == [0] and len(nodes) == 0 and rows is None and parent.tolist() == [0]


def test_numpy_refine_on_mixed_depth4():
    _, nodes, leaves = mixed_depth4()
    rows = np.arange(len(leaves) * 3, dtype=np.float32).reshape(-1, 3)
    keep = np.ones(len(leaves), np.uint8)
    ids, new_nodes, new_rows, parent = rref.refine(leaves, rows, keep)
    assert np.array_equal(ids, leaves) and np.array_equal(new_nodes, nodes)
    assert np.array_equal(new_rows, rows) and np.array_equal(parent, np.arange(len(leaves)))
    action = np.random.default_rng(3).integers(0, 3, len(leaves)).astype(np.uint8)
    assert len(set(action.tolist())) == 3
    ids, new_nodes, new_rows, parent = rref.refine(leaves, rows, action)
    assert len(ids) == (action == 1).sum() + 8 * (action == 2).sum()
    assert (np.diff(ids) > 0).all() and (action[parent] != 0).all()
    split = action[parent] == 2
    assert np.array_equal((ids[split] - 1) >> 3, leaves[parent[split]])
    assert np.array_equal(ids[~split], leaves[parent[~split]])
    assert np.array_equal(new_rows, rows[parent])
    # the interior nodes are exactly the ancestors: every one has a child, none is a leaf
    assert not np.isin(new_nodes, ids).any()
    children = np.concatenate([ids, new_nodes[new_nodes > 0]])
    assert np.array_equal(np.unique((children - 1) >> 3), new_nodes)
    # dropping all eight children of one parent removes the parent
    level = rref.id_levels(leaves)
    parents, counts = np.unique((leaves[level == 3] - 1) >> 3, return_counts=True)
    victim = parents[0]
    gone = ((leaves - 1) >> 3) == victim
    action = np.where(gone, 0, 1).astype(np.uint8)
    ids, new_nodes, _, _ = rref.refine(leaves, rows, action)
    assert victim in nodes and victim not in new_nodes and victim not in ids


# ------------------------------------------------------------------------------- invariance
def split_all(nodes, leaves, data):
    ids, new_nodes, rows, _ = rref.refine(leaves, data, np.full(len(leaves), 2, np.uint8))
    return new_nodes, ids, rows


def lattice_cases():
    scale, nodes, leaves = mixed_tree()
    yield "mixed", scale, nodes, leaves, 5
    nodes, leaves = grid_tree(4, level_cells(3, np.random.default_rng(2), 200))
    yield "level-3 cells", np.float32(1.0), nodes, leaves, 4


def check_split_invariance(what, scale, nodes, leaves, data, starts, dirs, t_min, min_t):
    new_nodes, new_leaves, new_data = split_all(nodes, leaves, data)
    before = vref.composite(wref.walk(scale, nodes, leaves, starts, dirs), scale, starts, dirs,
                            data, t_min, (0.25, 0.5, 0.125), min_t)
    after = vref.composite(wref.walk(scale, new_nodes, new_leaves, starts, dirs), scale, starts,
                           dirs, new_data, t_min, (0.25, 0.5, 0.125), min_t)
    worst = 0.0
    for key in ("color", "alpha", "trans"):
        a, b = before[key], after[key]
        with np.errstate(invalid="ignore", divide="ignore"):
            rel = np.where(a == b, 0.0, np.abs(a - b) / np.abs(a))
        worst = max(worst, float(rel.max()))
        assert (rel <= 1e-12).all(), (what, key, rel.max())
    assert (after["count"] >= before["count"]).all() and after["count"].sum() > before["count"].sum()
    print("%s t_min=%g: %d rays, %d -> %d taken crossings, worst relative difference %.3g"
          % (what, t_min, len(starts), before["count"].sum(), after["count"].sum(), worst))


def test_split_invariance_on_the_hand_case():
    scale, nodes, leaves, data, starts, dirs = hand_case()
    for t_min in (0.0, 0.75):
        check_split_invariance("hand case", scale, nodes, leaves, data, starts, dirs, t_min, 0.0)


@pytest.mark.parametrize("t_min", [0.0, 0.75])
def test_split_invariance_on_lattice_rays(t_min):
    for what, scale, nodes, leaves, depth in lattice_cases():
        data = random_leaf_data(scale, leaves)
        data[:, 3] *= 8.0
        starts, dirs = lattice_rays(scale, depth, 400, 7)
        check_split_invariance(what, scale, nodes, leaves, data, starts, dirs, t_min, 0.0)


# ------------------------------------------------------------------------------- refusals
def test_refine_refusals_without_a_device():
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    tree = ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match=r"\(num_leaves,\) = \(3,\)"):
        tree.refine(np.ones(4, np.uint8))
    with pytest.raises(ValueError, match=r"\(num_leaves,\)"):
        tree.refine(np.ones((3, 1), np.uint8))
    with pytest.raises(ValueError, match="0 .drop., 1 .keep. or 2 .split."):
        tree.refine(np.uint8([1, 3, 1]))
    with pytest.raises(ValueError, match="0 .drop., 1 .keep. or 2 .split."):
        tree.refine(np.int64([1, -1, 1]))
    with pytest.raises(ValueError, match="integers"):
        tree.refine(np.float32([1, 1, 1]))
    with pytest.raises(ValueError, match="no leaf"):
        tree.refine(np.zeros(3, np.uint8))
    # a leaf at level octree_max_depth() - 1 = 10 cannot split
    deep = 0
    for _ in range(10):
        deep = 8 * deep + 1
    deep_tree = ffn.OcTree(1.0, rref.ancestors([deep]), [deep])
    assert deep_tree.depth == 11
    with pytest.raises(ValueError, match="limit of 11"):
        deep_tree.refine(np.uint8([2]))


def test_leaf_weights_refusals_without_a_device():
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    rays = np.zeros((2, 3), np.float32), np.ones((2, 3), np.float32)
    with pytest.raises(ValueError, match="no leaf_data"):
        ffn.OcTree(float(scale), nodes, leaves).leaf_weights(*rays)
    with pytest.raises(ValueError, match="C >= 4"):
        ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 3), np.float32)).leaf_weights(*rays)
    tree = ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 4), np.float32))
    for bad in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="min_transmittance"):
            tree.leaf_weights(*rays, min_transmittance=bad)
    with pytest.raises(ValueError, match="rounds"):
        ffn.fit_octree_adaptive(tree, None, rounds=-1)
    with pytest.raises(ValueError, match="prune_below"):
        ffn.fit_octree_adaptive(tree, None, rounds=1, prune_below=0.5, split_above=0.1)
    with pytest.raises(ValueError, match="pass center="):
        ffn.leaf_weights_over(tree, None)

    class Empty:
        class sampler:
            num_cameras, rays_per_camera, starts = 0, 16, np.zeros((0, 3), np.float32)
    with pytest.raises(ValueError, match="no rays"):
        ffn.leaf_weights_over(tree, Empty, center=(0, 0, 0))
