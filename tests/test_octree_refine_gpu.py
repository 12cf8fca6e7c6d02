"""K21 on the GPU: the per-leaf maximum weight (``OcTree.leaf_weights``, K21a) against its float64
restatement and bit for bit under reordering and folding; the rebuild from a per-leaf decision
(``ops.octree_refine`` / ``OcTree.refine``, K21b) against the numpy restatement
(tests/octree_refine_reference.py); what the refined tree is worth as a tree; and the driver
``fit_octree_adaptive`` with ``scripts/train_octree.py --refine-rounds``.

The tolerance of K21a is derived in tests/octree_refine_reference.py: per leaf the largest alpha
budget of the rays that take it.  Camera-like rays are first thinned to those whose margin exceeds
the per-ray budget of the K13 tests (``ray_budget``; at most 2 % are left out -- asserted), so that
the kernel and the restatement see the same leaves; lattice rays are exact in f32 and all stay.
For every K21a case the restatement itself must give at least half of the leaves a non-zero
weight -- asserted -- so a kernel that writes nothing cannot pass."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_refine_reference as rref
from tests import octree_sh_reference as shref
from tests import octree_tv_reference as tvref
from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import grid_tree, lattice_rays, level_cells, mixed_tree
from tests.octree_render_helpers import (LEFT_OUT_CAP, SCENE, TREES as GOLDEN_TREES, camera_rays,
                                         golden_rays, load_tree, ray_budget)
from tests.octree_sh_helpers import eight_leaves, mixed_depth4, sh_leaf_data
from tests.octree_volume_helpers import hand_case, random_leaf_data
from tests.octree_walk_helpers import opaque_ball, two_level_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MINS = [0.0, float(np.float32(0.7))]
WALK_BLOCK = 64                       # kWalkThreads of csrc/octree_walk.hip
SCAN_TILE = 2048                      # kScanTile of csrc/octree.hip
SEEN_SHARE = 0.5
# leaf counts around the tile of the scan over 8 slots per leaf (256 leaves), around the tile itself,
# and several tiles
LEAF_COUNTS = [1, 7, 255, 256, 257, 2047, 2048, 2049, 5000]
BG = (0.25, 0.5, 0.125)


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def sure_rays(scale, nodes, leaves, starts, dirs):
    """The rays whose margin exceeds ``ray_budget`` (or that miss), and their walk."""
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    ok = ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts, dirs))
    assert 1.0 - ok.mean() <= LEFT_OUT_CAP
    starts, dirs = starts[ok], dirs[ok]
    return starts, dirs, wref.walk(scale, nodes, leaves, starts, dirs)


def expected_weights(what, scale, leaves, data, starts, dirs, w, t_min=0.0, min_t=0.0):
    """The restatement's weights, budget and taken mask for plain rows ``data``; asserts the share
    of leaves it gives a non-zero weight."""
    want, budget, taken, _ = rref.leaf_max_weights(w, scale, starts, dirs, data, len(leaves), t_min,
                                                   min_t)
    share = (want > 0).mean()
    print("%s t_min=%.2f min_T=%.2f: %d rays, %d leaves, %.3f of them with a weight > 0, %.3f "
          "taken by some ray" % (what, t_min, min_t, len(starts), len(leaves), share, taken.mean()))
    assert share >= SEEN_SHARE
    return want, budget, taken


def check_weights(what, got, want, budget, taken):
    assert got.dtype == np.float32 and got.shape == want.shape
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(invalid="ignore", divide="ignore"):
        print("   %s: worst error / budget %.3f" % (what, np.nanmax(np.where(taken, err / budget, 0))))
    assert (err <= budget).all()
    assert (bits(got[~taken]) == 0).all()                 # +0.0f exactly
    assert (got >= 0).all() and (got <= 1).all()


# ------------------------------------------------------------------------------- K21a
def test_leaf_weights_hand_case():
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs = hand_case()
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    got = tree.leaf_weights(starts, dirs)
    assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (3,)
    # leaf 2 is opaque and ray 4 meets it first: T a = 1 exactly.  Leaf 0 (density 2): ray 0 crosses
    # a world length of 1, the diagonal sqrt 3, and the diagonal wins; leaf 1 (density 3): ray 1
    # crosses 0.5 with T = 1, the diagonal 0.5 sqrt 3 with what leaf 0 left.  Ray 2 meets nothing.
    step = 8 * 4 * 2.0 ** -24                     # the rounding term of the budget, n + 1 <= 4
    assert got[2] == 1.0
    assert abs(got[0] - (1 - np.exp(-2 * np.sqrt(3.0)))) <= step
    assert abs(got[1] - (1 - np.exp(-1.5))) <= step
    # a tie: the same ray twice, and rays 0 and 1 alone, give what they give apart
    twice = tree.leaf_weights(np.concatenate([starts, starts]), np.concatenate([dirs, dirs]))
    assert np.array_equal(bits(twice), bits(got))
    apart = tree.leaf_weights(starts[:2], dirs[:2])
    assert abs(apart[0] - (1 - np.exp(-2.0))) <= step and bits(apart[1]) == bits(got[1])
    assert bits(apart[2]) == 0
    # the miss alone: nothing
    assert (bits(tree.leaf_weights(starts[2:3], dirs[2:3])) == 0).all()
    # t_min inside leaf 0 on ray 0 (t 0.5 .. 1, |d| = 2): the chord from t_min on
    t_min = 0.75
    inside = tree.leaf_weights(starts[:1], dirs[:1], t_min=t_min)
    assert abs(inside[0] - (1 - np.exp(-2 * 0.25 * 2))) <= step and (bits(inside[1:]) == 0).all()
    # behind the cut: on the diagonal leaf 0 leaves T = exp(-2 sqrt 3) < 0.5
    cut = tree.leaf_weights(starts[3:4], dirs[3:4], min_transmittance=0.5)
    assert bits(cut[0]) == bits(got[0]) and (bits(cut[1:]) == 0).all()
    whole = tree.leaf_weights(starts[3:4], dirs[3:4])
    assert (whole[1:] > 0).all()


@functools.lru_cache(maxsize=None)
def golden_case(name):
    starts, dirs = golden_rays(name)
    state = load_tree(name).state_dict
    scale, nodes, leaves = state["scale"], state["node_index"], state["leaf_index"]
    data = random_leaf_data(scale, leaves)
    starts, dirs, w = sure_rays(scale, nodes, leaves, starts, dirs)
    return load_tree(name, data), scale, leaves, data, starts, dirs, w


@pytest.mark.parametrize("min_t", [0.0, 0.5])
@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", GOLDEN_TREES)
def test_leaf_weights_on_the_golden_trees(name, t_min, min_t):
    tree, scale, leaves, data, starts, dirs, w = golden_case(name)
    want, budget, taken = expected_weights(name, scale, leaves, data, starts, dirs, w, t_min, min_t)
    check_weights(name, tree.leaf_weights(starts, dirs, t_min, min_t), want, budget, taken)


@functools.lru_cache(maxsize=None)
def mixed_case():
    """``mixed_depth4`` with 1000 camera rays and densities eight times those of the K15 cases."""
    scale, nodes, leaves = mixed_depth4()
    data = random_leaf_data(scale, leaves)
    data[:, 3] *= np.float32(8.0)
    starts, dirs = camera_rays(np.random.default_rng(21), 1000, scale)
    starts, dirs, w = sure_rays(scale, nodes, leaves, starts, dirs)
    return scale, nodes, leaves, data, starts, dirs, w


@pytest.mark.parametrize("min_t", [0.0, 0.5])
def test_leaf_weights_do_not_depend_on_the_row_layout(min_t):
    """Plain rows of stride 4 and 6 and the SH device rows of stride 16 and 28, the same densities:
    the same bits, and within the budget of the restatement."""
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs, w = mixed_case()
    want, budget, taken = expected_weights("mixed4", scale, leaves, data, starts, dirs, w, 0.0, min_t)
    got = ffn.OcTree(float(scale), nodes, leaves, data).leaf_weights(starts, dirs, 0.0, min_t)
    check_weights("stride 4", got, want, budget, taken)
    if min_t > 0:
        whole = ffn.OcTree(float(scale), nodes, leaves, data).leaf_weights(starts, dirs)
        assert (got <= whole).all()
    wide = np.concatenate([data, np.full((len(data), 2), 7.0, np.float32)], 1)
    assert np.array_equal(bits(ffn.OcTree(float(scale), nodes, leaves, wide)
                               .leaf_weights(starts, dirs, 0.0, min_t)), bits(got))
    for degree, stride in ((1, 16), (2, 28)):
        rows = sh_leaf_data(scale, leaves, degree)
        rows[:, -1] = data[:, 3]
        tree = ffn.OcTree(float(scale), nodes, leaves, rows, degree)
        assert tree._sh_rows_on_device().shape[1] == stride
        assert np.array_equal(bits(tree.leaf_weights(starts, dirs, 0.0, min_t)), bits(got))


def test_leaf_weights_behind_the_cut():
    """Eight leaves, rays along +x only: the four leaves in front leave T = exp(-1) <= 0.5, so with
    that cut the four behind weigh exactly nothing, and without it exp(-1) (1 - exp(-1))."""
    import fourier_feature_nets as ffn
    scale, nodes, leaves = eight_leaves()
    data = random_leaf_data(scale, leaves)
    data[:, 3] = 1.0
    side = np.float32([-0.75, -0.5, -0.25, 0.25, 0.5, 0.75])
    y, z = [g.ravel() for g in np.meshgrid(side, side)]
    starts = np.stack([np.full(len(y), -2, np.float32), y, z], 1)
    dirs = np.tile(np.float32([[1, 0, 0]]), (len(y), 1))
    front = ((leaves - 1) & 4) == 0                     # child index 4 bx + 2 by + bz
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    for min_t in (0.0, 0.5):
        want, budget, taken = expected_weights("behind the cut", scale, leaves, data, starts, dirs,
                                               w, 0.0, min_t)
        got = tree.leaf_weights(starts, dirs, 0.0, min_t)
        check_weights("behind the cut", got, want, budget, taken)
        assert (got[front] > 0.6).all()
        if min_t > 0:
            assert (bits(got[~front]) == 0).all() and not taken[~front].any()
        else:
            assert (np.abs(got[~front] - np.exp(-1.0) * (1 - np.exp(-1.0))) < 1e-6).all()


def test_leaf_weights_of_dead_densities_and_dead_rays():
    """A quarter of the leaves with a negative, -0, or NaN density weigh nothing and hide nothing;
    NaN rays, rays without a direction and rays that pass by change nothing."""
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs, w = mixed_case()
    data = data.copy()
    dead = np.arange(len(leaves)) % 4 == 1
    data[dead, 3] = np.resize(np.float32([-1.5, np.nan, -0.0, -np.inf]), int(dead.sum()))
    want, budget, taken = expected_weights("dead densities", scale, leaves, data, starts, dirs, w)
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    got = tree.leaf_weights(starts, dirs)
    check_weights("dead densities", got, want, budget, taken)
    assert (bits(got[dead]) == 0).all() and taken[dead].any()
    bad_o = np.float32([[np.nan, 0, 0], [0, 0, 0], [0.1, 0.1, 0.1], [9, 9, 9], [0, 0, -3]])
    bad_d = np.float32([[0, 0, 1], [np.nan, 1, 0], [0, 0, 0], [0, 0, 1], [1, 0, 0]])
    more = tree.leaf_weights(np.concatenate([bad_o, starts, bad_o]),
                             np.concatenate([bad_d, dirs, bad_d]))
    assert np.array_equal(bits(more), bits(got))
    assert (bits(tree.leaf_weights(bad_o, bad_d)) == 0).all()


@pytest.mark.parametrize("n", [1, WALK_BLOCK - 1, WALK_BLOCK, WALK_BLOCK + 1])
def test_leaf_weights_ray_counts(n):
    """The two-level tree: ray 0 is the diagonal through all three leaves, the rest lattice rays
    (exact in f32: every ray counts)."""
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    data = np.float32([[0.25, 0.5, 0.75, 0.5], [1.0, 0.5, 0.0, 3.0], [0.5, 0.25, 1.0, 2.0]])
    starts, dirs = lattice_rays(scale, 3, n, 5 + n)
    starts[0], dirs[0] = (-2, -2, -2), (1, 1, 1)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    want, budget, taken = expected_weights("n = %d" % n, scale, leaves, data, starts, dirs, w)
    got = ffn.OcTree(float(scale), nodes, leaves, data).leaf_weights(starts, dirs)
    check_weights("n = %d" % n, got, want, budget, taken)
    assert (got > 0).all()


def test_leaf_weights_root_only_every_lane_on_one_address():
    import fourier_feature_nets as ffn
    scale = np.float32(1.0)
    nodes, leaves = np.zeros(0, np.int64), np.zeros(1, np.int64)
    data = np.float32([[0.5, 0.5, 0.5, 0.75]])
    starts, dirs = camera_rays(np.random.default_rng(8), 4096, scale)
    starts, dirs, w = sure_rays(scale, nodes, leaves, starts, dirs)
    assert len(starts) > 4000
    want, budget, taken = expected_weights("root only", scale, leaves, data, starts, dirs, w)
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    got = tree.leaf_weights(starts, dirs)
    check_weights("root only", got, want, budget, taken)
    # the heaviest ray alone gives the same bits: the maximum is one ray's weight, not a blend
    v = vref.composite(w, scale, starts, dirs, data)
    order = np.argsort(-v["alpha"])
    top = order[:8]
    assert bits(tree.leaf_weights(starts[top], dirs[top]))[0] == bits(got)[0]


def test_leaf_weights_bits_do_not_depend_on_order_or_folding():
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs, _ = mixed_case()
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    dev_o, dev_d = cuda(starts), cuda(dirs)
    first = tree.leaf_weights(dev_o, dev_d, 0.0, 0.25)
    assert torch.is_tensor(first) and first.dtype == torch.float32 and first.is_cuda
    want = bits(first.cpu().numpy())
    assert (want != 0).mean() >= SEEN_SHARE
    again = tree.leaf_weights(dev_o, dev_d, 0.0, 0.25)
    assert again.data_ptr() != first.data_ptr() and np.array_equal(bits(again.cpu().numpy()), want)
    order = torch.from_numpy(np.random.default_rng(2).permutation(len(starts))).cuda()
    mixed = tree.leaf_weights(dev_o[order].contiguous(), dev_d[order].contiguous(), 0.0, 0.25)
    assert np.array_equal(bits(mixed.cpu().numpy()), want)
    half = len(starts) // 2 + 17
    out = tree.leaf_weights(dev_o[half:].contiguous(), dev_d[half:].contiguous(), 0.0, 0.25)
    part = bits(out.cpu().numpy())
    folded = tree.leaf_weights(dev_o[:half].contiguous(), dev_d[:half].contiguous(), 0.0, 0.25, out)
    assert folded.data_ptr() == out.data_ptr()
    assert np.array_equal(bits(folded.cpu().numpy()), want) and not np.array_equal(part, want)
    # folding the same rays once more changes nothing
    tree.leaf_weights(dev_o, dev_d, 0.0, 0.25, out)
    assert np.array_equal(bits(out.cpu().numpy()), want)
    # numpy rays give numpy weights with the same bits
    assert np.array_equal(bits(tree.leaf_weights(starts, dirs, 0.0, 0.25)), want)
    with pytest.raises(ValueError, match="out must be"):
        tree.leaf_weights(dev_o, dev_d, out=torch.zeros(len(leaves) + 1, device="cuda"))


# ------------------------------------------------------------------------------- K21b
@functools.lru_cache(maxsize=None)
def leaf_pool():
    """Sorted ids of a valid leaf set with leaves at levels 3 .. 5 (any subset of it is valid)."""
    rng = np.random.default_rng(12)
    _, leaves = grid_tree(4, level_cells(3))
    for _ in range(2):
        action = rng.choice(np.uint8([1, 2]), len(leaves), p=[0.6, 0.4])
        leaves = rref.refine(leaves, None, action)[0]
    assert len(leaves) > max(LEAF_COUNTS) and set(rref.id_levels(leaves).tolist()) == {3, 4, 5}
    return leaves


def random_rows(count, channels, seed):
    """Any bit pattern, NaN payloads and denormals included: the rows travel bit for bit."""
    raw = np.random.default_rng(seed).integers(0, 1 << 32, (count, channels), dtype=np.uint64)
    return raw.astype(np.uint32).view(np.float32)


def check_refine(leaves, rows, action, depth):
    from fourier_feature_nets_amd import ops
    got = ops.octree_refine(cuda(leaves, np.int64), None if rows is None else cuda(rows),
                            cuda(action, np.uint8), depth)
    ids, nodes, new_rows, parent = rref.refine(leaves, rows, action)
    assert got[0].dtype == torch.int64 and got[1].dtype == torch.int64 and got[3].dtype == torch.int64
    assert np.array_equal(got[0].cpu().numpy(), ids)
    assert np.array_equal(got[1].cpu().numpy(), nodes)
    assert np.array_equal(got[3].cpu().numpy(), parent)
    if rows is None:
        assert got[2] is None
    else:
        assert got[2].dtype == torch.float32 and got[2].shape == new_rows.shape
        assert np.array_equal(bits(got[2].cpu().numpy()), bits(new_rows))
    return ids


@pytest.mark.parametrize("count", LEAF_COUNTS)
def test_refine_against_numpy_at_the_scan_edges(count):
    rng = np.random.default_rng(count)
    leaves = np.sort(rng.choice(leaf_pool(), count, replace=False))
    depth = int(rref.id_levels(leaves).max()) + 1
    rows = random_rows(count, 4, count)
    mixes = {"every mix": rng.integers(0, 3, count), "keep all": np.ones(count),
             "split all": np.full(count, 2), "mostly drop": (rng.random(count) < 0.1) * 1,
             "all but one dropped": np.arange(count) == count // 2}
    for what, action in mixes.items():
        action = action.astype(np.uint8)
        if not action.any():
            action[0] = 2
        ids = check_refine(leaves, rows, action, depth)
        print("%d leaves, %s: %d new leaves" % (count, what, len(ids)))
    # the new leaf count on both sides of a scan tile: s splits and d drops with 7 s - d = target -
    # count, where the leaves allow it
    for target in (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1):
        splits = max(0, -((count - target) // 7))
        drops = count + 7 * splits - target
        if splits + drops > count or drops == count:
            continue
        action = np.ones(count, np.uint8)
        action[:splits] = 2
        action[count - drops:] = 0
        assert len(check_refine(leaves, rows, action, depth)) == target


@pytest.mark.parametrize("channels", [1, 4, 13, 16, 28])
def test_refine_row_strides(channels):
    rng = np.random.default_rng(channels)
    leaves = np.sort(rng.choice(leaf_pool(), 700, replace=False))
    depth = int(rref.id_levels(leaves).max()) + 1
    action = rng.integers(0, 3, len(leaves)).astype(np.uint8)
    check_refine(leaves, random_rows(len(leaves), channels, channels), action, depth)


def test_refine_small_trees_and_no_rows():
    import fourier_feature_nets as ffn
    ids = check_refine(np.int64([0]), random_rows(1, 4, 1), np.uint8([2]), 1)
    assert ids.tolist() == list(range(1, 9))
    check_refine(np.int64([0]), None, np.uint8([1]), 1)
    _, nodes, leaves = two_level_tree()
    for action in ([1, 1, 1], [2, 1, 0], [1, 0, 0], [0, 0, 2], [2, 2, 2]):
        check_refine(leaves, None, np.uint8(action), 3)
        check_refine(leaves, random_rows(3, 13, 4), np.uint8(action), 3)
    # the root-only tree through the class: eight leaves under node 0
    root = ffn.OcTree(2.0, [], [0], np.float32([[1, 2, 3, 4]]))
    root._center = (1.0, 2.0, 3.0)
    new, parent = root.refine([2])
    assert new.state_dict["leaf_index"].tolist() == list(range(1, 9))
    assert new.state_dict["node_index"].tolist() == [0] and parent.tolist() == [0] * 8
    assert parent.dtype == np.int64 and new.scale == 2.0 and new.center == (1.0, 2.0, 3.0)
    assert np.array_equal(new.leaf_data(), np.repeat(root.leaf_data(), 8, 0))
    assert new._cache == {} and new.sh_degree is None
    # no leaf_data
    bare = ffn.OcTree(1.0, nodes, leaves)
    new, parent = bare.refine(np.uint8([2, 1, 0]))
    assert new.leaf_data() is None and parent.tolist() == [0] * 8 + [1]
    assert new.state_dict["leaf_index"].tolist() == list(range(9, 17)) + [65]
    # float64 rows (a file of the reference) are carried by the parent map
    wide = ffn.OcTree(1.0, nodes, leaves, np.float64([[1, 2], [3, 4], [5, 6]]))
    new, parent = wide.refine([1, 2, 1])
    assert new.leaf_data().dtype == np.float64
    assert np.array_equal(new.leaf_data(), wide.leaf_data()[parent])


@pytest.mark.parametrize("degree", [None, 1, 2])
def test_refine_through_the_class(degree):
    import fourier_feature_nets as ffn
    scale, nodes, leaves = mixed_depth4()
    data = random_leaf_data(scale, leaves) if degree is None else sh_leaf_data(scale, leaves, degree)
    tree = ffn.OcTree(float(scale), nodes, leaves, data, degree)
    same, parent = tree.refine(np.ones(len(leaves), np.uint8))
    assert np.array_equal(same.state_dict["node_index"], nodes)
    assert np.array_equal(same.state_dict["leaf_index"], leaves)
    assert np.array_equal(bits(same.leaf_data()), bits(data)) and same.sh_degree == degree
    assert np.array_equal(parent, np.arange(len(leaves))) and same is not tree
    action = np.random.default_rng(6).integers(0, 3, len(leaves)).astype(np.uint8)
    new, parent = tree.refine(action)
    ids, new_nodes, rows, want_parent = rref.refine(leaves, data, action)
    assert np.array_equal(new.state_dict["leaf_index"], ids)
    assert np.array_equal(new.state_dict["node_index"], new_nodes)
    assert np.array_equal(bits(new.leaf_data()), bits(rows)) and np.array_equal(parent, want_parent)
    assert new.sh_degree == degree and new.depth == 5 and new.scale == tree.scale
    # this tree is as it was
    assert np.array_equal(tree.state_dict["leaf_index"], leaves)
    assert np.array_equal(bits(tree.leaf_data()), bits(data))


def test_refine_refusals():
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    _, nodes, leaves = two_level_tree()
    ids = cuda(leaves, np.int64)
    rows = cuda(np.zeros((3, 4)))

    def act(values):
        return cuda(values, np.uint8)
    with pytest.raises(ValueError, match=r"\(num_leaves,\) = \(3,\)"):
        ops.octree_refine(ids, rows, act([1, 1]), 3)
    with pytest.raises(ValueError, match=r"\(num_leaves,\) = \(3,\)"):
        ops.octree_refine(ids, rows, act([1, 1, 1, 1]), 3)
    with pytest.raises(ValueError, match="0 .drop., 1 .keep. or 2 .split., got 3"):
        ops.octree_refine(ids, rows, act([1, 3, 1]), 3)
    with pytest.raises(ValueError, match="no leaf"):
        ops.octree_refine(ids, rows, act([0, 0, 0]), 3)
    with pytest.raises(ValueError, match="rows must be"):
        ops.octree_refine(ids, cuda(np.zeros((2, 4))), act([1, 1, 1]), 3)
    with pytest.raises(ValueError, match="depth"):
        ops.octree_refine(ids, rows, act([1, 1, 1]), 12)
    with pytest.raises(ValueError, match="level 2 in a tree of depth 2"):
        ops.octree_refine(ids, rows, act([1, 1, 1]), 2)
    # a leaf at level octree_max_depth() - 1 = 10: kept it stays, split it would be level 11
    assert ops.octree_max_depth() == 11
    deep = 0
    for _ in range(10):
        deep = 8 * deep + 8
    both = cuda([1, deep], np.int64)
    out = ops.octree_refine(both, None, act([2, 1]), 11)
    assert out[0].cpu().tolist() == list(range(9, 17)) + [deep]
    with pytest.raises(ValueError, match="limit of 11"):
        ops.octree_refine(both, None, act([1, 2]), 11)
    deep_tree = ffn.OcTree(1.0, rref.ancestors([1, deep]), [1, deep])
    with pytest.raises(ValueError, match="limit of 11"):
        deep_tree.refine([1, 2])
    # 2^28 leaves could become 2^31: refused on the shapes alone, nothing is read
    many = 1 << 28
    with pytest.raises(ValueError, match="at or over the limit of 2.31"):
        ops.octree_refine(torch.empty((many,), dtype=torch.int64, device="cuda"), None,
                          torch.empty((many,), dtype=torch.uint8, device="cuda"), 11)


# ------------------------------------------------------------------------------- the tree
def test_the_refined_tree_is_a_tree():
    import fourier_feature_nets as ffn
    scale, nodes, leaves = mixed_tree()                       # depth 5, scale 2
    data = random_leaf_data(scale, leaves)
    action = np.random.default_rng(31).integers(0, 3, len(leaves)).astype(np.uint8)
    tree, parent = ffn.OcTree(float(scale), nodes, leaves, data).refine(action)
    state = tree.state_dict
    new_nodes, new_leaves = state["node_index"], state["leaf_index"]
    assert tree.depth == 6 and tree.num_leaves == len(parent)
    assert np.array_equal(new_nodes, rref.ancestors(new_leaves))
    # every new leaf's centre lies in that leaf
    assert np.array_equal(tree.query(tree.leaf_centers()), np.arange(tree.num_leaves))
    assert np.array_equal(tree.leaf_depths(), rref.id_levels(new_leaves))
    # and where it came from: the centre of a new leaf lies in its parent leaf of the old tree
    old = ffn.OcTree(float(scale), nodes, leaves)
    assert np.array_equal(old.query(tree.leaf_centers()), parent)
    assert np.array_equal(tree.neighbors(), tvref.neighbors(new_nodes, new_leaves))
    # the walk, on rays without a tie
    starts, dirs = camera_rays(np.random.default_rng(4), 600, scale)
    w = wref.walk(scale, new_nodes, new_leaves, starts, dirs)
    budget = ray_budget(w, scale, starts, dirs)
    ok = ~w["hit"] | (w["margin"] > budget)
    assert 1.0 - ok.mean() <= LEFT_OUT_CAP
    length = int(np.diff(w["offsets"]).max()) + 2
    want_t, want_leaves, written = wref.path(w, length)
    path = tree.walk(starts, dirs, length)
    assert np.array_equal(path.leaves[ok], want_leaves[ok])
    live = ok & w["hit"]
    err = np.abs(path.t_stops.astype(np.float64) - want_t)
    assert (err[live] <= budget[live][:, None]).all()
    assert (path.leaves[live] >= 0).any()


@pytest.mark.parametrize("degree", [None, 2])
def test_render_after_a_full_split(degree):
    """Every leaf split, rows copied: ``render_volume`` of the split tree within the budgets the
    restatement computes ON THE SPLIT TREE (and so, by the float64 invariance of
    tests/test_octree_refine_cpu.py, next to the render of the tree before)."""
    import fourier_feature_nets as ffn
    scale, nodes, leaves = mixed_depth4()
    data = random_leaf_data(scale, leaves) if degree is None else sh_leaf_data(scale, leaves, degree)
    if degree is None:
        data[:, 3] *= np.float32(8.0)
    before = ffn.OcTree(float(scale), nodes, leaves, data, degree)
    tree, parent = before.refine(np.full(len(leaves), 2, np.uint8))
    assert tree.num_leaves == 8 * len(leaves) and tree.depth == 5
    state = tree.state_dict
    starts, dirs = camera_rays(np.random.default_rng(17), 1000, scale)
    starts, dirs, w = sure_rays(scale, state["node_index"], state["leaf_index"], starts, dirs)
    got = tree.render_volume(starts, dirs, 0.0, BG)
    if degree is None:
        v = vref.composite(w, scale, starts, dirs, tree.leaf_data(), 0.0, BG)
    else:
        v = shref.composite(w, scale, starts, dirs, tree.leaf_data(), degree, 0.0, BG)
    err_c = np.abs(got.color.astype(np.float64) - v["color"]).max(1)
    err_a = np.abs(got.alpha.astype(np.float64) - v["alpha"])
    took = v["count"] > 0
    print("full split, degree %s: %d rays, %d take a leaf; worst error / budget: colour %.3f alpha "
          "%.3f" % (degree, len(starts), took.sum(), (err_c / v["budget_c"]).max(),
                    (err_a / v["budget_a"]).max()))
    assert took.mean() > 0.5
    assert (err_c <= v["budget_c"]).all() and (err_a <= v["budget_a"]).all()
    # and the render before the split differs from it by no more than the two budgets together
    w0 = wref.walk(scale, nodes, leaves, starts, dirs)
    if degree is None:
        v0 = vref.composite(w0, scale, starts, dirs, data, 0.0, BG)
    else:
        v0 = shref.composite(w0, scale, starts, dirs, data, degree, 0.0, BG)
    sure = ~w0["hit"] | (w0["margin"] > ray_budget(w0, scale, starts, dirs))
    old = before.render_volume(starts, dirs, 0.0, BG)
    gap_a = np.abs(old.alpha.astype(np.float64) - got.alpha)
    assert (gap_a <= v["budget_a"] + v0["budget_a"] + 1e-12)[sure].all()


@functools.lru_cache(maxsize=None)
def unseen_case():
    """A lattice tree at scale 1 (200 of the 512 level-3 cells), colours finite, three leaves in ten
    without density, one in ten opaque, and lattice rays: -> scale, nodes, leaves, data, rays."""
    scale = np.float32(1.0)
    nodes, leaves = grid_tree(4, level_cells(3, np.random.default_rng(2), 200))
    data = random_leaf_data(scale, leaves)
    data[:, 3] *= np.float32(8.0)
    kind = np.random.default_rng(3).random(len(leaves))
    data[kind < 0.3, 3] = 0.0
    data[kind > 0.9, 3] = 1e30
    starts, dirs = lattice_rays(scale, 4, 300, 19)
    return scale, nodes, leaves, data, starts, dirs


def test_pruning_what_nothing_sees_changes_nothing():
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs = unseen_case()
    assert np.isfinite(data[:, :3]).all() and (data[:, 3] == 0).sum() >= 3
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    weights = tree.leaf_weights(starts, dirs)
    # the restatement agrees on which leaves weigh nothing: every plane crossing is exact
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    want, _, _, v = rref.leaf_max_weights(w, scale, starts, dirs, data, len(leaves))
    assert np.array_equal(weights == 0, want == 0)
    behind = np.zeros(len(leaves), bool)
    crossed = np.zeros(len(leaves), bool)
    crossed[w["leaf"][(w["leaf"] >= 0) & (w["t_out"] > w["t_in"])]] = True
    behind = crossed & (data[:, 3] > 0) & (weights == 0)
    action = (weights != 0).astype(np.uint8)
    share = 1.0 - action.mean()
    print("unseen: %d leaves, %.3f dropped (%d without density, %d crossed but behind an opaque "
          "leaf on every ray)" % (len(leaves), share, (data[:, 3] == 0).sum(), behind.sum()))
    assert share >= 0.25 and behind.any() and (data[:, 3] == 1e30).any()
    pruned, parent = tree.refine(action)
    assert pruned.num_leaves == int(action.sum())
    assert np.array_equal(bits(pruned.leaf_data()), bits(data[parent]))
    for t_min in T_MINS:
        if t_min > 0:
            # the weights belong to a t_min: measure again
            weights = tree.leaf_weights(starts, dirs, t_min)
            pruned, _ = tree.refine((weights != 0).astype(np.uint8))
        want = tree.render_volume(starts, dirs, t_min, BG)
        got = pruned.render_volume(starts, dirs, t_min, BG)
        assert np.array_equal(bits(got.color), bits(want.color))
        assert np.array_equal(bits(got.alpha), bits(want.alpha))
        assert np.array_equal(bits(got.depth), bits(want.depth))
        if t_min == 0:
            assert (want.alpha > 0).mean() > 0.3           # the restatement: 0.38


# ------------------------------------------------------------------------------- driver
@functools.lru_cache(maxsize=None)
def scene():
    """scene16's training images and a small density tree of the opaque ball (depth 4), plain and
    with SH leaves of degree 1."""
    import fourier_feature_nets as ffn
    model = opaque_ball().to("cuda")
    dataset = ffn.ImageDataset.load(SCENE, "train", 64, True, False, None, device="cuda")
    tree = ffn.OcTree.build_from_model(model, 4)
    assert 8 < tree.num_leaves < 4096
    return dataset, tree, tree.bake_sh(model, 1, 8)


@pytest.mark.parametrize("kind", ["plain", "sh"])
def test_no_rounds_is_the_plain_fit(kind):
    import fourier_feature_nets as ffn
    dataset, plain, sh = scene()
    tree, fit = (plain, ffn.fit_octree) if kind == "plain" else (sh, ffn.fit_octree_sh)
    kwargs = dict(batch_size=1024, num_steps=12, report_interval=5, verbose=False)
    fitted, log = fit(tree, dataset, dataset, **kwargs)
    again, log2, reports = ffn.fit_octree_adaptive(tree, dataset, dataset, rounds=0, **kwargs)
    assert reports == [] and again.sh_degree == tree.sh_degree
    for key in ("node_index", "leaf_index"):
        assert np.array_equal(again.state_dict[key], fitted.state_dict[key])
    assert np.array_equal(bits(again.leaf_data()), bits(fitted.leaf_data()))
    assert not np.array_equal(bits(fitted.leaf_data()), bits(tree.leaf_data()))
    assert [e.step for e in log2] == [e.step for e in log] and len(log2) == 12
    assert np.array_equal(bits([e.loss for e in log2]), bits([e.loss for e in log]))
    assert np.array_equal(bits([e.val_psnr for e in log2]), bits([e.val_psnr for e in log]))


@pytest.mark.parametrize("kind", ["plain", "sh"])
def test_one_round_with_a_split(kind):
    import fourier_feature_nets as ffn
    dataset, plain, sh = scene()
    tree = plain if kind == "plain" else sh
    kwargs = dict(batch_size=1024, num_steps=10, report_interval=5, verbose=False)
    fitted, logs, reports = ffn.fit_octree_adaptive(tree, dataset, dataset, rounds=1, **kwargs)
    assert len(logs) == 2 and len(reports) == 1
    report = reports[0]
    kept = report.leaves_before - report.dropped - report.split
    print(kind, report)
    assert report.round == 0 and report.leaves_before == tree.num_leaves
    assert kept >= 0 and report.split > 0
    assert report.leaves_after == kept + 8 * report.split == fitted.num_leaves
    assert report.depth_before == tree.depth and report.depth_after == tree.depth + 1
    assert fitted.depth == tree.depth + 1 and fitted.sh_degree == tree.sh_degree
    assert len(report.weight_quantiles) == 5 and list(report.weight_quantiles) == \
        sorted(report.weight_quantiles) and 0.0 <= report.weight_quantiles[0] \
        and report.weight_quantiles[-1] <= 1.0
    state = fitted.state_dict
    assert np.array_equal(state["node_index"], rref.ancestors(state["leaf_index"]))
    assert fitted.leaf_data().shape == (fitted.num_leaves, tree.leaf_data().shape[1])
    assert np.isfinite(fitted.leaf_data()).all() and fitted.center == tree.center
    for log in logs:
        assert len(log) == 10 and [e.step for e in log] == list(range(10))
        assert np.isfinite([e.loss for e in log]).all()
        assert np.isfinite([e.val_psnr for e in log]).all()        # steps below 10 all report
    # the depth cap keeps what would split
    capped, _, reports = ffn.fit_octree_adaptive(tree, dataset, None, rounds=1,
                                                 max_depth=tree.depth, **kwargs)
    assert reports[0].split == 0 and capped.depth <= tree.depth
    # the measurement alone, camera by camera, is one call over all rays
    sampler = dataset.sampler
    weights = ffn.leaf_weights_over(tree, dataset)
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    whole = tree.leaf_weights(sampler.starts - shift, sampler.directions)
    assert weights.dtype == np.float32 and weights.shape == (tree.num_leaves,)
    assert np.array_equal(bits(weights), bits(whole.cpu().numpy())) and (weights > 0).any()


def test_train_octree_program_with_refinement(tmp_path):
    import fourier_feature_nets as ffn
    data_path, tree_path, out_path, pruned_path = [
        str(tmp_path / name) for name in ("data.npz", "tree.npz", "out.npz", "pruned.npz")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_synthetic_npz.py"),
                          data_path, "--size", "8", "--cameras", "4"], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    scale, nodes, leaves, data, _, _ = hand_case()
    data = data.copy()
    data[2, 3] = 1.5
    ffn.OcTree(float(scale), nodes, leaves, data).save(tree_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_octree.py"),
                          tree_path, data_path, out_path, "--center", "0", "0", "0", "--steps",
                          "10", "--batch-size", "64", "--refine-rounds", "1", "--prune-below", "0",
                          "--split-above", "0.05"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    told = [line for line in res.stdout.splitlines() if line.startswith("refine 0: leaves 3 -> ")]
    assert len(told) == 1
    fitted = ffn.OcTree.load(out_path)
    assert "%d leaves fitted" % fitted.num_leaves in res.stdout
    state = fitted.state_dict
    assert fitted.num_leaves >= 3 and fitted.leaf_data().shape == (fitted.num_leaves, 4)
    assert np.array_equal(state["node_index"], rref.ancestors(state["leaf_index"]))
    assert int(told[0].split("->")[1].split()[0]) == fitted.num_leaves
    # and the measure-and-refine program alone, pruning only
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "refine_octree.py"),
                          out_path, data_path, pruned_path, "--center", "0", "0", "0",
                          "--no-split", "--prune-below", "1e-6"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "refine 0: leaves %d -> " % fitted.num_leaves in res.stdout
    pruned = ffn.OcTree.load(pruned_path)
    assert 1 <= pruned.num_leaves <= fitted.num_leaves
    assert "%d leaves written" % pruned.num_leaves in res.stdout
