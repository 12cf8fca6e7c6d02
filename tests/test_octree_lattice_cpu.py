"""The lattice family of tests/octree_lattice_helpers.py on the host: the rays are exact in f32,
they are the rays the margin rule of the other octree tests leaves out, every tie class occurs,
and the hand-built trees are sound."""

import numpy as np
import pytest

from tests import octree_reference as oref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import (cell_id, closed_touch, grid_tree, lattice_rays,
                                          level_cells, mixed_tree, tie_classes)
from tests.octree_render_helpers import ray_budget
from tests.octree_walk_helpers import two_level_tree


def trees():
    scale, nodes, leaves = two_level_tree()
    yield "two levels", scale, nodes, leaves, 3
    yield ("mixed",) + mixed_tree() + (5,)
    yield "root only", np.float32(2.0), np.zeros(0, np.int64), np.array([0], np.int64), 1


@pytest.mark.parametrize("case", list(trees()), ids=lambda c: c[0])
def test_lattice_rays_are_exact_and_tied(case):
    name, scale, nodes, leaves, depth = case
    starts, dirs = lattice_rays(scale, depth, 4000, 3)
    assert starts.dtype == dirs.dtype == np.float32 and starts.shape == dirs.shape == (4000, 3)
    assert dirs.any(1).all() and set(np.unique(np.abs(dirs))) == {0.0, 0.5, 1.0, 2.0}
    half_side = float(scale) / 2 ** (depth - 1)
    assert (starts / half_side == np.round(starts / half_side)).all()
    assert np.abs(starts).max() == float(scale) + 2 * half_side          # one cell beyond
    inside = (np.abs(starts) < scale).all(1)
    on_face = (np.abs(starts) <= scale).all(1) & ~inside
    few = 0 if depth == 1 else 100                       # depth 1: the centre is the only inner point
    assert inside.sum() > few and on_face.sum() > 100 and (~inside & ~on_face).sum() > 100
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    for key in ("t_in", "t_out", "root_in", "root_out"):
        finite = np.isfinite(w[key])
        assert (w[key][finite].astype(np.float32).astype(np.float64) == w[key][finite]).all(), key
    hit = w["hit"]
    tied = hit & (w["margin"] == 0)
    left_out = (hit & ~(w["margin"] > ray_budget(w, scale, starts, dirs))).mean()
    print("%s: %d of %d rays hit, %.3f of them with margin 0; the margin rule would leave out "
          "%.3f of all rays" % (name, hit.sum(), len(hit), tied.sum() / hit.sum(), left_out))
    assert hit.sum() > 400
    if depth == 1:
        return                                           # one region: nothing to tie with
    assert tied.sum() >= 0.5 * hit.sum()
    assert left_out > 0.02                               # past the cap of the other tests


def test_every_tie_class_occurs():
    scale, nodes, leaves = two_level_tree()
    starts, dirs = lattice_rays(scale, 3, 4000, 3)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    classes = tie_classes(scale, 3, w, starts, dirs)
    assert len(classes) == 12
    for name, rows in classes.items():
        print("%-60s %d rays" % (name, rows.sum()))
        assert rows.any(), name
    scale, nodes, leaves = mixed_tree()
    starts, dirs = lattice_rays(scale, 5, 4000, 5)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    for name, rows in tie_classes(scale, 5, w, starts, dirs).items():
        assert rows.any(), name


def check_tree(scale, nodes, leaves, depth):
    assert nodes.dtype == leaves.dtype == np.int64
    assert (np.diff(nodes) > 0).all() and (np.diff(leaves) > 0).all()
    assert not np.isin(leaves, nodes).any()
    # interior nodes are exactly the ancestors of the leaves
    parents = set()
    for node in leaves.tolist():
        while node > 0:
            node = (node - 1) // 8
            parents.add(node)
    assert sorted(parents) == nodes.tolist()
    # the regions tile the cube
    _, slot, centers, half = wref.regions(scale, nodes, leaves)
    assert np.isclose(((2 * half) ** 3).sum(), (2.0 * float(scale)) ** 3, rtol=1e-12, atol=0)
    assert sorted(slot[slot >= 0]) == list(range(len(leaves)))
    # the centre of every leaf is found in that leaf, the centre of every empty region in none
    found = oref.query(np.float32(scale), nodes, leaves, centers.astype(np.float32))
    assert np.array_equal(found, slot)
    _, depths = oref.leaf_geometry(np.float32(scale), leaves)
    assert depths.max() == depth - 1


def test_grid_trees_are_sound():
    assert cell_id(0, 0, 0, 0) == 0 and cell_id(1, 0, 0, 0) == 1 and cell_id(1, 1, 1, 1) == 8
    assert cell_id(2, 2, 2, 2) == 65 and cell_id(2, 3, 3, 3) == 72
    scale, nodes, leaves = two_level_tree()
    built = grid_tree(3, [(1, 0, 0, 0), (2, 2, 2, 2), (2, 3, 3, 3)])
    assert np.array_equal(built[0], nodes) and np.array_equal(built[1], leaves)
    check_tree(scale, nodes, leaves, 3)
    scale, nodes, leaves = mixed_tree()
    check_tree(scale, nodes, leaves, 5)
    _, depths = oref.leaf_geometry(scale, leaves)
    assert set(depths.tolist()) == {2, 3, 4}
    _, slot, _, half = wref.regions(scale, nodes, leaves)
    assert len(np.unique(half[slot < 0])) >= 3               # empty regions of several sizes
    # any leaf count is reachable by dropping cells
    rng = np.random.default_rng(0)
    for count in (1, 2, 255, 256, 257):
        nodes, leaves = grid_tree(4, level_cells(3, rng, count))
        assert len(leaves) == count
        check_tree(np.float32(1.0), nodes, leaves, 4)
    complete = grid_tree(2, level_cells(1))
    assert complete[0].tolist() == [0] and complete[1].tolist() == list(range(1, 9))
    with pytest.raises(AssertionError):
        grid_tree(3, [(1, 0, 0, 0), (2, 0, 0, 0)])             # a leaf inside a leaf


def test_closed_touch():
    scale, _, _ = two_level_tree()
    # along the edge x = y = 0 of leaf 1 ([-1, 0]^3): a touch of the closed box, not a crossing
    t_in, t_out = closed_touch(scale, 1, np.float64([[0, 0, -2]]), np.float64([[0, 0, 1]]))
    assert t_in[0] == 1 and t_out[0] == 2
    # through the corner (0, 0, 0) of leaf 1 from outside it
    t_in, t_out = closed_touch(scale, 1, np.float64([[1, -1, 0]]), np.float64([[-1, 1, 0]]))
    assert t_in[0] == t_out[0] == 1
    t_in, t_out = closed_touch(scale, 1, np.float64([[1, 1, 0.5]]), np.float64([[-1, -1, 0]]))
    assert t_in[0] > t_out[0]                                  # z = 0.5 lies outside
