"""A vectorised numpy restatement of the reference's octree (octree.py of
matajoh/fourier_feature_nets), for inputs the golden fixtures do not cover: the GPU machine has no
reference.  It restates, level by level over whole arrays, what the reference does node by node:

* root cube: octree.py:756-760 (f32 min / max, ``scale = max(max - min) * 0.5``,
  ``center = 0.5 * (min + max)``, points shifted by the centre in f32);
* child index of a point: octree.py:274-286 (``>=`` on x, y, z adds 4, 2, 1), child centre
  ``c +- scale / 2^k`` with every add rounded to f32, as Node arithmetic on an np.float32 scale
  gives (octree.py:289-335, 544-561);
* build_from_samples: octree.py:762-803 (a child is followed iff it holds >= min_leaf_size
  points; a node none of whose children is followed becomes a leaf with all its points);
* query: octree.py:513-530; leaf centres / depths: octree.py:564-582.

``tests/test_octree_cpu.py`` checks it against trees the reference itself built
(tests/golden/octree.npz).

The second half restates the build OP BY OP, as ``csrc/octree.hip`` splits it (surface points, path
codes, structure from sorted codes, interior nodes), so that every K12 kernel can be compared on
inputs of the test's choosing.  These use no binary search: they count with ``np.unique`` and compare
code prefixes.  ``tests/test_octree_build_ops_cpu.py`` checks that chained together they give the
reference's trees (octree.npz, octree_edges.npz) and ``build``'s ``point_leaf``."""

import numpy as np


def root_cube(positions):
    """-> center (3,) f32, scale f32 (octree.py:756-759)."""
    positions = np.asarray(positions, np.float32)
    lo, hi = positions.min(0), positions.max(0)
    scale = np.float32((hi - lo).max() * np.float32(0.5))
    center = (np.float32(0.5) * (lo + hi)).astype(np.float32)
    return center, scale


def _descend(points, centers, half):
    """One level: child index per point, child centres (f32)."""
    side = points >= centers
    index = side[:, 0] * 4 + side[:, 1] * 2 + side[:, 2] * 1
    centers = np.where(side, centers + half, centers - half).astype(np.float32)
    return index.astype(np.int64), centers


def build(positions, depth, min_leaf_size, data=None):
    """-> dict(node_index, leaf_index (sorted int64), scale (f32), center, point_leaf (leaf id
    per point or -1), leaf_count, leaf_data (float64 means in leaf order, or None))."""
    positions = np.asarray(positions, np.float32)
    n = len(positions)
    center, scale = root_cube(positions)
    points = (positions - center).astype(np.float32)
    ids = np.zeros(n, np.int64)
    centers = np.zeros((n, 3), np.float32)
    alive = np.ones(n, bool)            # the point's node at the current level is visited
    point_leaf = np.full(n, -1, np.int64)
    nodes = []
    half = scale
    if depth == 1:
        alive[:] = n >= min_leaf_size
    for _ in range(1, depth):
        half = np.float32(half / np.float32(2))
        index, child_centers = _descend(points, centers, half)
        child = 8 * ids + 1 + index
        uniq, inverse, counts = np.unique(child[alive], return_inverse=True, return_counts=True)
        followed = np.zeros(n, bool)
        followed[alive] = counts[inverse] >= min_leaf_size
        # parents (among the visited nodes) with at least one followed child
        parents_with_child = np.unique(ids[followed])
        is_interior = alive & np.isin(ids, parents_with_child)
        nodes.append(parents_with_child)
        leaf_here = alive & ~is_interior
        point_leaf[leaf_here] = ids[leaf_here]
        alive = followed
        ids = np.where(alive, child, ids)
        centers = np.where(alive[:, None], child_centers, centers)
    point_leaf[alive] = ids[alive]      # visited at depth - 1 (>= min_leaf_size by construction)
    leaf_index, inverse, counts = np.unique(point_leaf[point_leaf >= 0], return_inverse=True,
                                            return_counts=True)
    leaf_data = None
    if data is not None and len(leaf_index):
        values = np.asarray(data, np.float64).reshape(n, -1)[point_leaf >= 0]
        sums = np.zeros((len(leaf_index), values.shape[1]), np.float64)
        np.add.at(sums, inverse, values)
        leaf_data = sums / counts[:, None]
    node_index = np.unique(np.concatenate(nodes)) if nodes else np.zeros(0, np.int64)
    node_index = np.setdiff1d(node_index, leaf_index).astype(np.int64)
    return dict(node_index=node_index, leaf_index=leaf_index.astype(np.int64), scale=scale,
                center=center, point_leaf=point_leaf, leaf_count=counts, leaf_data=leaf_data)


def query(scale, node_index, leaf_index, positions):
    """octree.py:513-530 for every position (N,3) -> (N,) int64.  Where the reference's loop
    runs off the end of ``leaf_index`` (an id above every leaf id) the answer is -1; a tree
    whose only leaf is the root answers 0 inside the cube."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    scale = np.float32(scale)
    n = len(positions)
    result = np.full(n, -1, np.int64)
    live = ~(np.abs(positions) > scale).any(1)
    if leaf_index[0] == 0:
        result[live] = 0
        return result
    ids = np.zeros(n, np.int64)
    centers = np.zeros((n, 3), np.float32)
    half = scale
    max_id = leaf_index[-1]
    while live.any():
        live &= ids <= max_id
        half = np.float32(half / np.float32(2))
        index, centers = _descend(positions, centers, half)
        ids = np.where(live, 8 * ids + 1 + index, ids)
        at = np.searchsorted(leaf_index, ids)
        hit = live & (leaf_index[np.minimum(at, len(leaf_index) - 1)] == ids)
        result[hit] = at[hit]
        live &= ~hit
        live &= np.isin(ids, node_index)
    return result


def leaf_geometry(scale, leaf_index):
    """Centres (L,3) f32 and depths (L,) int32 of the leaves from their ids."""
    scale = np.float32(scale)
    leaf_index = np.asarray(leaf_index, np.int64)
    depths = np.zeros(len(leaf_index), np.int32)
    digits = []
    ids = leaf_index.copy()
    while (ids > 0).any():
        live = ids > 0
        digits.append(np.where(live, (ids - 1) & 7, -1))
        depths[live] += 1
        ids = np.where(live, (ids - 1) >> 3, ids)
    centers = np.zeros((len(leaf_index), 3), np.float32)
    level = np.zeros(len(leaf_index), np.int32)
    # replay from the root: a leaf of depth d uses its last d digits, deepest first in `digits`
    for k in range(len(digits)):
        # digit of level k + 1 for a leaf of depth d is digits[d - 1 - k]
        which = depths - 1 - k
        live = which >= 0
        digit = np.zeros(len(leaf_index), np.int64)
        for j in range(len(digits)):
            pick = live & (which == j)
            digit[pick] = digits[j][pick]
        half = np.float32(scale / np.float32(2 ** (k + 1)))
        sign = np.stack([(digit & 4) > 0, (digit & 2) > 0, (digit & 1) > 0], 1)
        moved = np.where(sign, centers + half, centers - half).astype(np.float32)
        centers = np.where(live[:, None], moved, centers)
        level += live
    return centers, depths


# ---------------------------------------------------------------------------- op by op
def surface_points(alpha, depth, starts, directions, color, threshold):
    """voxelize_model.py:71-77 in f32: the rays with ``alpha > threshold``, in ray order, at
    ``starts + directions * depth`` (product and sum each rounded to f32), and their colours
    (``None`` without colours)."""
    alpha, depth = np.asarray(alpha, np.float32), np.asarray(depth, np.float32)
    starts, directions = np.asarray(starts, np.float32), np.asarray(directions, np.float32)
    valid = alpha > np.float32(threshold)
    position = starts + directions * depth[..., np.newaxis]
    assert position.dtype == np.float32
    return position[valid], None if color is None else np.asarray(color, np.float32)[valid]


def path_codes(positions, center, scale, depth):
    """The child indices (octree.py:274-286) of every position on its way down a cube the CALLER
    gives, 3 bits per level, root first -> (N,) int64.  The centre is subtracted in f32 first, as
    octree.py:760 shifts the cloud; then ``depth - 1`` descents."""
    positions = np.asarray(positions, np.float32).reshape(-1, 3)
    points = (positions - np.asarray(center, np.float32)).astype(np.float32)
    centers = np.zeros_like(points)
    half = np.float32(scale)
    codes = np.zeros(len(points), np.int64)
    for _ in range(1, depth):
        half = np.float32(half / np.float32(2))
        index, centers = _descend(points, centers, half)
        codes = codes * 8 + index
    return codes


def structure_from_codes(sorted_codes, depth, min_leaf_size):
    """octree.py:762-803 on sorted path codes: the node of level k a point lies in is the first k
    digits of its code.  -> ``leaf`` (N,) int64, the leaf id per sorted point or -1, and
    ``leaves`` (L,3) int64 rows ``(id, start, count)`` in code order: a leaf's points are one run of
    the sorted order."""
    codes = np.asarray(sorted_codes, np.int64)
    n = len(codes)
    assert (np.diff(codes) >= 0).all()
    leaf = np.full(n, -1, np.int64)
    ids = np.zeros(n, np.int64)
    alive = np.full(n, depth > 1 or n >= min_leaf_size)      # the root is always visited
    for level in range(1, depth):
        child = codes >> (3 * (depth - 1 - level))           # the level's node: a code prefix
        _, inverse, counts = np.unique(child[alive], return_inverse=True, return_counts=True)
        followed = np.zeros(n, bool)
        followed[alive] = counts[inverse] >= min_leaf_size
        # a visited node without a followed child is a leaf with all its points; below one
        # with a followed child, the points of the other children are dropped
        interior = alive & np.isin(child >> 3, np.unique(child[followed] >> 3))
        leaf_here = alive & ~interior
        leaf[leaf_here] = ids[leaf_here]
        alive = followed
        ids = np.where(alive, 8 * ids + 1 + (child & 7), ids)
    leaf[alive] = ids[alive]
    head = (leaf >= 0) & (np.concatenate([[-2], leaf[:-1]]) != leaf)
    start = np.flatnonzero(head)
    run = np.cumsum(head) - 1                                # which run a kept point lies in
    count = np.bincount(run[leaf >= 0], minlength=len(start))
    assert (leaf[leaf >= 0] == leaf[start][run[leaf >= 0]]).all()
    return leaf, np.stack([leaf[start], start, count], 1).astype(np.int64).reshape(-1, 3)


def interior_nodes(leaf_ids):
    """The proper ancestors of the leaves (parent of i is ``(i - 1) >> 3``), sorted, each once:
    the ``node_index`` of a tree with these leaves."""
    ids = np.unique(np.asarray(leaf_ids, np.int64))
    found = []
    while (ids > 0).any():
        ids = np.unique((ids[ids > 0] - 1) >> 3)
        found.append(ids)
    return np.unique(np.concatenate(found)) if found else np.zeros(0, np.int64)
