"""Inputs on which the K13 walk has EXACT answers: rays on the lattice of a tree's finest cells,
and trees built by hand from chosen cells (CPU and GPU tests).

With a power-of-two ``scale`` every plane of a region is a multiple of the finest side
``2 scale / 2^(depth-1)``.  ``lattice_rays`` starts on multiples of HALF that side (cell corners,
edge midpoints, face and cell centres) and takes direction components from {0, +-0.5, +-1, +-2},
so every plane crossing ``(plane - o) / d`` and every point ``o + t d`` is a small dyadic number:
f32 computes them without rounding, and so does the float64 restatement
(tests/octree_walk_reference.py).  Such rays tie all the time -- two or three exit planes at one
t, a zero component on a cell plane, an entry through an edge or a corner -- which is what the
margin rule of the other octree tests leaves out."""

import numpy as np

COMPONENTS = np.float32([0, 0.5, -0.5, 1, -1, 2, -2])


def lattice_rays(scale, depth, count, seed):
    """-> starts, directions (count,3) f32.  Starts: multiples of half a finest side, up to one
    cell beyond the cube on every axis (outside, on a face, inside).  Directions: components in
    {0, +-0.5, +-1, +-2}, not all zero."""
    scale = float(scale)
    assert scale > 0 and np.log2(scale) == np.round(np.log2(scale)), "scale: a power of two"
    rng = np.random.default_rng(seed)
    cells = 1 << (depth - 1)
    step = np.float32(scale / cells)                     # half a finest side
    reach = cells + 2                                    # the cube is +-cells steps
    # three coordinates in four lie on a cell plane (an even multiple), so that corners outweigh
    # edge midpoints, face centres and cell centres
    steps = rng.integers(-reach, reach + 1, (count, 3))
    steps = np.where(((steps - cells) % 2 != 0) & (rng.random((count, 3)) < 0.5), steps + 1, steps)
    steps = np.minimum(steps, reach)
    # one ray in eight is moved onto the cube's own planes, each coordinate with probability one
    # half: starts on its faces, edges and corners at any depth
    snap = (rng.random(count) < 0.125)[:, None] & (rng.random((count, 3)) < 0.5)
    steps = np.where(snap, np.where(rng.random((count, 3)) < 0.5, cells, -cells), steps)
    starts = steps.astype(np.float32) * step
    directions = COMPONENTS[rng.integers(0, len(COMPONENTS), (count, 3))]
    none = ~directions.any(1)
    directions[none, rng.integers(0, 3, int(none.sum()))] = np.float32(1)
    return starts, directions


def cell_id(level, ix, iy, iz):
    """The id of cell (ix, iy, iz) of the 2^level grid: ``8 * parent + 1 + digit`` from the root
    down, digit = 4 [x upper] + 2 [y upper] + [z upper]."""
    node = 0
    for k in range(level - 1, -1, -1):
        node = 8 * node + 1 + (4 * ((ix >> k) & 1) + 2 * ((iy >> k) & 1) + ((iz >> k) & 1))
    return node


def grid_tree(depth, leaf_codes):
    """``leaf_codes``: (level, ix, iy, iz) per leaf, level <= depth - 1, the cell of the 2^level
    grid (x, y, z from the cube's - corner).  -> node_index, leaf_index (sorted int64): the leaves,
    and as interior nodes exactly their ancestors.  No leaf may lie inside another."""
    leaves, nodes = set(), set()
    for level, ix, iy, iz in leaf_codes:
        assert 0 <= level <= depth - 1 and 0 <= min(ix, iy, iz) and max(ix, iy, iz) < 1 << level
        node = cell_id(int(level), int(ix), int(iy), int(iz))
        leaves.add(node)
        while node > 0:
            node = (node - 1) // 8
            nodes.add(node)
    assert not (leaves & nodes), "a leaf inside another leaf"
    return np.array(sorted(nodes), np.int64), np.array(sorted(leaves), np.int64)


def level_cells(level, rng=None, count=None):
    """Every cell of the 2^level grid as (level, ix, iy, iz) rows, or ``count`` of them drawn
    without repetition."""
    side = 1 << level
    flat = np.arange(side ** 3)
    if count is not None:
        flat = np.sort(rng.choice(flat, count, replace=False))
    return np.stack([np.full(len(flat), level), flat // (side * side), flat // side % side,
                     flat % side], 1)


def mixed_tree():
    """Depth 5, scale 2: leaves at levels 2, 3 and 4 and empty regions of four sizes.  Per level-2
    cell (64 of them) by a seeded draw: a leaf, empty, or split; per level-3 child of a split
    cell again; the level-4 children are leaves or empty.  -> scale, node_index, leaf_index."""
    rng = np.random.default_rng(41)
    codes = []
    for _, x, y, z in level_cells(2):
        kind = rng.integers(0, 4)                       # 0 leaf, 1 empty, 2 / 3 split
        if kind == 0:
            codes.append((2, x, y, z))
        if kind < 2:
            continue
        for c in range(8):
            x3, y3, z3 = 2 * x + (c >> 2), 2 * y + (c >> 1 & 1), 2 * z + (c & 1)
            kind = rng.integers(0, 3)                   # 0 leaf, 1 empty, 2 split
            if kind == 0:
                codes.append((3, x3, y3, z3))
            if kind < 2:
                continue
            fine = [(4, 2 * x3 + (e >> 2), 2 * y3 + (e >> 1 & 1), 2 * z3 + (e & 1))
                    for e in range(8) if rng.random() < 0.5]
            codes.extend(fine or [(4, 2 * x3, 2 * y3, 2 * z3)])
    nodes, leaves = grid_tree(5, codes)
    return np.float32(2.0), nodes, leaves


def closed_touch(scale, leaf_id, starts, directions):
    """Float64 slab test of the CLOSED box of node ``leaf_id`` (one id, or one per ray) against
    rays (K,3): -> t_in, t_out.  A zero component constrains nothing when ``lo <= o <= hi``."""
    from tests import octree_reference as oref
    ids = np.broadcast_to(np.asarray(leaf_id, np.int64), (len(starts),))
    centers, depths = oref.leaf_geometry(np.float32(scale), ids)
    half = (np.float64(np.float32(scale)) / 2.0 ** depths)[:, None]
    c = centers.astype(np.float64)
    o, d = np.asarray(starts, np.float64), np.asarray(directions, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (c - half - o) / d, (c + half - o) / d
    inside = (o >= c - half) & (o <= c + half)
    near = np.where(d == 0, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    far = np.where(d == 0, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    return near.max(1), far.min(1)


def tie_classes(scale, depth, w, starts, directions):
    """Which tie classes the rays hold: -> dict of bool (R,) arrays.  Exit ties are counted on
    crossings of positive chord whose exit lies inside the cube (``t_out < root_out``)."""
    scale = float(scale)
    o = np.asarray(starts, np.float64)
    d = np.asarray(directions, np.float64)
    count = len(o)
    side = 2.0 * scale / (1 << (depth - 1))
    ray = w["ray"]
    point = o[ray] + w["t_out"][:, None] * d[ray]
    on_plane = (np.abs(point / side - np.round(point / side)) == 0) & (d[ray] != 0)
    inner = w["t_out"] < w["root_out"][ray]
    planes = np.zeros(count, np.int64)
    np.maximum.at(planes, ray[inner], on_plane[inner].sum(1))
    # the same count over the tied axes the ray crosses BACKWARDS: a tie of negative directions
    # is one whose tied planes are all crossed with d < 0
    backward = on_plane & (d[ray] < 0)
    all_back = inner & (backward.sum(1) == on_plane.sum(1))
    planes_back = np.zeros(count, np.int64)
    np.maximum.at(planes_back, ray[all_back], on_plane[all_back].sum(1))
    zero = d == 0
    on_grid = (o / side == np.round(o / side))
    interior = zero & on_grid & (np.abs(o) < scale)
    hit = w["hit"]
    # a zero component has no sign of its own: the ray runs backwards on EVERY other axis
    others_back = ((d < 0) | zero).all(1)
    out = {
        "two-plane exit": hit & (planes == 2),
        "three-plane exit": hit & (planes == 3),
        "zero component on an interior plane": hit & interior.any(1),
        "zero component on the +face": hit & (zero & (o == scale)).any(1),
        "zero component on the -face": hit & (zero & (o == -scale)).any(1),
        "start on a corner of the cube": hit & (np.abs(o) == scale).all(1),
    }
    negative = {
        "two-plane exit": hit & (planes_back == 2),
        "three-plane exit": hit & (planes_back == 3),
        "zero component on an interior plane": others_back,
        "zero component on the +face": others_back,
        "zero component on the -face": others_back,
        # into the cube from a corner with a + coordinate, along that axis
        "start on a corner of the cube": ((o == scale) & (d < 0)).any(1),
    }
    for name in list(out):
        out[name + ", negative direction"] = out[name] & negative[name]
    return out
