"""The K30 mesh contract once more (see tests/octree_mesh_reference.py for the contract and for
the derivation of the budgets), restated for trees too deep to expand: nothing here is ``n^3``.

It works from the SET of solid finest cells.  Each solid leaf is enumerated as its ``k^3`` finest
cells (``k <= 8`` is asserted: a solid root leaf at depth 21 would be ``2^60`` cells); their corners
are the only corners that can be vertices; the eight samples of a corner are looked up in the sorted
int64 array of solid cell keys ``(x n + y) n + z`` (solidity) and, for the opacities of cells that
are not solid, by the ids of the cell's ancestors in the leaf index.  Keys, masks, ownership of
quads, faces, offsets, colours and normals are the dense module's, and the fields returned are its
``MeshReference``.

One budget differs.  The dense module bounds a position's three roundings by the cube's reach,
``M = |center|_max + (n/2 + 1) side``.  Here each vertex has its own operand magnitude:

    B_pos(v) = side * B_off(v) + 3 eps (|center|_max + (max_axis |c - n/2| + 1) side)

which is the same derivation (``(c - n/2) + off`` is at most ``max|c - n/2| + 1/2`` cells, times
``side``, plus the centre) and never exceeds the dense budget, since ``|c - n/2| <= n/2``.  A vertex
near the centre of a depth-21 cube is then held tightly, one at its far corner to what f32 can give
(``(c - n/2) + off`` rounds to 2^-5 of a cell at ``|c - n/2| = 2^19``)."""

import numpy as np

from tests.octree_mesh_reference import (EPS, PLACEMENTS, MeshReference, leaf_levels_cells,
                                         opacities)


def level_offset(level):
    """The id of cell (0, 0, 0) of the 2^level grid: (8^level - 1) / 7, a Python integer."""
    return (8 ** int(level) - 1) // 7


def path_codes(cells, level):
    """(K,3) int64 cells of the 2^level grid -> (K,) int64 path codes: three bits a level, the
    root's child first, digit 4 [x] + 2 [y] + [z]."""
    cells = np.asarray(cells, np.int64)
    code = np.zeros(len(cells), np.int64)
    for bit in range(int(level) - 1, -1, -1):
        digit = 4 * ((cells[:, 0] >> bit) & 1) + 2 * ((cells[:, 1] >> bit) & 1) + ((cells[:, 2] >> bit) & 1)
        code = 8 * code + digit
    return code


def cell_leaves(leaf_index, levels, depth, cells):
    """(K,3) finest cells -> (K,) the number of the leaf that covers each, -1 for empty space and
    for cells outside the cube: per level that has a leaf, the id of the cell's ancestor there."""
    cells = np.asarray(cells, np.int64).reshape(-1, 3)
    n = 1 << (depth - 1)
    inside = ((cells >= 0) & (cells < n)).all(1)
    found = np.full(len(cells), -1, np.int64)
    clipped = np.where(inside[:, None], cells, 0)
    for level in np.unique(levels).tolist():
        shift = depth - 1 - level
        ids = path_codes(clipped >> shift, level) + level_offset(level)
        at = np.minimum(np.searchsorted(leaf_index, ids), len(leaf_index) - 1)
        match = inside & (leaf_index[at] == ids)
        assert (found[match] == -1).all(), "a leaf inside another leaf"
        found[match] = at[match]
    return found


def solid_cells(levels, cells, leaf_solid, depth):
    """The finest cells of the solid leaves -> (S,3) int64."""
    out = []
    for l in np.nonzero(leaf_solid)[0].tolist():
        k = 1 << (depth - 1 - int(levels[l]))
        assert k <= 8, "a solid leaf of %d^3 finest cells: the sparse reference enumerates them" % k
        a = np.arange(k, dtype=np.int64)
        block = np.stack(np.meshgrid(a, a, a, indexing="ij"), -1).reshape(-1, 3)
        out.append(block + cells[l] * k)
    return np.concatenate(out) if out else np.zeros((0, 3), np.int64)


def corner_keys(corners, n):
    c = np.asarray(corners, np.int64)
    return (c[..., 0] * (n + 1) + c[..., 1]) * (n + 1) + c[..., 2]


BITS = np.array([[(b >> 2) & 1, (b >> 1) & 1, b & 1] for b in range(8)], np.int64)


def extract(scale, leaf_index, leaf_data=None, sh_degree=None, alpha_threshold=0.5,
            placement="surface_nets", center=(0.0, 0.0, 0.0), solid=None) -> MeshReference:
    assert placement in PLACEMENTS
    leaf_index = np.asarray(leaf_index, np.int64)
    assert (np.diff(leaf_index) > 0).all()
    num = len(leaf_index)
    levels, cells = leaf_levels_cells(leaf_index)
    depth = int(levels.max()) + 1
    n = 1 << (depth - 1)
    side = float(np.float32(2.0) * np.float32(scale) / np.float32(n))
    center = np.asarray([np.float32(c) for c in center], np.float64)
    alpha, thr, rgb, color_scale, sh_reach = opacities(leaf_data, sh_degree, num, side,
                                                       alpha_threshold, solid)
    leaf_solid = alpha > thr
    filled = solid_cells(levels, cells, leaf_solid, depth)
    filled_keys = np.sort((filled[:, 0] * n + filled[:, 1]) * n + filled[:, 2])
    assert (np.diff(filled_keys) > 0).all(), "a leaf inside another leaf"

    # candidates: the corners of the solid cells, once each, by ascending key
    candidates = (filled[:, None, :] + BITS[None, :, :]).reshape(-1, 3)
    _, first = np.unique(corner_keys(candidates, n), return_index=True)
    candidates = candidates[first]
    # sample b of corner c is the cell c - 1 + (dx, dy, dz)
    sample_cells = candidates[:, None, :] - 1 + BITS[None, :, :]                    # (K,8,3)
    inside = ((sample_cells >= 0) & (sample_cells < n)).all(-1)
    keys = (sample_cells[..., 0] * n + sample_cells[..., 1]) * n + sample_cells[..., 2]
    at = np.minimum(np.searchsorted(filled_keys, keys), max(len(filled_keys) - 1, 0))
    solid_s = inside & (filled_keys[at] == keys) if len(filled_keys) else np.zeros(keys.shape, bool)
    mask_all = (solid_s.astype(np.int64) << np.arange(8)).sum(-1)
    active = (mask_all != 0) & (mask_all != 255)
    corners = candidates[active]
    count = len(corners)
    masks = mask_all[active].astype(np.uint8)
    solid_s = solid_s[active]
    samples = cell_leaves(leaf_index, levels, depth, sample_cells[active].reshape(-1, 3))
    samples = samples.reshape(count, 8)
    # the two lookups agree: a cell is among the solid cells iff a solid leaf covers it
    assert np.array_equal(solid_s, (samples >= 0) & leaf_solid[np.maximum(samples, 0)])
    a = np.where(samples >= 0, alpha[np.maximum(samples, 0)], 0.0)                  # (V,8)

    # faces: per vertex, per axis x, y, z
    vertex_keys = corner_keys(corners, n)
    assert (np.diff(vertex_keys) > 0).all()
    eye = np.eye(3, dtype=np.int64)
    triangles = []
    for v, (c, mask) in enumerate(zip(corners.tolist(), masks.tolist())):
        for ax in range(3):
            here, below = (mask >> 7) & 1, (mask >> (7 ^ (4 >> ax))) & 1
            if here == below:
                continue
            e_u, e_v = eye[(ax + 1) % 3], eye[(ax + 2) % 3]
            quad = [np.array(c), c + e_u, c + e_u + e_v, c + e_v]
            if here:                                    # cell c is the solid one: reversed
                quad = [quad[0], quad[3], quad[2], quad[1]]
            wanted = corner_keys(np.array(quad), n)
            q = np.searchsorted(vertex_keys, wanted)
            assert (q < count).all() and (vertex_keys[np.minimum(q, count - 1)] == wanted).all(), \
                "a quad corner that is not a vertex"
            q = q.tolist()
            triangles += [(q[0], q[1], q[2]), (q[0], q[2], q[3])]
    triangles = np.array(triangles, np.int64).reshape(-1, 3)

    # offsets: the 12 pairs, x first, then y, then z, within an axis by ascending lower bit
    offsets = np.zeros((count, 3))
    swapped = np.zeros((count, 3))
    crossings = np.zeros(count, np.int64)
    smallest = np.full(count, np.inf)
    for ax in range(3):
        step = 4 >> ax
        for b0 in range(8):
            if b0 & step:
                continue
            b1 = b0 | step
            cut = solid_s[:, b0] != solid_s[:, b1]
            p = BITS[b0].astype(np.float64) - 0.5
            with np.errstate(divide="ignore", invalid="ignore"):
                t = (thr - a[:, b0]) / (a[:, b1] - a[:, b0])
                t_swapped = (thr - a[:, b1]) / (a[:, b0] - a[:, b1])
            for out, value in ((offsets, t), (swapped, t_swapped)):
                contribution = np.tile(p, (count, 1))
                contribution[:, ax] += np.where(cut, value, 0.0)
                out[cut] += contribution[cut]
            crossings += cut
            smallest = np.where(cut, np.minimum(smallest, np.abs(a[:, b1] - a[:, b0])), smallest)
    assert (crossings >= 3).all()
    offsets /= crossings[:, None]
    swapped /= crossings[:, None]
    assert (np.abs(offsets) <= 0.5).all()
    offset_budget = 8 * EPS / smallest + 25 * EPS
    if placement == "corners":
        offsets = np.zeros((count, 3))
        swapped = np.zeros((count, 3))
        offset_budget = np.zeros(count)
    vertices = center + (corners - n / 2 + offsets) * side
    reach = np.abs(center).max() + (np.abs(corners - n / 2).max(1) + 1) * side if count else \
        np.zeros(0)
    vertex_budget = side * offset_budget + 3 * EPS * reach

    colors, color_budget = None, 0.0
    if rgb is not None:
        picked = np.where(solid_s[..., None], rgb[np.maximum(samples, 0)], 0.0)     # (V,8,3)
        colors = picked.sum(1) / solid_s.sum(1)[:, None]
        color_budget = 57 * EPS * color_scale
        if sh_degree is not None:
            color_budget += (sh_reach / 4 + 4) * EPS

    signs = 2.0 * BITS - 1.0
    g = (a[..., None] * signs).sum(1)
    length = np.sqrt((g * g).sum(1))
    with np.errstate(divide="ignore", invalid="ignore"):
        normals = np.where(length[:, None] > 0, -g / length[:, None], 0.0)
        normal_budget = np.where(length > 0, 2 * np.sqrt(3) * 72 * EPS / length + 8 * EPS, 0.0)

    return MeshReference(corners, masks, triangles, offsets, vertices, colors, normals,
                         offset_budget, vertex_budget, color_budget, normal_budget, swapped,
                         alpha, thr, float(np.abs(alpha - thr).min()), len(filled), side, n)


# ------------------------------------------------------------------- checkers of a device mesh
def check_integers(corners, masks, triangles, ref):
    """The integer fields of a mesh against ``ref``, exactly."""
    np.testing.assert_array_equal(np.asarray(corners, np.int64), ref.corners)
    np.testing.assert_array_equal(np.asarray(masks), ref.masks)
    np.testing.assert_array_equal(np.asarray(triangles, np.int64), ref.triangles)


def check_keys(keys, ref):
    """int64 corner keys against the reference's, computed in Python integers."""
    n1 = ref.cells + 1
    want = [(int(i) * n1 + int(j)) * n1 + int(k) for i, j, k in ref.corners.tolist()]
    assert np.asarray(keys).dtype == np.int64
    assert [int(x) for x in np.asarray(keys).tolist()] == want
