"""The trees of the K30 tests (CPU and GPU): built by hand from chosen cells
(tests/octree_lattice_helpers.py) with data drawn so that no leaf's solidity hangs on the last bit
of ``expm1f``.  ``case(name)`` -> ``MeshCase``; ``CASES`` names them all."""

from functools import lru_cache
from typing import NamedTuple, Optional

import numpy as np

from tests.octree_lattice_helpers import cell_id, grid_tree, level_cells, mixed_tree

MeshCase = NamedTuple("MeshCase", [
    ("scale", float), ("nodes", np.ndarray), ("leaves", np.ndarray),
    ("leaf_data", Optional[np.ndarray]), ("sh_degree", Optional[int]), ("kwargs", dict),
    ("euler", Optional[int]),       # the Euler characteristic of the surface, where it is known
])


def _order(depth, codes):
    """-> nodes, leaves, and per sorted leaf the position of its code in ``codes``."""
    nodes, leaves = grid_tree(depth, codes)
    ids = np.array([cell_id(int(c[0]), int(c[1]), int(c[2]), int(c[3])) for c in codes], np.int64)
    return nodes, leaves, np.argsort(ids)


def densities(rng, count, side, solid=None):
    """``count`` densities whose opacity over ``side`` lies in [0.05, 0.4] (``solid`` False) or
    [0.6, 0.98] (True; a seeded coin where ``solid`` is None): at least 0.1 from a threshold of
    0.5."""
    if solid is None:
        solid = rng.random(count) < 0.5
    alpha = np.where(solid, rng.uniform(0.6, 0.98, count), rng.uniform(0.05, 0.4, count))
    return (-np.log1p(-alpha) / side).astype(np.float32)


def plain_rows(rng, sigma):
    return np.concatenate([rng.uniform(0.0, 1.0, (len(sigma), 3)).astype(np.float32),
                           np.asarray(sigma, np.float32)[:, None]], 1)


def sh_rows(rng, sigma, degree):
    bases = (degree + 1) ** 2
    return np.concatenate([rng.normal(0.0, 2.0, (len(sigma), 3 * bases)).astype(np.float32),
                           np.asarray(sigma, np.float32)[:, None]], 1)


def side_of(scale, leaves):
    from tests.octree_mesh_reference import tree_depth
    return 2.0 * float(scale) / (1 << (tree_depth(leaves) - 1))


def levels_tree():
    """Depth 5, scale 2, levels 1 to 4.  The level-1 leaf (0, 0, 0) is solid; across its +x face lie,
    mid-face, a solid level-2 leaf, a level-2 leaf that is not solid, solid and not-solid level-3
    leaves, level-4 leaves and empty space.  -> scale, nodes, leaves, solid flag per sorted leaf."""
    codes = [(1, 0, 0, 0, True), (1, 1, 1, 1, False),
             (2, 2, 0, 0, True), (2, 2, 1, 0, False), (2, 3, 1, 1, True),
             (3, 4, 0, 2, True), (3, 4, 1, 2, False), (3, 5, 1, 3, True), (3, 4, 2, 2, True),
             (4, 8, 2, 6, True), (4, 8, 3, 7, True), (4, 9, 3, 7, False), (4, 8, 0, 6, False),
             (4, 7, 8, 7, True), (4, 0, 8, 0, True)]
    nodes, leaves, order = _order(5, [c[:4] for c in codes])
    return np.float32(2.0), nodes, leaves, np.array([c[4] for c in codes])[order]


def random_tree(seed=5):
    """Depth 4: per level-1 cell a split, per level-2 cell a leaf, empty or a split whose level-3
    children are leaves or empty, by a seeded draw."""
    rng = np.random.default_rng(seed)
    codes = []
    for _, x, y, z in level_cells(2):
        kind = rng.integers(0, 3)
        if kind == 0:
            codes.append((2, x, y, z))
        if kind < 2:
            continue
        fine = [(3, 2 * x + (e >> 2), 2 * y + (e >> 1 & 1), 2 * z + (e & 1))
                for e in range(8) if rng.random() < 0.5]
        codes.extend(fine or [(3, 2 * x, 2 * y, 2 * z)])
    nodes, leaves = grid_tree(4, codes)
    return np.float32(1.0), nodes, leaves


def _cells(depth, cells):
    return grid_tree(depth, [(depth - 1, x, y, z) for x, y, z in cells])


CUBOID = (2, 3, 4)          # cells along x, y, z


@lru_cache(maxsize=None)
def case(name) -> MeshCase:
    rng = np.random.default_rng(sum(map(ord, name)))       # a seed per name, the same in every run
    if name == "lone":
        nodes, leaves = _cells(3, [(1, 2, 1)])
        return MeshCase(1.0, nodes, leaves, np.float32([[0.2, 0.4, 0.6]]), None, {}, 2)
    if name == "lone_coarse":
        # one level-1 leaf of 2^3 finest cells; a far level-2 leaf of density 0 makes the depth 3
        nodes, leaves, order = _order(3, [(1, 0, 1, 0), (2, 3, 0, 3)])
        sigma = np.float32([50.0, 0.0])[order]
        return MeshCase(1.0, nodes, leaves, plain_rows(rng, sigma), None, {}, 2)
    if name == "cuboid":
        p, q, r = CUBOID
        cells = [(1 + x, 2 + y, 3 + z) for x in range(p) for y in range(q) for z in range(r)]
        nodes, leaves = _cells(4, cells)
        data = rng.uniform(0, 1, (len(leaves), 3)).astype(np.float32)
        return MeshCase(2.0, nodes, leaves, data, None, {}, 2)
    if name == "ring":
        cells = [(x, 1, z) for x in range(3) for z in range(1, 4) if (x, z) != (1, 2)]
        nodes, leaves = _cells(3, cells)
        return MeshCase(1.0, nodes, leaves, None, None, {}, 0)
    if name == "root":
        return MeshCase(0.5, np.zeros(0, np.int64), np.zeros(1, np.int64),
                        np.float32([[0.9, 0.1, 0.3]]), None, {}, 2)
    if name == "full":
        nodes, leaves = grid_tree(3, level_cells(2))
        data = rng.uniform(0, 1, (len(leaves), 3)).astype(np.float32)
        return MeshCase(1.0, nodes, leaves, data, None, {}, 2)
    if name == "none_solid":
        nodes, leaves = grid_tree(3, level_cells(2, rng, 20))
        sigma = densities(rng, len(leaves), side_of(1.0, leaves), np.zeros(len(leaves), bool))
        return MeshCase(1.0, nodes, leaves, plain_rows(rng, sigma), None, {}, None)
    if name == "touching":
        # (0,0,0) and (1,1,0) share an edge, (1,1,0) and (2,2,1) a corner
        nodes, leaves = _cells(3, [(0, 0, 0), (1, 1, 0), (2, 2, 1)])
        data = rng.uniform(0, 1, (3, 3)).astype(np.float32)
        return MeshCase(1.0, nodes, leaves, data, None, {}, None)
    if name.startswith("mixed"):
        scale, nodes, leaves = mixed_tree()
        sigma = densities(rng, len(leaves), side_of(scale, leaves))
        sigma[::17] = 0.0
        sigma[5::23] = -3.0
        sigma[7::29] = np.nan
        if name == "mixed":
            return MeshCase(scale, nodes, leaves, plain_rows(rng, sigma), None, {}, None)
        if name == "mixed_threshold":
            # 0.3 and 0.7: the opacities keep at least 0.1 from both
            sigma = densities(rng, len(leaves), side_of(scale, leaves))
            alpha = -np.expm1(-sigma.astype(np.float64) * side_of(scale, leaves))
            low = (alpha > 0.2) & (alpha < 0.45)
            sigma[low] *= 0.25
            return MeshCase(scale, nodes, leaves, plain_rows(rng, sigma), None,
                            {"alpha_threshold": 0.3}, None)
        if name == "mixed_solid":
            return MeshCase(scale, nodes, leaves, plain_rows(rng, sigma), None,
                            {"solid": rng.random(len(leaves)) < 0.4}, None)
        if name == "mixed_center":
            return MeshCase(scale, nodes, leaves, plain_rows(rng, sigma), None,
                            {"center": (0.3, -1.7, 2.9)}, None)
        if name == "mixed_wide":
            # more columns than four: the first four are read
            rows = np.concatenate([plain_rows(rng, sigma),
                                   rng.normal(0, 1, (len(leaves), 3)).astype(np.float32)], 1)
            return MeshCase(scale, nodes, leaves, rows.astype(np.float64), None, {}, None)
    if name == "levels":
        scale, nodes, leaves, solid = levels_tree()
        sigma = densities(rng, len(leaves), side_of(scale, leaves), solid)
        return MeshCase(scale, nodes, leaves, plain_rows(rng, sigma), None, {}, None)
    if name.startswith("random"):
        scale, nodes, leaves = random_tree()
        sigma = densities(rng, len(leaves), side_of(scale, leaves))
        if name == "random":
            return MeshCase(scale, nodes, leaves, plain_rows(rng, sigma), None, {}, None)
        if name == "random_colors":
            data = rng.uniform(0, 1, (len(leaves), 3)).astype(np.float32)
            return MeshCase(scale, nodes, leaves, data, None, {}, None)
        if name in ("random_sh1", "random_sh2"):
            degree = int(name[-1])
            return MeshCase(scale, nodes, leaves, sh_rows(rng, sigma, degree), degree, {}, None)
    raise KeyError(name)


CASES = ("lone", "lone_coarse", "cuboid", "ring", "root", "full", "none_solid", "touching", "mixed",
         "mixed_threshold", "mixed_solid", "mixed_center", "mixed_wide", "levels", "random",
         "random_colors", "random_sh1", "random_sh2")


@lru_cache(maxsize=None)
def reference(name, placement="surface_nets"):
    """The reference mesh of ``case(name)``, computed once and shared: do not write into it."""
    from tests import octree_mesh_reference as mref
    c = case(name)
    return mref.extract(c.scale, c.leaves, c.leaf_data, c.sh_degree, placement=placement,
                        **c.kwargs)


def parse_obj(path):
    """-> vertices (V,3) f32, colors (V,3) f32 or None, normals or None, faces (F,3) 0-based, and
    whether every face corner was written as ``a//a``."""
    rows, normals, faces, paired = [], [], [], True
    with open(path) as f:
        for line in f:
            parts = line.split()
            if not parts or parts[0].startswith("#"):
                continue
            if parts[0] == "v":
                rows.append([np.float32(x) for x in parts[1:]])
            elif parts[0] == "vn":
                normals.append([np.float32(x) for x in parts[1:]])
            elif parts[0] == "f":
                corner = [p.split("//") for p in parts[1:]]
                paired = paired and all(len(c) == 2 and c[0] == c[1] for c in corner)
                faces.append([int(c[0]) - 1 for c in corner])
    rows = np.array(rows, np.float32).reshape(len(rows), len(rows[0]) if rows else 3)
    return (rows[:, :3], rows[:, 3:] if rows.shape[1] == 6 else None,
            np.array(normals, np.float32) if normals else None,
            np.array(faces, np.int64).reshape(-1, 3), paired)
