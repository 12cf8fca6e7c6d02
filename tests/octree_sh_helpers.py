"""Inputs shared by the K18 SH tests (CPU and GPU): two small trees, their rays, seeded SH leaf data
and the share of rays a case leaves out."""

import functools

import numpy as np

from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import grid_tree, level_cells
from tests.octree_render_helpers import camera_rays, ray_budget
from tests.octree_volume_helpers import random_leaf_data

SIZES = [1, 63, 64, 65, 1000]            # around the wave edge, and sixteen workgroups
DEGREES = [1, 2]
K_MAX = 4.0
# optical depth: eight times that of the K15 cases, whose trees are deeper (more leaves per ray)
DENSITY_GAIN = 8.0


def eight_leaves():
    """Depth 2: the eight children of the root, all leaves.  -> scale, node_index, leaf_index."""
    nodes, leaves = grid_tree(2, level_cells(1))
    return np.float32(1.0), nodes, leaves


def mixed_depth4():
    """Depth 4, scale 1.5: leaves at levels 1, 2 and 3 and empty cells of three sizes, by a seeded
    draw per level-1 cell (leaf / empty / split) and again per level-2 child."""
    rng = np.random.default_rng(43)
    codes = []
    for _, x, y, z in level_cells(1):
        kind = rng.integers(0, 4)                       # 0 leaf, 1 empty, 2 / 3 split
        if kind == 0:
            codes.append((1, x, y, z))
        if kind < 2:
            continue
        for c in range(8):
            x2, y2, z2 = 2 * x + (c >> 2), 2 * y + (c >> 1 & 1), 2 * z + (c & 1)
            kind = rng.integers(0, 3)                   # 0 leaf, 1 empty, 2 split
            if kind == 0:
                codes.append((2, x2, y2, z2))
            if kind < 2:
                continue
            fine = [(3, 2 * x2 + (e >> 2), 2 * y2 + (e >> 1 & 1), 2 * z2 + (e & 1))
                    for e in range(8) if rng.random() < 0.5]
            codes.extend(fine or [(3, 2 * x2, 2 * y2, 2 * z2)])
    nodes, leaves = grid_tree(4, codes)
    return np.float32(1.5), nodes, leaves


TREES = {"eight": eight_leaves, "mixed4": mixed_depth4}


def sh_leaf_data(scale, leaf_index, degree, seed=17):
    """(L, 3B+1) float32: coefficients uniform in [-K_MAX, K_MAX], the density of
    ``random_leaf_data`` times DENSITY_GAIN."""
    bases = (degree + 1) ** 2
    rng = np.random.default_rng(seed + degree)
    data = np.empty((len(leaf_index), 3 * bases + 1), np.float32)
    data[:, :-1] = (rng.random((len(leaf_index), 3 * bases)) * 2 - 1) * K_MAX
    data[:, -1] = random_leaf_data(scale, leaf_index)[:, 3] * np.float32(DENSITY_GAIN)
    return data


@functools.lru_cache(maxsize=None)
def case(name):
    """-> scale, node_index, leaf_index, starts, directions (1000 rays), the float64 walk, and per
    ray whether its margin exceeds ``ray_budget`` (or it misses the cube)."""
    scale, nodes, leaves = TREES[name]()
    starts, directions = camera_rays(np.random.default_rng(len(leaves)), max(SIZES), scale)
    w = wref.walk(scale, nodes, leaves, starts, directions)
    ok = ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts, directions))
    return scale, nodes, leaves, starts, directions, w, ok


def prefix(w, n):
    """The walk result of the first ``n`` rays of ``w``."""
    end = int(w["offsets"][n])
    out = {}
    for key, value in w.items():
        if key == "offsets":
            out[key] = value[:n + 1]
        elif key in ("hit", "root_in", "root_out", "margin"):
            out[key] = value[:n]
        else:
            out[key] = value[:end]
    return out
