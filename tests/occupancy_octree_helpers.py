"""Inputs shared by the K25 tests (CPU and GPU): trees, placements of a tree and a grid's box, and
densities round a threshold.  The smallest shapes at which the kernels can go wrong."""

import functools

import numpy as np

from tests import occupancy_octree_reference as kref
from tests.octree_lattice_helpers import grid_tree, level_cells, mixed_tree

F = np.float32
RESOLUTIONS = (1, 5, 31, 32, 33, 64)          # G: one word, odd, and the three round a word
THRESHOLD = F(0.75)


def _leaves(depth, codes):
    return grid_tree(depth, codes)[1]


@functools.lru_cache(maxsize=None)
def tree(name):
    """-> leaf_index (sorted int64).  The scale and the centre come from the placement."""
    rng = np.random.default_rng(25)
    if name == "root":
        return np.zeros(1, np.int64)
    if name == "three":                       # 3 of the 8 depth-2 leaves
        return _leaves(2, [(1, 0, 0, 0), (1, 1, 0, 1), (1, 1, 1, 1)])
    if name == "mixed":                       # 583 leaves, levels 2 - 4
        return mixed_tree()[2]
    if name == "fine":                        # 300 level-7 leaves, all finer than a G = 4 cell
        return _leaves(8, level_cells(7, rng, 300))
    if name.startswith("count"):              # that many level-5 leaves
        return _leaves(6, level_cells(5, rng, int(name[5:])))
    if name.startswith("rows"):
        # under the root cube at G = 64 a level-4 leaf has 4 x 4 = 16 rows, a level-6 leaf one:
        # 127 level-4 leaves in the lower half (2032 rows) and level-6 leaves in the upper half
        total = int(name[4:])
        coarse = [c for c in level_cells(4) if c[3] < 8][:127]
        fine = [c for c in level_cells(6, rng, 4000) if c[3] >= 32][:total - 2032]
        return _leaves(7, coarse + fine)
    raise KeyError(name)


# (scale, centre, box_min, box_size): the root cube of the scale-2 tree; a smaller anisotropic box
# that leaves lie partly and wholly outside of, some with a face on it; a larger box; and a centre
# and a scale at which c +- h + center rounds, under that cube's own box
PLACEMENTS = {
    "cube": (2.0, (0.0, 0.0, 0.0), (-2.0, -2.0, -2.0), (4.0, 4.0, 4.0)),
    "small": (2.0, (0.0, 0.0, 0.0), (-1.0, -0.5, -2.0), (2.5, 1.0, 3.0)),
    "large": (2.0, (0.0, 0.0, 0.0), (-3.0, -2.5, -4.0), (7.0, 6.0, 9.0)),
    "rounded": (0.7, (0.3, -0.2, 0.1), (0.3 - 0.7, -0.2 - 0.7, 0.1 - 0.7), (1.4, 1.4, 1.4)),
}


def placement(name):
    scale, center, box_min, box_size = PLACEMENTS[name]
    return (float(F(scale)), tuple(float(F(v)) for v in center),
            tuple(float(F(v)) for v in box_min), tuple(float(F(v)) for v in box_size))


def densities(count, seed=7):
    """(count,) f32 round THRESHOLD: exactly at it, the f32 just below and just above it, clearly
    below and above, and NaN, in a seeded order."""
    rng = np.random.default_rng(seed)
    pool = np.array([THRESHOLD, np.nextafter(THRESHOLD, F(0)), np.nextafter(THRESHOLD, F(2)),
                     0.0, -1.0, 3.0, np.nan], F)
    return pool[rng.integers(0, len(pool), count)]


@functools.lru_cache(maxsize=None)
def reference(tree_name, place, resolution, with_density=False, dilate=0):
    """The restatement's words for a case, computed once and shared (read-only)."""
    scale, center, box_min, box_size = placement(place)
    ids = tree(tree_name)
    density = densities(len(ids)) if with_density else None
    words = kref.Rule().words(ids, scale, center, box_min, box_size, resolution, density,
                              THRESHOLD if with_density else None, dilate)
    words.setflags(write=False)
    return words
