"""Inputs shared by the K15 volume-render tests (CPU and GPU): seeded leaf data and the hand-worked
case."""

import numpy as np

from tests import octree_reference as oref
from tests.octree_render_helpers import random_colors
from tests.octree_walk_helpers import two_level_tree

# Optical depth of a leaf crossed along its whole side: DENSITY u^2 with u uniform in [0, 1), so
# that a ray through a handful of leaves is neither empty nor saturated.  Chosen once, on the golden
# trees and the depth-6 cloud, from the restatement alone (the share it gives is asserted).
DENSITY = 0.3


def random_leaf_data(scale, leaf_index, seed=11, channels=4):
    """(L, channels) float32: ``random_colors`` and a density per unit of world length."""
    leaf_index = np.asarray(leaf_index, np.int64)
    _, depths = oref.leaf_geometry(np.float32(scale), leaf_index)
    side = 2.0 * np.float64(np.float32(scale)) / 2.0 ** depths
    u = np.random.default_rng(seed).random(len(leaf_index))
    data = np.zeros((len(leaf_index), channels), np.float32)
    data[:, :3] = random_colors(len(leaf_index), 3)
    data[:, 3] = (DENSITY * u * u / side).astype(np.float32)
    if channels > 4:
        data[:, 4:] = 7.0                                        # never read
    return data


def tie_density(length):
    """A float64 density whose opacity over ``length`` is 0.5 exactly (``np.exp``): followed by an
    opaque leaf, the two weights are T / 2 and (T / 2) * 1, a tie without any rounding."""
    for toward in (np.inf, 0.0):
        sigma = np.log(2.0) / length
        for _ in range(64):
            if 1.0 - np.exp(-(sigma * length)) == 0.5:
                return float(sigma)
            sigma = np.nextafter(sigma, toward)
    raise AssertionError("no float64 density gives an opacity of exactly one half")


def hand_case():
    """``two_level_tree()``: leaf 0 is the cube [-1, 0]^3, leaf 1 [0, 0.5]^3, leaf 2 [0.5, 1]^3.
    An axis-aligned ray meets at most one of them (they touch along the main diagonal only), so
    the rays that need two leaves run along that diagonal.

    -> scale, nodes, leaves, data (3,4) f32, starts, dirs (5,3) f32."""
    scale, nodes, leaves = two_level_tree()
    data = np.float32([[0.25, 0.5, 0.75, 2.0],
                       [1.0, 0.5, 0.0, 3.0],
                       [0.5, 0.25, 1.0, 1e30]])
    starts = np.float32([[-2, -0.5, -0.5],      # +x through leaf 0: t 0.5 .. 1, world length 1
                         [0.25, 0.3, -3],       # +z through leaf 1: t 3 .. 3.5, world length 0.5
                         [0.25, -0.5, -0.25],   # +y from inside the empty (+,-,-) octant: nothing
                         [-2, -2, -2],          # the diagonal: leaves 0, 1, 2 at t 1, 2, 2.5 .. 3
                         [3, 0.75, 0.8]])       # -x through leaf 2 (opaque): t 2 .. 2.5
    dirs = np.float32([[2, 0, 0], [0, 0, 1], [0, 1, 0], [1, 1, 1], [-1, 0, 0]])
    return scale, nodes, leaves, data, starts, dirs
