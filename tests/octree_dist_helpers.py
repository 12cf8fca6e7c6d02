"""Inputs shared by the K29 distortion tests (CPU and GPU): the cases of the K17 tests -- the hand
case, the golden trees with their recorded rays, the depth-6 cloud with 20 000 camera rays -- and a
seeded depth-4 tree, each with its float64 walk.  Everything here runs without a GPU: the cloud's
tree comes from the restatement of the build (``octree_reference.build``)."""

import functools
import os

import numpy as np

from tests import octree_reference as oref
from tests import octree_walk_reference as wref
from tests.octree_lattice_helpers import grid_tree, level_cells
from tests.octree_render_helpers import big_cloud, camera_rays, golden_rays, ray_budget
from tests.octree_volume_helpers import hand_case, random_leaf_data

HERE = os.path.dirname(os.path.abspath(__file__))
T_MINS = [0.0, float(np.float32(0.7))]
MIN_TS = [0.0, 1e-3]
CASES = ["hand", "shell", "planes", "cloud"]


class Case:
    """scale, node_index, leaf_index, data (L,4) f32 ``[r, g, b, sigma]``, starts, dirs (R,3) f32,
    w (the float64 walk), center, ok (R,) the rays whose margin exceeds ``ray_budget`` (misses
    included): the others have no single right answer and are left out of both sides."""

    def __init__(self, scale, nodes, leaves, data, starts, dirs, center=(0.0, 0.0, 0.0),
                 every_ray=False):
        self.scale, self.nodes, self.leaves = float(scale), nodes, leaves
        self.data, self.starts, self.dirs, self.center = data, starts, dirs, center
        self.w = wref.walk(scale, nodes, leaves, starts, dirs)
        self.ok = ~self.w["hit"] | (self.w["margin"] > ray_budget(self.w, scale, starts, dirs))
        if every_ray:                # crossings exact in f32: the margin is 0 by construction
            self.ok[:] = True
        self.depth = int(oref.leaf_geometry(np.float32(scale), leaves)[1].max()) + 1

    @property
    def sigma(self):
        return self.data[:, 3]


@functools.lru_cache(maxsize=None)
def case(name):
    if name == "hand":
        scale, nodes, leaves, data, starts, dirs = hand_case()
        data = data.copy()
        data[2, 3] = 1.5             # the opaque leaf made finite, as in the K17 tests
        return Case(scale, nodes, leaves, data, starts, dirs, every_ray=True)
    if name in ("shell", "planes"):
        with np.load(os.path.join(HERE, "golden", "octree.npz")) as g:
            scale, nodes, leaves = (float(g[name + "/scale"]), g[name + "/node_index"],
                                    g[name + "/leaf_index"])
        starts, dirs = golden_rays(name)
        return Case(scale, nodes, leaves, random_leaf_data(scale, leaves), starts, dirs)
    if name == "cloud":
        depth = 6
        built = oref.build(big_cloud(depth), depth, 4)
        scale, nodes, leaves = float(built["scale"]), built["node_index"], built["leaf_index"]
        starts, dirs = camera_rays(np.random.default_rng(depth), 20000, np.float32(scale))
        return Case(scale, nodes, leaves, random_leaf_data(scale, leaves), starts, dirs,
                    tuple(float(c) for c in built["center"]))
    assert name == "depth4"
    rng = np.random.default_rng(29)
    nodes, leaves = grid_tree(4, level_cells(3, rng, 160))
    starts, dirs = camera_rays(rng, 700, np.float32(2.0))
    return Case(2.0, nodes, leaves, random_leaf_data(2.0, leaves, seed=29), starts, dirs)
