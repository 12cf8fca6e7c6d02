"""Inputs and the per-ray budget shared by the K14 first-hit tests: the generators and the
``ray_budget`` expression of the K13 GPU tests (tests/test_octree_walk_gpu.py), restated here so
that no test module is imported."""

import os

import numpy as np

from tests import octree_walk_reference as wref

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "scene16.npz")
TREES = ["shell", "planes", "nodata"]
LEFT_OUT_CAP = 0.02


def load_tree(name, leaf_data=None):
    import fourier_feature_nets as ffn
    with np.load(os.path.join(HERE, "golden", "octree.npz")) as g:
        return ffn.OcTree(float(g[name + "/scale"]), g[name + "/node_index"],
                          g[name + "/leaf_index"], leaf_data)


def golden_rays(name):
    """The rays of the recorded fixture (its inputs only)."""
    with np.load(os.path.join(HERE, "golden", "octree_walk.npz")) as g:
        return g[name + "/starts"], g[name + "/directions"]


def big_cloud(depth, count=1 << 18):
    """Dense at the centre, sparse towards the faces: leaves at several depths."""
    rng = np.random.default_rng(1000 + depth)
    pos = (rng.random((count, 3), dtype=np.float32) * np.float32(2) - np.float32(1)) ** 5
    return pos


def camera_rays(rng, count, scale):
    """Pinhole-like rays from a few eyes around the cube (|o| 1.5 .. 2.5 scales) towards points
    inside it, and a tenth of them from inside."""
    eyes = rng.normal(size=(16, 3))
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * rng.uniform(1.5, 2.5, (16, 1))
    o = eyes[rng.integers(0, 16, count)] * scale
    target = (rng.random((count, 3)) * 2 - 1) * scale * 1.1        # some pass by
    inside = rng.random(count) < 0.1
    o[inside] = (rng.random((int(inside.sum()), 3)) * 2 - 1) * scale * 0.9
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


def ray_budget(w, scale, starts, directions):
    """Per ray: the largest crossing budget, and the same expression for the planes that do not
    show up as a crossing (a near miss is decided on them too): the cube's extent, the ray's
    smallest nonzero direction component."""
    _, _, per_ray = wref.budgets(w, scale, starts, directions)
    o = np.abs(np.asarray(starts, np.float64)).max(1)
    d = np.abs(np.asarray(directions, np.float64))
    d_min = np.where(d > 0, d, np.inf).min(1)
    t_max = np.maximum(np.abs(w["root_in"]), np.abs(w["root_out"]))
    t_max = np.where(np.isfinite(t_max), t_max, 0.0)
    with np.errstate(divide="ignore", invalid="ignore"):
        wide = 4 * (np.spacing(np.float32(np.float64(scale) + o)).astype(np.float64) / d_min
                    + np.spacing(t_max.astype(np.float32)).astype(np.float64))
    return np.maximum(per_ray, np.where(np.isfinite(wide), wide, np.inf))


def random_colors(count, channels=3, seed=5):
    return np.random.default_rng(seed).random((count, channels), dtype=np.float32)
