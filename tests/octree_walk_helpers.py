"""Small fixtures shared by the K13 ray-walk tests (CPU and GPU)."""

import numpy as np


def two_level_tree():
    """Root (interior) with children 1 (leaf), 8 (interior; its children 65 and 72 leaves);
    scale 1.  Child index 4 [x >= 0] + 2 [y >= 0] + [z >= 0]: node 1 is the (-,-,-) octant,
    node 8 the (+,+,+) octant, 65 / 72 its (-,-,-) / (+,+,+) corners.
    -> scale, node_index, leaf_index."""
    return np.float32(1.0), np.array([0, 8], np.int64), np.array([1, 65, 72], np.int64)


def opaque_ball(side=16):
    """A Voxels model with an opaque ball of radius 0.45 in empty space (the model that
    tests/test_octree_gpu.py voxelizes): rays through it end with alpha ~ 1, the others ~ 0."""
    import torch
    import fourier_feature_nets as ffn
    model = ffn.Voxels(side, 1.0)
    axis = (np.arange(side) + 0.5) / side * 2 - 1
    x, y, z = np.meshgrid(axis, axis, axis, indexing="ij")
    inside = x * x + y * y + z * z < 0.45 ** 2
    volume = np.random.default_rng(3).normal(size=(1, 4, side, side, side)).astype(np.float32)
    volume[0, 3] = np.where(inside, 12.0, -12.0)
    with torch.no_grad():
        model.voxels.copy_(torch.from_numpy(volume))
        model.bias.zero_()
    return model
