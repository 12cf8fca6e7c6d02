"""Scenes shared by the K24 tests (CPU and GPU): trees with seeded densities, camera arrays, and the
two-leaves-in-a-row hand case."""

import numpy as np

from tests.carve_helpers import rig
from tests.octree_lattice_helpers import grid_tree, level_cells, mixed_tree

F = np.float32
OPACITIES = (0.0, 0.3, 1.0, 3.0, 50.0)          # optical depth of one finest side


def densities(scale, depth, count, seed):
    """(count,) f32 drawn from OPACITIES / finest side: transparent, thin, about one e-fold, dense,
    and opaque within a fraction of a cell."""
    side = 2.0 * float(scale) / 2 ** (depth - 1)
    rng = np.random.default_rng(seed)
    return (np.asarray(OPACITIES)[rng.integers(0, len(OPACITIES), count)] / side).astype(F)


def grid_scene(leaves=200, seed=5):
    """``leaves`` cells of the 8^3 grid of a depth-4 tree, scale 1 -> scale, nodes, leaf ids."""
    nodes, ids = grid_tree(4, level_cells(3, np.random.default_rng(seed), leaves))
    return F(1.0), nodes, ids


def mixed_scene():
    return mixed_tree()                          # depth 5, scale 2, leaves of three sizes


def depth_of(leaf_index):
    """1 + the deepest leaf's level."""
    deepest, level, first = int(np.max(leaf_index)), 0, 0
    while deepest >= first + 8 ** level:
        first += 8 ** level
        level += 1
    return level + 1


def camera_arrays(cameras, center):
    """float64 restatement of ``projection_matrices(cameras, origin=center)`` and
    ``eye_positions(cameras, center)``, rounded once -> proj (C,3,4) f32, eyes (C,3) f32."""
    shift = np.eye(4)
    shift[:3, 3] = np.asarray(center, np.float64)
    proj = np.empty((len(cameras), 3, 4), F)
    eyes = np.empty((len(cameras), 3), F)
    for k, cam in enumerate(cameras):
        big = np.eye(4)
        big[:3, :3] = np.asarray(cam.intrinsics, np.float64)
        pose = np.asarray(cam.extrinsics, np.float64)
        proj[k] = (big @ np.linalg.inv(pose) @ shift)[:3]
        eyes[k] = pose[:3, 3] - np.asarray(center, np.float64)
    return proj, eyes


def constant_images(colours, height, width, alpha=255):
    """(C,H,W,4) u8: image c is colours[c] everywhere."""
    colours = np.asarray(colours, np.uint8)
    images = np.zeros((len(colours), height, width, 4), np.uint8)
    images[..., :3] = colours[:, None, None, :]
    images[..., 3] = alpha
    return images


def two_in_a_row(front_density):
    """Depth 2, scale 1, two leaves: the (-,-,-) octant (leaf 0, id 1) and its +x neighbour (leaf 1,
    id 5), and one camera at (-4, 0, 0) looking at the origin.  The ray to leaf 1's centre
    (0.5, -0.5, -0.5) has d = (4.5, -0.5, -0.5): it enters the cube through x = -1 at t = 2/3,
    y = z = -1/3, inside leaf 0, and crosses into leaf 1 at x = 0, t = 8/9: leaf 0 lies in front over
    a chord of (2/9) |d| = 1.012.  The ray to leaf 0's own centre meets leaf 0 first.
    -> scale, nodes, leaf ids, densities (2,), cameras."""
    nodes, ids = grid_tree(2, [(1, 0, 0, 0), (1, 1, 0, 0)])
    assert ids.tolist() == [1, 5]
    return F(1.0), nodes, ids, np.array([front_density, 1.0], F), rig([(-1, 0, 0)], 4.0, 16, 16)
