"""Scenes shared by the K27 box-carve tests (CPU and GPU), on top of ``tests/carve_helpers``: the
nine-camera rig, a thin rod drawn into the masks, the ball, and the cell a point falls into."""

import numpy as np

from tests.carve_helpers import AXIS_EYES, OBLIQUE_EYES, ball_images, rig

ROD = (np.array([-0.7, -0.55, -0.62]), np.array([0.66, 0.71, 0.58]))
SIZE = 32


def cameras9(size=SIZE):
    return rig(AXIS_EYES + OBLIQUE_EYES, 4.0, size, size)


def exact_matrices(cameras):
    """(C,3,4) float64: [[K,0],[0,1]] inv(pose), unrounded."""
    out = []
    for cam in cameras:
        big = np.eye(4)
        big[:3, :3] = np.asarray(cam.intrinsics, np.float64)
        out.append((big @ np.linalg.inv(np.asarray(cam.extrinsics, np.float64)))[:3])
    return np.stack(out)


def nearest_pixels(matrix, points, width, height):
    """float64: on (N) bool (in front and on the image), col, row (N) int64 (0 where not on)."""
    homog = np.concatenate([points, np.ones((len(points), 1))], 1) @ np.asarray(matrix, np.float64).T
    front = homog[:, 2] > 0
    w = np.where(front, homog[:, 2], 1.0)
    fu, fv = homog[:, 0] / w + 0.5, homog[:, 1] / w + 0.5
    on = front & (fu >= 0) & (fu < width) & (fv >= 0) & (fv < height)
    return on, np.where(on, np.floor(fu), 0).astype(np.int64), \
        np.where(on, np.floor(fv), 0).astype(np.int64)


def rod_points(n=4000):
    t = np.linspace(0.0, 1.0, n)[:, None]
    return ROD[0][None, :] * (1 - t) + ROD[1][None, :] * t


def rod_scene(size=SIZE):
    """-> cameras, images (C,H,W,4) u8: the nearest pixels of 4000 points of the rod, opaque."""
    cameras = cameras9(size)
    images = np.zeros((len(cameras), size, size, 4), np.uint8)
    points = rod_points()
    for c, matrix in enumerate(exact_matrices(cameras)):
        on, col, row = nearest_pixels(matrix, points, size, size)
        images[c, row[on], col[on]] = (220, 40, 90, 255)
    return cameras, images


def ball_scene(size=SIZE, radius=0.6):
    cameras = cameras9(size)
    return cameras, ball_images(cameras, radius)


def codes_of_points(points, center, scale, depth):
    """The path code of the finest cell (level depth - 1) of the cube center +- scale that holds
    each point (N,3), float64; the x bit is 4, y 2, z 1, root digit first."""
    side = 2 ** (depth - 1)
    unit = (np.asarray(points, np.float64) - np.asarray(center, np.float64) + scale) / (2 * scale)
    index = np.clip(np.floor(unit * side).astype(np.int64), 0, side - 1)
    codes = np.zeros(len(points), np.int64)
    for level in range(depth - 1):
        shift = depth - 2 - level
        digit = (((index[:, 0] >> shift) & 1) << 2) | (((index[:, 1] >> shift) & 1) << 1) \
            | ((index[:, 2] >> shift) & 1)
        codes = (codes << 3) | digit
    return codes
