"""Small scenes shared by the K23 space-carving tests (CPU and GPU): camera rigs, analytic ball
silhouettes, seeded RGBA stacks, and a stand-in for the dataset ``build_from_silhouettes`` reads."""

import numpy as np

from tests.helpers import look_at_camera

AXIS_EYES = [(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)]
OBLIQUE_EYES = [(1, 1, 1), (-1, 0.5, 0.8), (0.3, -1, -0.6)]


class Scene:
    """What ``OcTree.build_from_silhouettes`` reads of a dataset."""

    def __init__(self, images, cameras, color_space="RGB"):
        self.images, self.cameras, self.color_space = images, cameras, color_space


def rig(eyes, distance, width, height, fov_deg=40.0):
    """Cameras at ``distance`` along ``eyes``, looking at the origin."""
    import fourier_feature_nets as ffn
    cameras = []
    for k, eye in enumerate(eyes):
        eye = np.asarray(eye, np.float64)
        intr, pose = look_at_camera(eye * distance / np.linalg.norm(eye), width, height, fov_deg)
        cameras.append(ffn.CameraInfo.create("c%d" % k, ffn.Resolution(width, height), intr, pose))
    return cameras


def turned_away(camera):
    """The same eye, looking the other way: the origin and the cube round it lie behind it."""
    import fourier_feature_nets as ffn
    pose = np.array(camera.extrinsics, np.float32)
    pose[:3, 0] = -pose[:3, 0]
    pose[:3, 2] = -pose[:3, 2]
    return ffn.CameraInfo.create(camera.name + "away", camera.resolution, camera.intrinsics, pose)


def ball_images(cameras, radius, color=(200, 120, 40)):
    """RGBA images of a ball of ``radius`` at the origin, for cameras that look at the origin: pixel
    (x, y) is set iff the ray through (x, y) meets the ball, that is iff the squared tangent of its
    angle to the optical axis is at most r^2 / (d^2 - r^2).  float64, from the intrinsics."""
    res = cameras[0].resolution
    images = np.zeros((len(cameras), res.height, res.width, 4), np.uint8)
    ys, xs = np.meshgrid(np.arange(res.height), np.arange(res.width), indexing="ij")
    for k, cam in enumerate(cameras):
        intr = np.asarray(cam.intrinsics, np.float64)
        d2 = float((np.asarray(cam.extrinsics, np.float64)[:3, 3] ** 2).sum())
        tan2 = ((xs - intr[0, 2]) / intr[0, 0]) ** 2 + ((ys - intr[1, 2]) / intr[1, 1]) ** 2
        inside = tan2 <= radius ** 2 / (d2 - radius ** 2)
        images[k, inside, :3] = color
        images[k, inside, 3] = 255
    return images


def seeded_images(cameras, height, width, seed, fill=0.6):
    """(C,H,W,4) u8: colours uniform, alpha one of 0 / 100 / 255 -- background, a pixel below a
    threshold of 128 that a grown mask can still cover, and foreground."""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(cameras, height, width, 4), dtype=np.uint8)
    kind = rng.random((cameras, height, width))
    images[..., 3] = np.where(kind < fill, 255, np.where(kind < fill + 0.15, 100, 0))
    return images


def farthest_depth(cameras, points):
    """The largest distance along an optical axis from any camera to any of ``points`` (N,3)."""
    deepest = 0.0
    for cam in cameras:
        pose = np.asarray(cam.extrinsics, np.float64)
        deepest = max(deepest, float(((points - pose[:3, 3]) @ pose[:3, 2]).max()))
    return deepest
