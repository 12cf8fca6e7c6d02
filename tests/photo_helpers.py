"""Scenes shared by the K28 tests (CPU and GPU): seeded RGBA stacks with alphas round a threshold,
the pixel rays that ``visible_reference.project`` inverts, and the two-blob scene with its phantom
cells."""

import functools

import numpy as np

from tests import octree_render_reference as rref
from tests import octree_walk_reference as wref
from tests.carve_helpers import AXIS_EYES, OBLIQUE_EYES, rig
from tests.octree_lattice_helpers import cell_id, grid_tree
from tests.visible_helpers import densities, grid_scene, mixed_scene

F = np.float32
OPAQUE = 50.0                                   # optical depth of one finest side: a = 1 in f32


def rgba_images(cameras, height, width, seed, alpha_u8):
    """(C,H,W,4) u8: colours uniform, alpha one of 0, ``alpha_u8 - 1``, ``alpha_u8`` and 255 (all
    four present in every image stack)."""
    rng = np.random.default_rng(seed)
    images = rng.integers(0, 256, size=(cameras, height, width, 4), dtype=np.uint8)
    kinds = np.array([0, alpha_u8 - 1, alpha_u8, 255], np.uint8)
    images[..., 3] = kinds[rng.integers(0, 4, (cameras, height, width))]
    assert all((images[..., 3] == k).any() for k in kinds)
    return images


def pixel_rays(camera):
    """The rays through the pixels' centres, row-major: the projection maps a point to pixel
    ``(int)(x / w + 0.5)``, so pixel (col, row) is centred on image coordinate (col, row).
    -> starts, directions (H W, 3) f32."""
    intr = np.asarray(camera.intrinsics, np.float64)
    pose = np.asarray(camera.extrinsics, np.float64)
    res = camera.resolution
    rows, cols = np.meshgrid(np.arange(res.height), np.arange(res.width), indexing="ij")
    local = np.stack([(cols - intr[0, 2]) / intr[0, 0], (rows - intr[1, 2]) / intr[1, 1],
                      np.ones_like(cols, np.float64)], -1).reshape(-1, 3)
    directions = local @ pose[:3, :3].T
    starts = np.broadcast_to(pose[:3, 3], directions.shape)
    return np.ascontiguousarray(starts, F), np.ascontiguousarray(directions, F)


def images_of(render, cameras):
    """``render(starts, directions) -> (color (N,3) in [0,1], alpha (N,))`` per camera ->
    (C,H,W,4) u8: the colour's bytes, alpha 255 on a hit."""
    out = []
    for cam in cameras:
        color, alpha = render(*pixel_rays(cam))
        res = cam.resolution
        rgba = np.concatenate([np.rint(np.asarray(color, np.float64) * 255.0),
                               255.0 * (np.asarray(alpha, np.float64) > 0)[:, None]], 1)
        out.append(rgba.astype(np.uint8).reshape(res.height, res.width, 4))
    return np.stack(out)


def reference_render(scale, nodes, ids, colors):
    """The float64 first hit (tests/octree_render_reference.py) as a ``render`` for ``images_of``:
    what ``OcTree.render`` computes, without a device."""
    def render(starts, directions):
        w = wref.walk(scale, nodes, ids, starts, directions)
        leaf = rref.first_hit(w, scale, ids, starts, directions)["leaf"]
        return np.where(leaf[:, None] >= 0, np.asarray(colors)[np.maximum(leaf, 0)], 0.0), leaf >= 0
    return render


# ------------------------------------------------------------------------------- the moments
NINE = AXIS_EYES + OBLIQUE_EYES
MOMENT_SCENES = {"grid": (grid_scene, 4, NINE[3:9], 4.0), "mixed": (mixed_scene, 5, NINE[4:9], 6.0)}
SEED, ALPHA_U8 = 3, 128


@functools.lru_cache(maxsize=None)
def moment_scene(name):
    """The scenes of the GPU test of the moments: tree, seeded densities, cameras, seeded RGBA
    images of 24 x 20 with alphas 0, 127, 128 and 255."""
    make, depth, eyes, distance = MOMENT_SCENES[name]
    scale, nodes, ids = make()
    cameras = rig(eyes, distance, 24, 20, fov_deg=90.0)
    return (scale, nodes, ids, densities(scale, depth, len(ids), SEED), cameras,
            rgba_images(len(cameras), 20, 24, SEED, ALPHA_U8))


# ------------------------------------------------------------------------------- the two blobs
RED, BLUE = (230, 40, 30), (20, 60, 220)
BLOB_A = [(x, y, z) for x in (1, 2) for y in (3, 4) for z in (3, 4)]
BLOB_B = [(x, y, z) for x in (5, 6) for y in (3, 4) for z in (3, 4)]
# cells of free space that two or more cameras see in front of different blobs (found with the
# reference: tests/test_octree_photo_cpu.py holds the scene to it)
PHANTOMS = [(2, 3, 7), (2, 4, 7), (2, 7, 4), (3, 0, 5), (3, 1, 5), (3, 3, 5), (3, 3, 6), (3, 3, 7),
            (3, 4, 5), (3, 4, 6), (3, 4, 7), (3, 5, 4), (3, 6, 4), (3, 7, 3), (3, 7, 4), (4, 0, 5),
            (4, 1, 5), (4, 3, 5), (4, 3, 6), (4, 3, 7), (4, 4, 5), (4, 4, 6), (4, 4, 7), (4, 5, 4),
            (4, 6, 4), (4, 7, 3), (4, 7, 4), (5, 3, 7), (5, 4, 7), (5, 7, 4)]
EYES = [(0, 0, 1), (0.6, 0, 1), (-0.6, 0, 1), (0, 1, 0.2), (0.6, 1, 0), (-0.6, 1, 0), (0.5, -1, 0.5),
        (-0.5, -1, 0.5), (0, 0.3, -1)]


def blob_rows(cells, phantoms=()):
    """ids and rows ``[r, g, b, sigma]`` of the cells of the depth-4 grid, in id order: the blobs in
    their colours, phantoms grey, all opaque within a fraction of a cell."""
    sigma = OPAQUE / 0.25
    rows = {}
    for cell in cells:
        colour = RED if cell in BLOB_A else BLUE
        rows[cell_id(3, *cell)] = [colour[0] / 255, colour[1] / 255, colour[2] / 255, sigma]
    for cell in phantoms:
        rows[cell_id(3, *cell)] = [0.5, 0.5, 0.5, sigma]
    ids = np.array(sorted(rows), np.int64)
    return ids, np.array([rows[int(i)] for i in ids], F)


@functools.lru_cache(maxsize=None)
def blob_scene():
    """Depth 4, scale 1: two blobs of eight cells each, red and blue, and ``PHANTOMS``.  -> dict:
    ``scale``, the ``true`` tree (nodes, ids, rows), the ``start`` tree (true leaves and phantoms),
    ``phantom_ids`` and the ``cameras``."""
    cameras = rig(EYES, 4.0, 24, 20)
    true_ids, true_rows = blob_rows(BLOB_A + BLOB_B)
    start_ids, start_rows = blob_rows(BLOB_A + BLOB_B, PHANTOMS)
    codes = [(3,) + c for c in BLOB_A + BLOB_B]
    true_nodes, ids = grid_tree(4, codes)
    assert np.array_equal(ids, true_ids)
    start_nodes, ids = grid_tree(4, codes + [(3,) + c for c in PHANTOMS])
    assert np.array_equal(ids, start_ids)
    return dict(scale=F(1.0), true=(true_nodes, true_ids, true_rows),
                start=(start_nodes, start_ids, start_rows),
                phantom_ids=np.array(sorted(cell_id(3, *c) for c in PHANTOMS), np.int64),
                cameras=cameras)
