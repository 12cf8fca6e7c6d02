"""K27 on the device: ``ops.octree_carve_box_level`` against the numpy restatement
(tests/carve_box_reference.py), exact codes and bit-equal rows, at the shapes where the kernel and
the scan take another path and on one scene that holds every kind of camera and rectangle; the
kept set against K23's on the device; ``OcTree.build_from_silhouettes(footprint="box")`` coarse to
fine from several start levels; the rod the point carve loses; the float64 guarantee; and the
feature end to end, down to ``scripts/carve_octree.py --footprint box``."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import carve_box_reference as bref
from tests import carve_reference as cref
from tests.carve_box_helpers import (ball_scene, codes_of_points, exact_matrices,
                                     nearest_pixels, rod_points, rod_scene)
from tests.carve_helpers import AXIS_EYES, Scene, ball_images, rig, seeded_images, turned_away
from tests.helpers import look_at_camera

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIGMA0 = 1.25


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda").contiguous()


def same_as_restatement(images, mask, proj, codes, level, center, scale, depth, max_misses,
                        min_views, expand=False, details=None):
    """One call of the op against ``bref.box_level``.  ``codes`` are the candidates, or with
    ``expand`` the parents.  -> the kept codes and rows of the restatement."""
    from fourier_feature_nets_amd import ops
    codes = np.asarray(codes, np.int64)
    tested = ((codes[:, None] << 3) | np.arange(8)[None, :]).reshape(-1) if expand else codes
    keep, data, want_visited = bref.box_level(images, mask, proj, tested, level, center, scale,
                                              depth, 128, max_misses, min_views, SIGMA0)
    if details is not None:
        bref.box_level(images, mask, proj, tested, level, center, scale, depth, 128, max_misses,
                       min_views, SIGMA0, early_out=False, details=details)
    sat = ops.octree_carve_box_tables(dev(mask))
    assert np.array_equal(sat.cpu().numpy().astype(np.int64), bref.tables(mask))
    got, rows, visited = ops.octree_carve_box_level(
        dev(images), sat, dev(proj), dev(codes.astype(np.int32)), level, center, scale, depth, 128,
        max_misses, min_views, SIGMA0, expand=expand, want_visited=True)
    assert got.dtype == torch.int32 and got.shape == (int(keep.sum()),)
    assert np.array_equal(got.cpu().numpy().astype(np.int64), tested[keep])
    assert np.array_equal(visited.cpu().numpy(), want_visited)
    if level == depth - 1:
        assert rows.dtype == torch.float32 and rows.shape == (int(keep.sum()), 4)
        assert np.array_equal(bits(rows.cpu().numpy()), bits(data[keep]))
    else:
        assert rows is None
    return tested[keep], data[keep]


@functools.lru_cache(maxsize=None)
def pictures(cameras, height, width, dilate):
    """``cameras`` of the nine at distance 4.  Alpha: the ball of radius 0.6, with a ring of pixels
    of alpha 100 round it that only a grown mask covers (own alpha below the threshold); seeded
    colours.  Small images are mostly background with seeded foreground pixels."""
    import fourier_feature_nets as ffn
    cams = rig((AXIS_EYES + [(1, 1, 1), (-1, 0.5, 0.8), (0.3, -1, -0.6)])[:cameras], 4.0, width,
               height)
    images = seeded_images(cameras, height, width, 17 + height, fill=0.06)
    if height >= 16:
        ball = ball_images(cams, 0.6)[..., 3]
        ring = cref.grow((ball > 0).astype(np.uint8), 1)
        images[..., 3] = np.where(ball > 0, 255, np.where(ring > 0, 100, 0))
    mask = cref.grow((images[..., 3] >= 128).astype(np.uint8), dilate)
    return images, mask, ffn.projection_matrices(cams)


def subset(n, cells, seed):
    return np.sort(np.random.default_rng(seed).choice(cells, size=n, replace=False))


# ------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 2047, 2048, 2049])
def test_given_lists_round_the_wave_the_block_and_the_scan_tile(count):
    images, mask, proj = pictures(9, 32, 32, 0)
    kept, _ = same_as_restatement(images, mask, proj, subset(count, 4096, count), 4, (0, 0, 0), 1.0,
                                  5, 0, 2)
    if count >= 257:
        assert 0 < len(kept) < count
    # and below the finest level, where no row is written
    same_as_restatement(images, mask, proj, subset(count, 4096, count + 1), 4, (0, 0, 0), 1.0, 6, 0,
                        2)


@pytest.mark.parametrize("parents", [1, 8, 32, 256, 257])
def test_expanded_lists(parents):
    images, mask, proj = pictures(9, 32, 32, 1)
    chosen = subset(parents, 512, parents)
    kept, _ = same_as_restatement(images, mask, proj, chosen, 4, (0, 0, 0), 1.0, 5, 0, 2,
                                  expand=True)
    given, _ = same_as_restatement(images, mask, proj,
                                   ((chosen[:, None] << 3) | np.arange(8)[None, :]).reshape(-1), 4,
                                   (0, 0, 0), 1.0, 5, 0, 2)
    assert np.array_equal(kept, given)
    same_as_restatement(images, mask, proj, chosen, 4, (0, 0, 0), 1.0, 6, 1, 0, expand=True)


@pytest.mark.parametrize("cameras", [1, 3, 9])
@pytest.mark.parametrize("depth", [1, 2, 5])
def test_every_level_of_depths_and_camera_counts(depth, cameras):
    images, mask, proj = pictures(cameras, 32, 32, 0)
    survivors = []
    for level in range(depth):
        kept, _ = same_as_restatement(images, mask, proj, np.arange(8 ** level), level, (0, 0, 0),
                                      1.0, depth, 0, 0)
        survivors.append(len(kept))
    if depth == 5 and cameras == 9:
        assert 0 < survivors[-1] < 4096


CUBES = [((0, 0, 0), 1.0), ((0.3, -0.2, 0.1), 0.7)]


@pytest.mark.parametrize("height,width", [(1, 1), (5, 7), (32, 32)])
@pytest.mark.parametrize("dilate", [0, 1])
def test_image_sizes_cubes_and_slack_against_the_restatement_and_k23(height, width, dilate):
    """Every combination of image size, cube, max_misses, min_views and dilate: the finest level of
    depth 4 against the restatement, one coarse level with it, and against K23 on the device: K27
    keeps a superset, and the rows of the cells both keep are equal bit for bit."""
    from fourier_feature_nets_amd import ops
    images, mask, proj = pictures(9, height, width, dilate)
    depth, cells = 4, 512
    for center, scale in CUBES:
        for max_misses in (0, 1):
            for min_views in (0, 2):
                kept, rows = same_as_restatement(images, mask, proj, np.arange(cells), depth - 1,
                                                 center, scale, depth, max_misses, min_views)
                point, point_rows = ops.octree_carve_select(
                    dev(images), dev(mask), dev(proj), 0, cells, center, scale, depth, 128,
                    max_misses, min_views, SIGMA0)
                point = point.cpu().numpy().astype(np.int64)
                where = np.searchsorted(kept, point)
                assert (where < len(kept)).all() and np.array_equal(kept[where], point)
                assert np.array_equal(bits(rows[where]), bits(point_rows.cpu().numpy()))
                if (height, width) == (1, 1):
                    # a pad of one pixel never fits a one-pixel image: no camera can refute
                    assert len(kept) == cells or min_views > 0
            same_as_restatement(images, mask, proj, np.arange(64), 2, center, scale, depth,
                                max_misses, 0)
    if (height, width) == (32, 32):
        assert len(point) < len(kept) < cells


def test_one_scene_with_every_kind_of_camera_and_rectangle():
    """Cameras: three at distance 3.2 whose 24 x 20 images the cube overflows (rectangles touch
    and cross every border), one turned away (nothing in front), one inside the cube (cells with
    some corners behind it), and one whose first two rows are scaled by 1e30 and whose third by
    1e-30 (all normal numbers), so that w > 0 and x / w overflows: undecided.  Camera 0's mask is one pixel, the corner of a cell's rectangle.  Each
    kind is asserted from the restatement, then the device must agree at every level."""
    import fourier_feature_nets as ffn
    width, height, depth = 24, 20, 4
    cams = rig(AXIS_EYES[:3], 3.2, width, height)
    cams.append(turned_away(cams[1]))
    intr, pose = look_at_camera((0.2, 0.1, -0.6), width, height, 70.0)
    cams.append(ffn.CameraInfo.create("inside", ffn.Resolution(width, height), intr, pose))
    proj = ffn.projection_matrices(cams)
    tiny = proj[2].copy()
    tiny[:2] *= F(1e30)
    tiny[2] *= F(1e-30)
    proj = np.ascontiguousarray(np.concatenate([proj, tiny[None]]))
    assert np.isfinite(proj).all()
    images = seeded_images(len(proj), height, width, 41, fill=0.05)
    images[0, ..., 3] = 0
    mask = (images[..., 3] >= 128).astype(np.uint8)
    cells = np.arange(8 ** (depth - 1))
    first = bref.footprint(bref.cell_points(cells, depth - 1, (0, 0, 0), 1.0), proj[0],
                           bref.tables(mask)[0], width, height, 1)
    chosen = np.nonzero(first["inside"])[0][7]
    images[0, first["r0"][chosen], first["c0"][chosen], 3] = 255
    mask = (images[..., 3] >= 128).astype(np.uint8)

    details = []
    big = 1000000     # max_misses: no cell is rejected, every camera's verdict on every cell counts
    same_as_restatement(images, mask, proj, cells, depth - 1, (0, 0, 0), 1.0, depth, big, 0,
                        details=details)
    assert len(details) == len(proj)
    away, inside_cube, undecided = details[3], details[4], details[5]
    assert (away["front"] == 0).all() and not away["seen"].any() and not away["miss"].any()
    partly = (inside_cube["front"] > 0) & (inside_cube["front"] < 9)
    assert partly.any() and inside_cube["seen"][partly].all() and not inside_cube["miss"][partly].any()
    assert (inside_cube["front"] == 0).any() and (inside_cube["front"] == 9).any()
    assert undecided["undecided"].all() and undecided["seen"].all() and not undecided["miss"].any()
    whole = [(d["front"] == 9) & ~d["undecided"] for d in details[:3]]

    def occurs(test):
        return any(test(d, w).any() for d, w in zip(details[:3], whole))

    assert occurs(lambda d, w: d["inside"] & (d["c0"] == 0))
    assert occurs(lambda d, w: w & (d["c0"] == -1) & ~d["inside"])
    assert occurs(lambda d, w: d["inside"] & (d["c1"] == width - 1))
    assert occurs(lambda d, w: w & (d["c1"] == width) & ~d["inside"])
    assert occurs(lambda d, w: d["inside"] & (d["r0"] == 0))
    assert occurs(lambda d, w: w & (d["r0"] == -1) & ~d["inside"])
    assert occurs(lambda d, w: d["inside"] & (d["r1"] == height - 1))
    assert occurs(lambda d, w: w & (d["r1"] == height) & ~d["inside"])
    assert occurs(lambda d, w: d["miss"]) and occurs(lambda d, w: d["inside"] & ~d["miss"])
    one = details[0]
    assert one["inside"][chosen] and one["count"][chosen] == 1 and not one["miss"][chosen]
    assert mask[0].sum() == 1 and mask[0, one["r0"][chosen], one["c0"][chosen]] == 1
    # the verdicts decide: every level, both slacks, given and expanded
    for level in range(depth):
        for max_misses in (0, 1):
            kept, _ = same_as_restatement(images, mask, proj, np.arange(8 ** level), level,
                                          (0, 0, 0), 1.0, depth, max_misses, 2)
        if level > 0:
            same_as_restatement(images, mask, proj, np.arange(8 ** (level - 1)), level, (0, 0, 0),
                                1.0, depth, 0, 2, expand=True)
    assert 0 < len(kept) < len(cells)


# ------------------------------------------------------------------------------- the method
def build(scene, depth, **kwargs):
    import fourier_feature_nets as ffn
    cameras, images = scene
    kwargs.setdefault("dilate", 0)
    return ffn.OcTree.build_from_silhouettes(Scene(images, cameras), depth, **kwargs)


def same_tree(a, b):
    return (np.array_equal(a.state_dict["leaf_index"], b.state_dict["leaf_index"])
            and np.array_equal(a.state_dict["node_index"], b.state_dict["node_index"])
            and np.array_equal(bits(a.leaf_data()), bits(b.leaf_data())))


def finest_codes(tree, depth):
    assert (tree.leaf_depths() == depth - 1).all()
    return np.asarray(tree.state_dict["leaf_index"], np.int64) - (8 ** (depth - 1) - 1) // 7


@pytest.mark.parametrize("depth,starts", [(5, (0, 1, 2, 4)), (6, (0, 3))])
def test_every_start_level_gives_the_flat_carve(depth, starts):
    import fourier_feature_nets as ffn
    scene = ball_scene()
    images = scene[1]
    mask = (images[..., 3] >= 128).astype(np.uint8)
    side = F(2.0) / F(2.0 ** (depth - 1))
    sigma0 = F(-np.log1p(-0.5) / np.float64(side))
    codes, rows = bref.box_flat(images, mask, ffn.projection_matrices(scene[0]), (0, 0, 0), 1.0,
                                depth, 128, 0, 2, sigma0)
    trees = [build(scene, depth, footprint="box", start_level=s) for s in starts]
    assert np.array_equal(finest_codes(trees[0], depth), codes)
    assert np.array_equal(bits(trees[0].leaf_data()), bits(rows))      # code order is id order here
    for tree in trees[1:]:
        assert same_tree(tree, trees[0])
    # batches: kernel-expanded children of 12 parents per call, and lists of five given cells
    for batch_size in (100, 5) if depth == 5 else (1000,):
        assert same_tree(build(scene, depth, footprint="box", start_level=1,
                               batch_size=batch_size), trees[0])


@pytest.mark.parametrize("depth", [4, 5, 6])
def test_every_rod_cell_is_kept(depth):
    scene = rod_scene()
    cells = np.unique(codes_of_points(rod_points(), (0, 0, 0), 1.0, depth))
    box = finest_codes(build(scene, depth, footprint="box"), depth)
    assert len(np.setdiff1d(cells, box)) == 0 and len(box) < 8 ** (depth - 1)
    try:
        point = finest_codes(build(scene, depth), depth)
    except ValueError as error:        # at depth 4 the point carve loses the rod and all else
        assert "no leaf" in str(error)
        point = np.zeros(0, np.int64)
    assert len(np.setdiff1d(cells, point)) >= 1                    # what the point carve loses
    assert len(np.setdiff1d(point, box)) == 0


@pytest.mark.parametrize("dilate", [0, 1])
def test_float64_guarantee(dilate):
    """20 000 seeded points in the cube.  A point is consistent if, in float64 with the unrounded
    projection, every camera either does not see it or has it on grown-mask foreground at its
    nearest pixel.  The cell of every consistent point is kept (max_misses 0, min_views 0); no
    point is set aside for lying near a pixel border."""
    depth = 5
    cameras, images = scene = ball_scene()
    mask = cref.grow((images[..., 3] >= 128).astype(np.uint8), dilate)
    points = np.random.default_rng(2027).random((20000, 3)) * 2 - 1
    consistent = np.ones(len(points), bool)
    for c, matrix in enumerate(exact_matrices(cameras)):
        on, col, row = nearest_pixels(matrix, points, images.shape[2], images.shape[1])
        consistent &= ~on | (mask[c, row, col] != 0)
    assert consistent.sum() >= 1000
    kept = finest_codes(build(scene, depth, footprint="box", dilate=dilate, min_views=0), depth)
    cells = np.unique(codes_of_points(points[consistent], (0, 0, 0), 1.0, depth))
    assert len(np.setdiff1d(cells, kept)) == 0
    assert len(kept) < 8 ** (depth - 1)


# ------------------------------------------------------------------------------- end to end
def test_point_stays_the_default_and_box_composes():
    import fourier_feature_nets as ffn
    scene = ball_scene()
    depth = 5
    default = build(scene, depth, dilate=1)
    assert same_tree(build(scene, depth, dilate=1, footprint="point", start_level=0), default)
    box = build(scene, depth, dilate=1, footprint="box")
    assert same_tree(build(scene, depth, dilate=1, footprint="box"), box)    # the same bits twice
    assert box.num_leaves > default.num_leaves
    assert (box.query(default.leaf_centers()) >= 0).all()
    # K24 recolours the same cells; the merge passes run on them
    visible = build(scene, depth, dilate=1, footprint="box", color="visible")
    assert np.array_equal(visible.state_dict["leaf_index"], box.state_dict["leaf_index"])
    assert np.isfinite(visible.leaf_data()).all()
    assert np.array_equal(bits(visible.leaf_data()[:, 3]), bits(box.leaf_data()[:, 3]))
    merged = build(scene, depth, dilate=1, footprint="box", color="visible",
                   merge_tolerance=(1.0, 1e9))
    assert merged.num_leaves < box.num_leaves and merged.leaf_depths().min() < depth - 1
    assert (merged.query(box.leaf_centers()) >= 0).all()
    with pytest.raises(ValueError, match="no leaf"):
        build(scene, depth, footprint="box", min_views=len(scene[0]) + 1)
    # the occupancy grid of the box carve has every bit of the point carve's
    bounds = np.diag([2, 2, 2, 1]).astype(F)
    data = Scene(scene[1], scene[0])
    grids = [ffn.OccupancyGrid.from_silhouettes(data, bounds, resolution=32, depth=depth, **extra)
             for extra in ({}, {"footprint": "box"}, {"footprint": "box", "start_level": 1})]
    point_bits, box_bits, again = [g.bits.cpu().numpy() for g in grids]
    assert np.array_equal(point_bits & box_bits, point_bits)
    assert not np.array_equal(point_bits, box_bits) and np.array_equal(box_bits, again)


def test_carve_octree_program_with_the_box_footprint(tmp_path):
    import fourier_feature_nets as ffn
    cameras, images = ball_scene()
    data_path, tree_path = str(tmp_path / "data.npz"), str(tmp_path / "tree.npz")
    count = len(cameras)
    np.savez(data_path, images=images,
             intrinsics=np.stack([np.asarray(c.intrinsics, F) for c in cameras]),
             extrinsics=np.stack([np.asarray(c.extrinsics, F) for c in cameras]),
             bounds=np.diag([2, 2, 2, 1]).astype(F),
             split_counts=np.array([count - 2, 1, 1], np.int32))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "carve_octree.py"), data_path,
                          tree_path, "--voxel-depth", "5", "--footprint", "box", "--start-level",
                          "2"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    tree = ffn.OcTree.load(tree_path)
    assert "%d leaves" % tree.num_leaves in res.stdout
    want = ffn.OcTree.build_from_silhouettes(Scene(images[:count - 2], cameras[:count - 2]), 5,
                                             footprint="box")
    assert np.array_equal(tree.state_dict["leaf_index"], want.state_dict["leaf_index"])
    assert np.array_equal(bits(tree.leaf_data()), bits(want.leaf_data()))
