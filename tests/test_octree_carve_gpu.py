"""K23 on the device: ``ops.octree_carve_select`` against the numpy restatement
(tests/carve_reference.py) bit for bit at the shapes where the kernel takes another path, the
projection convention against ``CameraInfo.raycast``, ``OcTree.build_from_silhouettes`` end to end on
a small mesh scene, a fit from the carved tree, ``build_from_model`` against its bits from before
the shared tail, and ``scripts/carve_octree.py`` as a program."""

import contextlib
import functools
import io
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import carve_reference as cref
from tests.carve_helpers import (AXIS_EYES, OBLIQUE_EYES, Scene, farthest_depth, rig,
                                 seeded_images, turned_away)
from tests.helpers import GOLDEN, look_at_camera
from tests.octree_walk_helpers import opaque_ball

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda").contiguous()


def same_as_restatement(images, mask, proj, first, count, center, scale, depth, alpha_u8,
                        max_misses, min_views, sigma0=1.25):
    from fourier_feature_nets_amd import ops
    args = (first, count, center, scale, depth, alpha_u8, max_misses, min_views, sigma0)
    want_codes, want_data, want_visited = cref.carve(images, mask, proj, *args)
    codes, data, visited = ops.octree_carve_select(dev(images), dev(mask), dev(proj), *args,
                                                   want_visited=True)
    assert codes.dtype == torch.int32 and data.dtype == torch.float32
    assert codes.shape == (len(want_codes),) and data.shape == (len(want_codes), 4)
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    assert np.array_equal(bits(data.cpu().numpy()), bits(want_data))
    assert np.array_equal(visited.cpu().numpy(), want_visited)
    plain = ops.octree_carve_select(dev(images), dev(mask), dev(proj), *args)
    assert len(plain) == 2 and np.array_equal(plain[0].cpu().numpy(), want_codes)
    assert np.array_equal(bits(plain[1].cpu().numpy()), bits(want_data))
    return want_codes, want_data, want_visited


@functools.lru_cache(maxsize=None)
def nine_cameras(height, width):
    """Six axis cameras and three oblique ones at distance 4; one of them turned away (it sees no
    cell), one moved to the edge of the cube (cells lie behind it: w <= 0)."""
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES + OBLIQUE_EYES, 4.0, width, height)
    cameras[3] = turned_away(cameras[3])
    intr, pose = look_at_camera((0.2, 0.1, -0.6), width, height, 70.0)
    cameras[5] = ffn.CameraInfo.create("inside", ffn.Resolution(width, height), intr, pose)
    return cameras, ffn.projection_matrices(cameras)


def scene(cameras, height, width, seed=5):
    """Seeded RGBA and the mask ``alpha >= 100``: with alpha_u8 = 128 a pixel of alpha 100 is in the
    mask while its own alpha is below the threshold."""
    _, proj = nine_cameras(height, width)
    # the turned-away camera and the one at the cube come first and second when there are few
    order = [3, 5, 0, 8, 1, 2, 4, 6, 7][:cameras]
    images = seeded_images(cameras, height, width, seed)
    mask = (images[..., 3] >= 100).astype(np.uint8)
    return images, mask, np.ascontiguousarray(proj[order])


# ------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("count", [1, 63, 64, 65, 257, 2500])
def test_counts_round_the_wave_the_block_and_the_scan_tile(count):
    images, mask, proj = scene(9, 32, 32)
    codes, data, visited = same_as_restatement(images, mask, proj, 777, count, (0, 0, 0), 1.0, 5,
                                               128, 1, 2)
    if count >= 257:
        assert 0 < len(codes) < count and visited.min() < 9 and visited.max() == 9


@pytest.mark.parametrize("cameras", [1, 3, 9])
@pytest.mark.parametrize("depth", [1, 2, 5])
def test_depths_and_camera_counts(depth, cameras):
    images, mask, proj = scene(cameras, 32, 32)
    cells = 8 ** (depth - 1)
    for max_misses in (0, 1):
        for min_views in (0, 1, cameras):
            same_as_restatement(images, mask, proj, 0, cells, (0, 0, 0), 1.0, depth, 128,
                                max_misses, min_views)


@pytest.mark.parametrize("height,width", [(1, 1), (5, 7), (32, 32)])
def test_image_sizes_and_a_moved_cube(height, width):
    """A non-square image tells rows from columns; the cube is neither centred nor of unit size, so
    the centre chain rounds."""
    images, mask, proj = scene(9, height, width, seed=height)
    center = (0.3, -0.2, 0.1)
    codes, data, visited = same_as_restatement(images, mask, proj, 100, 3000, center, 0.7, 5, 128,
                                               1, 1)
    assert len(codes) > 0
    want = cref.cell_centers(100, 3000, center, 0.7, 5)
    from fourier_feature_nets_amd import ops
    got = ops.octree_cell_centers(100, 3000, center, 0.7, 5, "cuda").cpu().numpy()
    assert np.array_equal(bits(got), bits(want))           # the centres K16a makes


def test_the_scene_has_every_kind_of_camera_and_pixel():
    """What the cases above rely on: a camera that sees no cell, a camera with cells behind it, and
    kept cells whose pixels are all in the mask with an own alpha below the threshold (grey)."""
    images, mask, proj = scene(9, 32, 32)
    points = cref.cell_centers(0, 4096, (0, 0, 0), 1.0, 5)
    seen_by = [cref.project(points, proj[c], 32, 32)[0] for c in range(9)]
    assert not seen_by[0].any() and seen_by[2].all()
    with np.errstate(all="ignore"):
        w = points @ proj[1, 2, :3] + proj[1, 2, 3]
    assert (w <= 0).any() and (w > 0).any() and 0 < seen_by[1].sum() < 4096
    assert ((mask != 0) & (images[..., 3] < 128)).any()
    # one camera, every pixel in the mask, every own alpha below the threshold
    dim = images.copy()
    dim[..., 3] = 100
    codes, data, _ = same_as_restatement(dim[2:3], np.ones_like(mask[2:3]), proj[2:3], 0, 4096,
                                         (0, 0, 0), 1.0, 5, 128, 0, 1)
    assert len(codes) == 4096 and (data[:, :3] == F(0.5)).all() and (data[:, 3] == F(1.25)).all()
    # and with a threshold they reach, the colour of the one pixel
    codes, data, _ = same_as_restatement(dim[2:3], np.ones_like(mask[2:3]), proj[2:3], 0, 4096,
                                         (0, 0, 0), 1.0, 5, 100, 0, 1)
    _, col, row = cref.project(points, proj[2], 32, 32)
    assert np.array_equal(bits(data[:, :3]), bits(dim[2, row, col, :3].astype(F) / F(255)))


def test_cells_exactly_on_the_image_border():
    """An axis-aligned camera at (0, 0, -2) with focal length 16 and principal point 3.5 in an
    8 x 8 image: P = [[16, 0, 3.5, 7], [0, 16, 3.5, 7], [0, 0, 1, 2]].  In the cube of centre
    (0.25, 0, -0.25) at depth 3 the cell centres are x in {-0.5, 0, 0.5, 1}, y in {+-0.25, +-0.75},
    z in {-1, -0.5, 0, 0.5}; every product, sum and quotient below is exact in f32.  At z = 0 (w = 2):
    x = -0.5 gives fu = -8 / 2 + 3.5 + 0.5 = 0, the first column, seen; x = 0.5 gives fu = 8 = W, not
    seen.  With min_views = 1 and a full mask the first is kept and the second is not."""
    proj = np.array([[[16, 0, 3.5, 7], [0, 16, 3.5, 7], [0, 0, 1, 2]]], F)
    images = seeded_images(1, 8, 8, 3, fill=1.0)
    mask = np.ones((1, 8, 8), np.uint8)
    center, depth = (0.25, 0.0, -0.25), 3
    points = cref.cell_centers(0, 64, center, 1.0, depth)
    assert sorted(set(points[:, 0].tolist())) == [-0.5, 0.0, 0.5, 1.0]
    seen, col, row = cref.project(points, proj[0], 8, 8)
    plane = points[:, 2] == 0
    left, right = plane & (points[:, 0] == F(-0.5)), plane & (points[:, 0] == F(0.5))
    assert left.sum() == right.sum() == 4
    # the y of these cells: 16 * (+-0.25, +-0.75) / 2 + 4 = 2, 6 (seen) and -2, 10 (not seen)
    inside = np.abs(points[:, 1]) == F(0.25)
    assert seen[left & inside].all() and (col[left & inside] == 0).all()
    assert not seen[right].any() and not seen[left & ~inside].any()
    codes, data, _ = same_as_restatement(images, mask, proj, 0, 64, center, 1.0, depth, 128, 0, 1)
    kept = np.zeros(64, bool)
    kept[codes] = True
    assert kept[left & inside].all() and not kept[right].any()
    assert np.array_equal(kept, seen)
    # the kept cell's colour is that of column 0
    first = np.nonzero(left & inside)[0][0]
    want = images[0, row[first], 0, :3].astype(F) / F(255)
    assert np.array_equal(bits(data[np.searchsorted(codes, first), :3]), bits(want))


# ------------------------------------------------------------------------------- convention
def test_a_pixels_ray_projects_back_onto_the_pixel():
    """Pixel (x, y) is the ray through the integer coordinates (x, y), forward is w > 0: the point
    two units along the ray of ``CameraInfo.raycast`` projects onto that pixel, through the
    restatement with ``projection_matrices`` and through the kernel (a one-cell grid centred on
    the point, a mask with that one pixel set)."""
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    width, height = 7, 5
    cameras = rig([(1, 0.2, 0.1), (-0.4, 1, 0.3), (0.5, -0.7, -1)], 3.0, width, height)
    proj = ffn.projection_matrices(cameras)
    ys, xs = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    pixels = np.stack([xs.reshape(-1), ys.reshape(-1)], 1)
    images = np.full((1, height, width, 4), 255, np.uint8)
    for index, cam in enumerate(cameras):
        ray = cam.raycast(pixels.astype(F))
        points = (ray.origin + F(2) * ray.direction).astype(F)
        seen, col, row = cref.project(points, proj[index], width, height)
        assert seen.all() and np.array_equal(col, pixels[:, 0]) and np.array_equal(row, pixels[:, 1])
        for k in (0, 9, 17, len(pixels) - 1):
            mask = np.zeros((1, height, width), np.uint8)
            mask[0, pixels[k, 1], pixels[k, 0]] = 1
            codes, _ = ops.octree_carve_select(dev(images), dev(mask), dev(proj[index:index + 1]),
                                               0, 1, tuple(points[k].tolist()), 1.0, 1, 128, 0, 1,
                                               1.0)
            assert codes.cpu().tolist() == [0]
            codes, _ = ops.octree_carve_select(dev(images), dev(1 - mask),
                                               dev(proj[index:index + 1]), 0, 1,
                                               tuple(points[k].tolist()), 1.0, 1, 128, 0, 1, 1.0)
            assert codes.shape[0] == 0


# ------------------------------------------------------------------------------- end to end
DEPTH, SIZE, DISTANCE = 6, 96, 3.0


@functools.lru_cache(maxsize=None)
def torus():
    """The procedural torus as a depth-6 colour tree (every leaf at the finest level), rendered by
    the first-hit walk from eight 96 x 96 cameras as scripts/make_mesh_npz.py renders its frames,
    and the dataset of those frames.  96 pixels, not 64: at distance 3 and 40 degrees a 64-pixel
    frame has a focal length of 88, and the half side of a finest cell (0.025) would span only
    0.58 pixels at the far side of the torus, less than the 0.5 sqrt(2) the covering claim needs;
    at 96 pixels it spans 0.87 (the test asserts the inequality from the cameras)."""
    import fourier_feature_nets as ffn
    truth = ffn.OcTree.build_from_triangles(*ffn.procedural_torus(), DEPTH, 1)
    cameras = rig(AXIS_EYES[:2] + AXIS_EYES[4:] + OBLIQUE_EYES + [(-1, -0.6, -0.9)], DISTANCE, SIZE,
                  SIZE)
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        sampler = ffn.RaySampler(bounds, cameras, 8, device="cuda")
    images = np.zeros((len(cameras), SIZE, SIZE, 4), np.uint8)
    for index in range(len(cameras)):
        color, alpha, _ = truth.render_image(sampler, index, shading="flat", include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.where(alpha > 0, 255, 0)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset("train", images, bounds, cameras, 8, device="cuda")
    return truth, dataset


def carved(**kwargs):
    import fourier_feature_nets as ffn
    truth, dataset = torus()
    return ffn.OcTree.build_from_silhouettes(dataset, DEPTH, truth.center, truth.scale, **kwargs)


def test_build_from_silhouettes_covers_the_mesh_it_was_rendered_from():
    """The ray through the nearest pixel of a leaf's centre passes within 0.5 sqrt(2) pixels of it,
    which at depth z is 0.5 sqrt(2) z / f in the world; when that is less than the half side of a
    finest cell, the ray goes through the leaf's cube, so it hit that leaf or one in front of it and
    the pixel is foreground.  Hence no camera carves a ground-truth leaf, with no dilation at all."""
    import fourier_feature_nets as ffn
    truth, dataset = torus()
    assert (truth.leaf_depths() == DEPTH - 1).all() and truth.num_leaves > 1000
    relative = truth.leaf_centers()
    world = (relative + np.asarray(truth.center, F)).astype(np.float64)
    focal = float(dataset.cameras[0].intrinsics[0, 0])
    half_side = truth.scale / 2 ** (DEPTH - 1)
    footprint = farthest_depth(dataset.cameras, world) / focal           # one pixel, in the world
    assert half_side > 0.5 * np.sqrt(2) * footprint
    assert 0.05 < (dataset.images[..., 3] > 0).mean() < 0.6

    tree = carved(dilate=0)
    assert (tree.query(relative) >= 0).all()
    assert tree.num_leaves >= truth.num_leaves and (tree.leaf_depths() == DEPTH - 1).all()
    assert tree.num_leaves < 8 ** (DEPTH - 1) // 2                       # and it did carve
    assert tree.scale == truth.scale and tree.center == truth.center
    data = tree.leaf_data()
    side = F(2 * truth.scale) / F(2.0 ** (DEPTH - 1))
    sigma0 = F(-np.log1p(-0.5) / np.float64(side))
    assert data.dtype == F and data.shape == (tree.num_leaves, 4)
    assert (data[:, 3] == sigma0).all() and data[:, :3].min() >= 0 and data[:, :3].max() <= 1
    # one cell side starts at the opacity asked for
    assert abs(1 - np.exp(-np.float64(sigma0) * np.float64(side)) - 0.5) < 1e-6

    loaded = ffn.OcTree.load(tree.state_dict)
    assert np.array_equal(loaded.state_dict["leaf_index"], tree.state_dict["leaf_index"])
    assert np.array_equal(bits(loaded.leaf_data()), bits(data))
    sampler = dataset.sampler
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    rays = torch.arange(0, sampler.starts.shape[0], 7, device="cuda")
    out = tree.render_volume((sampler.starts[rays] - shift).contiguous(),
                             sampler.directions[rays].contiguous())
    color, alpha = out.color.cpu().numpy(), out.alpha.cpu().numpy()
    assert np.isfinite(color).all() and 0.05 < (alpha > 0.5).mean() < 0.9

    again = carved(dilate=0)
    small = carved(dilate=0, batch_size=1000)
    for other in (again, small):
        for key in ("node_index", "leaf_index"):
            assert np.array_equal(other.state_dict[key], tree.state_dict[key])
        assert np.array_equal(bits(other.leaf_data()), bits(data))

    merged = carved(dilate=0, merge_tolerance=(1.0, 1e9))
    assert merged.num_leaves < tree.num_leaves and merged.leaf_depths().min() < DEPTH - 1
    assert (merged.query(relative) >= 0).all()
    # the default grows the silhouettes by a pixel: a superset
    grown = carved()
    assert grown.num_leaves > tree.num_leaves
    assert (grown.query(tree.leaf_centers()) >= 0).all()
    # the restatement, fed with the mask the method makes, gives the tree's cells and rows
    mask = cref.grow((dataset.images[..., 3] >= 128).astype(np.uint8), 1)
    proj = ffn.projection_matrices(dataset.cameras)
    codes, rows, _ = cref.carve(dataset.images, mask, proj, 0, 8 ** (DEPTH - 1), truth.center,
                                truth.scale, DEPTH, 128, 0, 2, sigma0)
    ids = np.sort(codes.astype(np.int64) + (8 ** (DEPTH - 1) - 1) // 7)
    assert np.array_equal(grown.state_dict["leaf_index"], ids)
    assert np.array_equal(bits(grown.leaf_data()), bits(rows))          # code order is id order here

    with pytest.raises(ValueError, match="no leaf"):
        carved(min_views=len(dataset.cameras) + 1)


def test_a_fit_starts_from_the_carved_tree():
    import fourier_feature_nets as ffn
    _, dataset = torus()
    tree = carved()
    fitted, log = ffn.fit_octree(tree, dataset, None, batch_size=4096, num_steps=30,
                                 report_interval=10, verbose=False)
    losses = np.array([entry.loss for entry in log])
    print("training loss, first and last of 30 steps: %.5f %.5f" % (losses[0], losses[-1]))
    assert len(log) == 30 and np.isfinite(losses).all()
    assert losses[-1] < losses[0]
    assert np.array_equal(fitted.state_dict["leaf_index"], tree.state_dict["leaf_index"])
    assert np.isfinite(fitted.leaf_data()).all()
    assert not np.array_equal(bits(fitted.leaf_data()), bits(tree.leaf_data()))


# ------------------------------------------------------------------------------- what is shared
@pytest.mark.parametrize("kind", ["plain", "merged"])
def test_build_from_model_keeps_its_bits(kind):
    """``build_from_model`` on the opaque-ball voxel model at depth 5, against the arrays the commit
    before K23 gave on the same model (tests/golden/octree_build_from_model_ball.npz): K16a now
    calls the shared centre function and K16b and the builder share their tails with K23."""
    import fourier_feature_nets as ffn
    golden = np.load(os.path.join(GOLDEN, "octree_build_from_model_ball.npz"))
    tolerance = None if kind == "plain" else (1.0, 1e9)
    tree = ffn.OcTree.build_from_model(opaque_ball(16).to("cuda"), 5, merge_tolerance=tolerance)
    assert np.array_equal(tree.state_dict["leaf_index"], golden[kind + "_leaf_index"])
    assert np.array_equal(tree.state_dict["node_index"], golden[kind + "_node_index"])
    assert np.array_equal(bits(tree.leaf_data()), golden[kind + "_leaf_data"].view(np.uint32))
    assert golden[kind + "_leaf_data"].dtype == F and len(golden[kind + "_leaf_index"]) > 50


# ------------------------------------------------------------------------------- the program
def test_carve_octree_program(tmp_path):
    truth, dataset = torus()
    data_path, tree_path, out_dir = [str(tmp_path / name) for name in ("data.npz", "tree.npz", "out")]
    cameras = dataset.cameras
    count = len(cameras)
    np.savez(data_path, images=dataset.images,
             intrinsics=np.stack([np.asarray(c.intrinsics, F) for c in cameras]),
             extrinsics=np.stack([np.asarray(c.extrinsics, F) for c in cameras]),
             bounds=np.diag([2, 2, 2, 1]).astype(F),
             split_counts=np.array([count - 2, 1, 1], np.int32))
    center = [np.format_float_positional(F(c), trim="0") for c in truth.center]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "carve_octree.py"), data_path,
                          tree_path, "--voxel-depth", str(DEPTH), "--center", *center, "--scale",
                          repr(float(truth.scale))], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    import fourier_feature_nets as ffn
    tree = ffn.OcTree.load(tree_path)
    assert "%d leaves" % tree.num_leaves in res.stdout
    assert "--center " + " ".join(center) in res.stdout
    want = ffn.OcTree.build_from_silhouettes(Scene(dataset.images[:count - 2], cameras[:count - 2]),
                                             DEPTH, truth.center, truth.scale)
    assert np.array_equal(tree.state_dict["leaf_index"], want.state_dict["leaf_index"])
    assert np.array_equal(bits(tree.leaf_data()), bits(want.leaf_data()))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_octree.py"), tree_path,
                          data_path, out_dir, "--center", *center, "--mode", "volume", "--split",
                          "val"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "mean psnr over 1 cameras" in res.stdout
    assert os.path.exists(os.path.join(out_dir, "frame_00000.png"))
