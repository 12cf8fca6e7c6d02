"""Host side of K23, space carving: ``cameras.projection_matrices`` against ``CameraInfo.project``,
what ``ops.octree_carve_check``, the C ABI and ``OcTree.build_from_silhouettes`` refuse without a
GPU, and the numpy restatement (tests/carve_reference.py) on scenes whose answer is known."""

import ctypes
import os
import sys

import numpy as np
import pytest
import torch

from tests import carve_reference as cref
from tests.carve_helpers import (AXIS_EYES, OBLIQUE_EYES, Scene, ball_images, farthest_depth, rig,
                                 seeded_images, turned_away)

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SYMBOLS = ("ffn_octree_carve_select", "ffn_octree_carve_max_cameras")


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


# ------------------------------------------------------------------------------- projection
def test_projection_matrices_against_camera_project():
    """``projection_matrices`` is float64 arithmetic rounded once; ``CameraInfo.project`` is a float32
    LAPACK inverse of the pose, a float32 4x4 product, a float32 product with the points and a
    float32 division.  With u = 2^-24 and A = |[[K,0],[0,1]]| |inv(E)| |[p, 1]| (the products of the
    absolute values, row by row):

    * the inverse of the 4x4 pose by LU carries a relative error of at most 8 u cond(E) in every
      entry (n = 4, the usual first-order bound with its constant rounded up to 2 n);
    * each of the two f32 products has inner length 4: 4 u each, 8 u together, on A;
    * rounding P once to f32: u on A.

    So a row of ``P [p, 1]`` differs by at most e = (8 cond(E) + 9) u A_row, and the pixel
    coordinate x / w by (e_x + |x / w| e_w) / |w| to first order, plus u |x / w| for the division.
    The test allows exactly that, times 2 for the second-order terms."""
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES + OBLIQUE_EYES, 4.0, 40, 30)
    matrices = ffn.projection_matrices(cameras)
    assert matrices.shape == (len(cameras), 3, 4) and matrices.dtype == F
    rng = np.random.default_rng(7)
    points = (rng.random((500, 3)) * 2 - 1).astype(F)
    homog = np.concatenate([points.astype(np.float64), np.ones((500, 1))], 1)
    u = 2.0 ** -24
    worst = 0.0
    for cam, matrix in zip(cameras, matrices):
        pose = np.asarray(cam.extrinsics, np.float64)
        big = np.eye(4)
        big[:3, :3] = cam.intrinsics
        exact = (big @ np.linalg.inv(pose))[:3]
        assert np.array_equal(bits(matrix), bits(exact.astype(F)))
        got = homog @ matrix.astype(np.float64).T                     # (N,3): x, y, w
        assert (got[:, 2] > 0).all()
        pixel = got[:, :2] / got[:, 2:3]
        absolute = np.abs(homog) @ (np.abs(big) @ np.abs(np.linalg.inv(pose)))[:3].T
        bound = (8 * np.linalg.cond(pose) + 9) * u * absolute
        allowed = 2 * ((bound[:, :2] + np.abs(pixel) * bound[:, 2:3]) / got[:, 2:3]
                       + u * np.abs(pixel))
        error = np.abs(cam.project(points).astype(np.float64) - pixel)
        worst = max(worst, float((error / allowed).max()))
        assert (error <= allowed).all()
        assert allowed.max() < 0.01                # a hundredth of a pixel: the bound says something
    print("largest error / allowed: %.3f" % worst)


# ------------------------------------------------------------------------------- refusals
def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_carve_symbols_are_declared_exported_and_built_without_contraction():
    from fourier_feature_nets_amd import build, ops
    _lib, lib = library()
    assert set(SYMBOLS) <= set(_lib.declared_symbols())
    for name in SYMBOLS:
        assert getattr(lib, name)
    assert build.SOURCES["carve.hip"] == ["-ffp-contract=off"]
    with open(_lib.HEADER_PATH) as f:
        assert "K23" in f.read()
    # 255 C is exact in f32 up to the limit and not one camera further
    limit = ops.octree_carve_max_cameras()
    assert 255 * limit <= 2 ** 24 < 255 * (limit + 1) and limit == 65793


def test_bad_arguments_return_nonzero_without_a_device():
    _, lib = library()
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    lib.ffn_octree_carve_select.restype = ctypes.c_int
    f, i64, i = ctypes.c_float, ctypes.c_int64, ctypes.c_int
    buffer = (ctypes.c_float * 64)()
    base = ctypes.addressof(buffer)
    base += (-base) % 16
    host, odd, byte = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 1)

    def call(images=host, mask=host, proj=host, cameras=2, height=4, width=4, first=0, count=8,
             depth=2, alpha=128, misses=0, views=0, rows=host, out=host, total=host):
        return (images, mask, proj, i(cameras), i(height), i(width), i64(first), i64(count), f(0),
                f(0), f(0), f(1), i(depth), i(alpha), i(misses), i(views), f(1.0), host, host,
                host, rows, None, host, out, total, None)

    for kwargs, why in (({"images": None}, "null argument"), ({"mask": None}, "null argument"),
                        ({"proj": None}, "null argument"), ({"total": None}, "null argument"),
                        ({"images": byte}, "aligned"), ({"rows": odd}, "aligned"),
                        ({"out": odd}, "aligned"), ({"count": 0}, "shape"),
                        ({"first": 1}, "shape"), ({"first": -1}, "shape"),
                        ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
                        ({"cameras": 0}, "cameras"), ({"cameras": 65794}, "cameras"),
                        ({"height": 0}, "height"), ({"width": (1 << 24) + 1}, "width"),
                        ({"alpha": 0}, "alpha_u8"), ({"alpha": 256}, "alpha_u8"),
                        ({"misses": -1}, "max_misses"), ({"views": -1}, "min_views")):
        status = lib.ffn_octree_carve_select(*call(**kwargs))
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and "ffn_octree_carve_select" in text and why in text, (kwargs, text)


def good():
    return dict(images_u8=torch.zeros((3, 5, 7, 4), dtype=torch.uint8),
                mask_u8=torch.zeros((3, 5, 7), dtype=torch.uint8),
                proj=torch.ones((3, 3, 4), dtype=torch.float32), first_code=0, count=8, depth=2,
                alpha_u8=128, max_misses=0, min_views=2)


def test_octree_carve_check_refuses_what_needs_no_device():
    from fourier_feature_nets_amd import ops
    assert ops.octree_carve_check(**good()) == (3, 5, 7)
    nan = torch.ones((3, 3, 4))
    nan[1, 2, 3] = float("nan")
    inf = torch.ones((3, 3, 4))
    inf[0, 0, 0] = float("-inf")
    wide = torch.zeros((3, 5, 7, 8), dtype=torch.uint8)
    for change, why in (
            ({"images_u8": np.zeros((3, 5, 7, 4), np.uint8)}, "images_u8 must be a"),
            ({"images_u8": torch.zeros((3, 5, 7, 4))}, "images_u8 must be a"),
            ({"images_u8": torch.zeros((3, 5, 7, 3), dtype=torch.uint8)}, "images_u8 must be"),
            ({"images_u8": torch.zeros((5, 7, 4), dtype=torch.uint8)}, "images_u8 must be"),
            ({"images_u8": wide[..., ::2]}, "images_u8 must be contiguous"),
            ({"images_u8": torch.zeros((0, 5, 7, 4), dtype=torch.uint8),
              "mask_u8": torch.zeros((0, 5, 7), dtype=torch.uint8),
              "proj": torch.ones((0, 3, 4))}, "0 cameras"),
            ({"mask_u8": torch.zeros((3, 5, 7), dtype=torch.bool)}, "mask_u8 must be a"),
            ({"mask_u8": torch.zeros((3, 7, 5), dtype=torch.uint8)}, "mask_u8 must be"),
            ({"mask_u8": torch.zeros((3, 7, 5), dtype=torch.uint8).transpose(1, 2)},
             "mask_u8 must be contiguous"),
            ({"proj": torch.ones((3, 3, 4), dtype=torch.float64)}, "proj must be a"),
            ({"proj": torch.ones((2, 3, 4))}, "proj must be"),
            ({"proj": torch.ones((3, 4, 4))}, "proj must be"),
            ({"proj": torch.ones((3, 4, 3)).transpose(1, 2)}, "proj must be contiguous"),
            ({"proj": nan}, "NaN or an infinity"), ({"proj": inf}, "NaN or an infinity"),
            ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
            ({"count": 0}, "count"), ({"count": 2 ** 31, "depth": 11}, "fit the scan"),
            ({"first_code": -1}, "first_code"), ({"first_code": 1}, "first_code"),
            ({"alpha_u8": 0}, "alpha_u8"), ({"alpha_u8": 256}, "alpha_u8"),
            ({"max_misses": -1}, "max_misses"), ({"min_views": -1}, "min_views")):
        with pytest.raises(ValueError, match=why):
            ops.octree_carve_check(**{**good(), **change})
    # the check comes first: host tensors never reach a launch
    with pytest.raises(ValueError, match="first_code"):
        ops.octree_carve_select(center=(0, 0, 0), scale=1.0, sigma0=1.0,
                                **{**good(), "first_code": 4})


class Untouched(Scene):
    """A dataset whose sampler (and with it the device) must not be asked for."""

    @property
    def sampler(self):
        raise AssertionError("build_from_silhouettes went to the device before checking")


def test_build_from_silhouettes_refuses_bad_arguments_before_any_device():
    import fourier_feature_nets as ffn
    build = ffn.OcTree.build_from_silhouettes
    cameras = rig(AXIS_EYES[:2], 4.0, 8, 8)
    images = np.zeros((2, 8, 8, 4), np.uint8)
    scene = Untouched(images, cameras)
    for depth in (0, -1, 12):
        with pytest.raises(ValueError, match="build_from_silhouettes: depth"):
            build(scene, depth)
    for kwargs in ({"center": (0, 0)}, {"batch_size": 0}):
        with pytest.raises(ValueError, match="three components"):
            build(scene, 4, **kwargs)
    for value in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="scale"):
            build(scene, 4, scale=value)
    for value in (-0.01, 1.5, float("nan")):
        with pytest.raises(ValueError, match="alpha_threshold"):
            build(scene, 4, alpha_threshold=value)
    for value in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="cell_opacity"):
            build(scene, 4, cell_opacity=value)
    for kwargs in ({"dilate": -1}, {"max_misses": -1}, {"min_views": -1}):
        with pytest.raises(ValueError, match="dilate, max_misses and min_views"):
            build(scene, 4, **kwargs)
    for value in (-1.0, float("nan"), (0.1, -0.1), (0.1, 0.2, 0.3)):
        with pytest.raises(ValueError, match="merge_tolerance"):
            build(scene, 4, merge_tolerance=value)
    with pytest.raises(ValueError, match="dataset.images .* alpha channel"):
        build(Untouched(images[..., :3], cameras), 4)
    with pytest.raises(ValueError, match="dataset.images"):
        build(Untouched(images.astype(np.float32), cameras), 4)
    with pytest.raises(ValueError, match="dataset.color_space must be RGB"):
        build(Untouched(images, cameras, "YCrCb"), 4)
    with pytest.raises(ValueError, match="1 cameras for 2 images"):
        build(Untouched(images, cameras[:1]), 4)
    with pytest.raises(AssertionError, match="went to the device"):        # all checks passed
        build(scene, 4, alpha_threshold=0.0, cell_opacity=0.0, dilate=0, min_views=0,
              merge_tolerance=(0.0, 1e9))


def test_program_parser_defaults():
    sys.path.insert(0, ROOT)
    from scripts import carve_octree
    parser = carve_octree.build_parser()
    args = parser.parse_args(["data.npz", "tree.npz"])
    assert (args.data_path, args.output_path, args.split) == ("data.npz", "tree.npz", "train")
    assert args.voxel_depth == 8 and args.center == [0.0, 0.0, 0.0] and args.scale == 1.0
    assert args.alpha_threshold == 0.5 and args.dilate == 1 and args.max_misses == 0
    assert args.min_views == 2 and args.cell_opacity == 0.5 and args.merge_tolerance is None
    args = parser.parse_args(["d", "t", "--split", "val", "--voxel-depth", "6", "--center", "0.25",
                              "-0.5", "0", "--scale", "0.8", "--alpha-threshold", "0.25",
                              "--dilate", "0", "--max-misses", "2", "--min-views", "3",
                              "--cell-opacity", "0.9", "--merge-tolerance", "0.01", "0.5"])
    assert args.split == "val" and args.voxel_depth == 6 and args.center == [0.25, -0.5, 0.0]
    assert args.scale == 0.8 and args.alpha_threshold == 0.25 and args.dilate == 0
    assert (args.max_misses, args.min_views, args.cell_opacity) == (2, 3, 0.9)
    assert args.merge_tolerance == [0.01, 0.5]
    # the defaults of the program are those of the method
    import inspect
    import fourier_feature_nets as ffn
    sig = inspect.signature(ffn.OcTree.build_from_silhouettes).parameters
    plain = parser.parse_args(["d", "t"])
    for flag, name in (("alpha_threshold", "alpha_threshold"), ("dilate", "dilate"),
                       ("max_misses", "max_misses"), ("min_views", "min_views"),
                       ("cell_opacity", "cell_opacity"), ("merge_tolerance", "merge_tolerance"),
                       ("batch_size", "batch_size"), ("scale", "scale")):
        assert getattr(plain, flag) == sig[name].default
    with pytest.raises(SystemExit):
        parser.parse_args(["d"])


# ------------------------------------------------------------------------------- the restatement
def random_scene(seed, cameras=5, size=16):
    cams = rig((AXIS_EYES + OBLIQUE_EYES)[:cameras], 4.0, size, size)
    import fourier_feature_nets as ffn
    images = seeded_images(cameras, size, size, seed)
    mask = (images[..., 3] >= 128).astype(np.uint8)
    return images, mask, ffn.projection_matrices(cams)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_more_cameras_never_keep_more(seed):
    """max_misses = 0, min_views = 0: a cell kept with cameras 0 .. C-1 has no miss among them, so
    none among 0 .. C-2."""
    images, mask, proj = random_scene(seed)
    depth, cells = 4, 8 ** 3
    kept = []
    for c in range(1, len(proj) + 1):
        codes, _, _ = cref.carve(images[:c], mask[:c], proj[:c], 0, cells, (0, 0, 0), 1.0, depth,
                                 128, 0, 0, 1.0)
        kept.append(set(codes.tolist()))
    for fewer, more in zip(kept, kept[1:]):
        assert more <= fewer
    assert 0 < len(kept[-1]) < len(kept[0]) < cells


@pytest.mark.parametrize("max_misses,min_views", [(0, 0), (0, 2), (1, 3), (2, 5)])
def test_the_early_out_changes_no_kept_row(max_misses, min_views):
    images, mask, proj = random_scene(11)
    mask = (images[..., 3] >= 100).astype(np.uint8)     # some mask pixels have an own alpha < 128
    args = (images, mask, proj, 37, 400, (0.1, -0.2, 0.05), 0.9, 4, 128, max_misses, min_views,
            2.5)
    codes, data, visited = cref.carve(*args, early_out=True)
    codes2, data2, visited2 = cref.carve(*args, early_out=False)
    assert np.array_equal(codes, codes2) and np.array_equal(bits(data), bits(data2))
    assert (visited2 == len(proj)).all() and (visited <= visited2).all()
    assert (visited[codes - 37] == len(proj)).all()            # a kept cell saw the loop through
    assert visited.min() == max_misses + 1 < len(proj)
    assert 0 < len(codes) < 400 and (data[:, 3] == F(2.5)).all()


@pytest.mark.parametrize("dilate", [0, 1])
def test_the_ball_keeps_its_inside(dilate):
    """Discs of a ball of radius r at the origin, drawn analytically for six axis cameras.  The
    nearest pixel of a projected centre lies at most 0.5 sqrt(2) pixels from the projection, and the
    mask reaches ``dilate`` pixels further; k pixels at depth z are k z / f in the world.  With z the
    largest depth of any cell centre from any camera, m = (0.5 sqrt(2) + dilate) z / f is the largest
    displacement rounding and dilation can cause, so a centre within r - m of the origin lands on
    the silhouette in every camera.  (No outer bound: the hull of six views is larger than the
    ball.)"""
    import fourier_feature_nets as ffn
    radius, depth, size = 0.6, 5, 32
    cameras = rig(AXIS_EYES, 4.0, size, size)
    images = ball_images(cameras, radius)
    mask = cref.grow((images[..., 3] >= 128).astype(np.uint8), dilate)
    proj = ffn.projection_matrices(cameras)
    cells = 8 ** (depth - 1)
    centers = cref.cell_centers(0, cells, (0, 0, 0), 1.0, depth).astype(np.float64)
    focal = float(cameras[0].intrinsics[0, 0])
    assert all(float(c.intrinsics[0, 0]) == float(c.intrinsics[1, 1]) == focal for c in cameras)
    margin = (0.5 * np.sqrt(2) + dilate) * farthest_depth(cameras, centers) / focal
    assert 0.0 < margin < radius / 2
    norms = np.linalg.norm(centers, axis=1)
    # the f32 projection moves a centre by some 1e-5 pixels: no centre sits that close to the shell
    assert (np.abs(norms - (radius - margin)) > 1e-3).all()
    codes, data, visited = cref.carve(images, mask, proj, 0, cells, (0, 0, 0), 1.0, depth, 128, 0,
                                      2, 1.0)
    kept = np.zeros(cells, bool)
    kept[codes] = True
    inside = norms <= radius - margin
    assert inside.sum() > 50 and kept[inside].all()
    assert kept.sum() < cells // 4                         # and it did carve
    if dilate == 0:
        # a kept cell projects onto ball pixels only: exactly the ball's colour
        want = (F([200, 120, 40]) * 6 / F(255 * 6)).astype(F)
        assert np.array_equal(bits(data[:, :3]), bits(np.tile(want, (len(data), 1))))


def test_known_colours():
    """Constant images: a cell seen by n cameras with colours c_k gets exactly sum c_k / (255 n), one
    f32 division of two exact integers.  A camera that looks away does not vote, and one whose
    pixels are masked in but whose own alpha is below the threshold counts as seen, not coloured."""
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES[:4], 4.0, 8, 8)
    cameras[1] = turned_away(cameras[1])
    proj = ffn.projection_matrices(cameras)
    images = np.zeros((4, 8, 8, 4), np.uint8)
    colours = np.array([[10, 200, 33], [1, 2, 3], [250, 0, 77], [90, 90, 91]], np.uint8)
    images[..., :3] = colours[:, None, None, :]
    images[..., 3] = np.array([255, 255, 100, 255], np.uint8)[:, None, None]
    mask = np.ones((4, 8, 8), np.uint8)
    depth, cells = 3, 64
    codes, data, visited = cref.carve(images, mask, proj, 0, cells, (0, 0, 0), 0.5, depth, 128, 0, 3,
                                      0.75)
    assert len(codes) == cells and (visited == 4).all()            # three cameras see every cell
    total = colours[0].astype(np.int64) + colours[3]
    want = (total.astype(F) / F(255 * 2)).astype(F)
    assert np.array_equal(bits(data[:, :3]), bits(np.tile(want, (cells, 1))))
    assert (data[:, 3] == F(0.75)).all()
    codes, _, _ = cref.carve(images, mask, proj, 0, cells, (0, 0, 0), 0.5, depth, 128, 0, 4, 0.75)
    assert len(codes) == 0                                         # the fourth never sees a cell
    # nothing coloured: grey
    images[..., 3] = 100
    codes, data, _ = cref.carve(images, mask, proj, 0, cells, (0, 0, 0), 0.5, depth, 128, 0, 3, 0.75)
    assert len(codes) == cells and (data[:, :3] == F(0.5)).all()
    # a threshold the pixels reach: all three vote
    codes, data, _ = cref.carve(images, mask, proj, 0, cells, (0, 0, 0), 0.5, depth, 100, 0, 3, 0.75)
    total = colours[[0, 2, 3]].astype(np.int64).sum(0)
    want = (total.astype(F) / F(255 * 3)).astype(F)
    assert np.array_equal(bits(data[:, :3]), bits(np.tile(want, (cells, 1))))


def test_grow_is_a_square_maximum():
    mask = np.zeros((1, 5, 6), np.uint8)
    mask[0, 2, 3] = 1
    grown = cref.grow(mask, 1)
    assert grown.sum() == 9 and grown[0, 1:4, 2:5].all()
    assert np.array_equal(cref.grow(mask, 0), mask)
    pooled = torch.nn.functional.max_pool2d(torch.from_numpy(mask.astype(np.float32))[:, None], 5,
                                            stride=1, padding=2)[:, 0].numpy()
    assert np.array_equal(cref.grow(mask, 2), pooled.astype(np.uint8))
