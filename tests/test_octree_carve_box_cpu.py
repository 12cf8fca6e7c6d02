"""Host side of K27, the conservative coarse-to-fine carve: the symbol and its build flags, what the
C ABI, ``ops.octree_carve_box_check`` and ``OcTree.build_from_silhouettes`` refuse without a GPU,
the programs' flags, and the numpy restatement (tests/carve_box_reference.py) on the rod and ball
scenes: the box carve keeps a superset of the point carve, coarse to fine equals flat, and the rod
that the point carve loses survives whole."""

import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from tests import carve_box_reference as bref
from tests import carve_reference as cref
from tests.carve_box_helpers import ball_scene, codes_of_points, rod_points, rod_scene
from tests.carve_helpers import AXIS_EYES, Scene, rig

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SYMBOL = "ffn_octree_carve_box_level"


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


# ------------------------------------------------------------------------------- symbol, refusals
def test_symbol_is_declared_exported_and_built_without_contraction():
    from fourier_feature_nets_amd import build
    _lib, lib = library()
    assert SYMBOL in set(_lib.declared_symbols())
    assert getattr(lib, SYMBOL)
    assert build.SOURCES["carve_box.hip"] == ["-ffp-contract=off"]
    assert build.SOURCES["carve.hip"] == ["-ffp-contract=off"]
    with open(_lib.HEADER_PATH) as f:
        assert "K27" in f.read()
    with open(os.path.join(build.CSRC, "carve_box.hip")) as f:
        source = f.read()
    code = source[source.index("namespace ffn"):]              # below the header comment
    assert "atomic" not in code and "__shared__" not in code


def test_bad_arguments_return_nonzero_without_a_device():
    _, lib = library()
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    fn = getattr(lib, SYMBOL)
    fn.restype = ctypes.c_int
    f, i64, i = ctypes.c_float, ctypes.c_int64, ctypes.c_int
    buffer = (ctypes.c_float * 64)()
    base = ctypes.addressof(buffer)
    base += (-base) % 16
    host, odd, byte = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 1)

    def call(images=host, sat=host, proj=host, cameras=2, height=4, width=4, cand=host, count=8,
             expand=0, level=1, depth=2, alpha=128, misses=0, views=0, flags=host, rows=host,
             codes=host, out=host, total=host):
        return (images, sat, proj, i(cameras), i(height), i(width), cand, i64(count), i(expand),
                i(level), f(0), f(0), f(0), f(1), i(depth), i(alpha), i(misses), i(views), f(1.0),
                flags, host, host, rows, None, codes, out, total, None)

    for kwargs, why in (({"images": None}, "null argument"), ({"sat": None}, "null argument"),
                        ({"proj": None}, "null argument"), ({"cand": None}, "null argument"),
                        ({"flags": None}, "null argument"), ({"rows": None}, "null argument"),
                        ({"codes": None}, "null argument"), ({"out": None}, "null argument"),
                        ({"total": None}, "null argument"),
                        ({"images": byte}, "aligned"), ({"sat": byte}, "aligned"),
                        ({"cand": byte}, "aligned"), ({"rows": odd}, "aligned"),
                        ({"out": odd}, "aligned"),
                        ({"level": -1}, "level"), ({"level": 2}, "level"),
                        ({"level": 11, "depth": 11}, "level"),
                        ({"count": 0}, "count"), ({"count": -8}, "count"),
                        ({"count": 2 ** 31}, "count"), ({"count": 12, "expand": 1}, "count"),
                        ({"expand": 2}, "expand"), ({"expand": 1, "level": 0}, "expand"),
                        ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
                        ({"cameras": 0}, "cameras"), ({"cameras": 65794}, "cameras"),
                        ({"height": 0}, "height"), ({"width": (1 << 24) + 1}, "width"),
                        ({"height": 1 << 16, "width": 1 << 15}, "height * width"),
                        ({"alpha": 0}, "alpha_u8"), ({"alpha": 256}, "alpha_u8"),
                        ({"misses": -1}, "max_misses"), ({"views": -1}, "min_views")):
        status = fn(*call(**kwargs))
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and SYMBOL in text and why in text, (kwargs, text)


def good():
    return dict(images_u8=torch.zeros((3, 5, 7, 4), dtype=torch.uint8),
                sat=torch.zeros((3, 6, 8), dtype=torch.int32),
                proj=torch.ones((3, 3, 4), dtype=torch.float32),
                candidates=torch.arange(8, dtype=torch.int32), expand=False, level=1, depth=2,
                alpha_u8=128, max_misses=0, min_views=2)


def test_octree_carve_box_check_refuses_what_needs_no_device():
    from fourier_feature_nets_amd import ops
    assert ops.octree_carve_box_check(**good()) == (3, 5, 7, 8)
    assert ops.octree_carve_box_check(**{**good(), "expand": True, "depth": 3})[3] == 64
    nan = torch.ones((3, 3, 4))
    nan[1, 2, 3] = float("nan")
    for change, why in (
            ({"images_u8": np.zeros((3, 5, 7, 4), np.uint8)}, "images_u8 must be a"),
            ({"images_u8": torch.zeros((3, 5, 7, 3), dtype=torch.uint8)}, "images_u8 must be"),
            ({"sat": torch.zeros((3, 6, 8), dtype=torch.int64)}, "sat must be a"),
            ({"sat": torch.zeros((3, 5, 7), dtype=torch.int32)}, "sat must be"),
            ({"sat": torch.zeros((3, 8, 6), dtype=torch.int32).transpose(1, 2)},
             "sat must be contiguous"),
            ({"proj": torch.ones((2, 3, 4))}, "proj must be"),
            ({"proj": nan}, "NaN or an infinity"),
            ({"candidates": torch.arange(8, dtype=torch.int64)}, "candidates must be a"),
            ({"candidates": torch.zeros((8, 1), dtype=torch.int32)}, "candidates must be"),
            ({"candidates": torch.arange(16, dtype=torch.int32)[::2]},
             "candidates must be contiguous"),
            ({"candidates": torch.zeros((0,), dtype=torch.int32)}, "count = 0"),
            ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
            ({"level": -1}, "level"), ({"level": 2}, "level"),
            ({"expand": True, "level": 0}, "expand"),
            ({"alpha_u8": 0}, "alpha_u8"), ({"alpha_u8": 256}, "alpha_u8"),
            ({"max_misses": -1}, "max_misses"), ({"min_views": -1}, "min_views")):
        with pytest.raises(ValueError, match=why):
            ops.octree_carve_box_check(**{**good(), **change})
    # the check comes first: host tensors never reach a launch
    with pytest.raises(ValueError, match="level"):
        ops.octree_carve_box_level(center=(0, 0, 0), scale=1.0, sigma0=1.0,
                                   **{k: v for k, v in {**good(), "level": 5}.items()})
    # the table on the host, against the restatement's
    mask = (np.random.default_rng(3).random((2, 5, 7)) < 0.4).astype(np.uint8)
    sat = ops.octree_carve_box_tables(torch.from_numpy(mask))
    assert sat.dtype == torch.int32 and tuple(sat.shape) == (2, 6, 8)
    assert np.array_equal(sat.numpy().astype(np.int64), bref.tables(mask))
    with pytest.raises(ValueError, match="mask_u8"):
        ops.octree_carve_box_tables(torch.zeros((2, 5, 7)))


class Untouched(Scene):
    """A dataset whose sampler (and with it the device) must not be asked for."""

    @property
    def sampler(self):
        raise AssertionError("build_from_silhouettes went to the device before checking")


def test_build_from_silhouettes_refuses_footprint_and_start_level_before_any_device():
    import fourier_feature_nets as ffn
    build = ffn.OcTree.build_from_silhouettes
    scene = Untouched(np.zeros((2, 8, 8, 4), np.uint8), rig(AXIS_EYES[:2], 4.0, 8, 8))
    for value in ("Box", "sphere", None, 1):
        with pytest.raises(ValueError, match="footprint is 'point' or 'box'"):
            build(scene, 4, footprint=value)
    for value in (-1, 1.5, "2", True):
        with pytest.raises((ValueError, TypeError), match="start_level"):
            build(scene, 4, footprint="box", start_level=value)
    for kwargs in ({"footprint": "box", "start_level": 9}, {"footprint": "point", "start_level": -3},
                   {"footprint": "box", "start_level": 0}):
        with pytest.raises(AssertionError, match="went to the device"):    # all checks passed
            build(scene, 4, **kwargs)
    sig = inspect.signature(build).parameters
    assert sig["footprint"].default == "point" and sig["start_level"].default == 4


def test_programs_take_the_footprint():
    sys.path.insert(0, ROOT)
    from scripts import _cli, carve_octree
    parser = carve_octree.build_parser()
    plain = parser.parse_args(["d", "t"])
    assert plain.footprint == "point" and plain.start_level == 4
    args = parser.parse_args(["d", "t", "--footprint", "box", "--start-level", "2"])
    assert args.footprint == "box" and args.start_level == 2
    with pytest.raises(SystemExit):
        parser.parse_args(["d", "t", "--footprint", "disc"])
    drivers = _cli.build_parser("t", _cli.TRAIN_COMMON, _cli.SKIP_GRID, _cli.FOCUS_TREE)
    known = drivers.parse_args(["d", "r"])
    assert known.skip_carve_footprint == "point" and known.focus_carve_footprint == "point"
    assert _cli.carve_footprint(known, "skip") == {} and _cli.carve_footprint(known, "focus") == {}
    known = drivers.parse_args(["d", "r", "--skip-carve-footprint", "box", "--focus-carve-footprint",
                                "box"])
    assert _cli.carve_footprint(known, "skip") == {"footprint": "box"}
    assert _cli.carve_footprint(known, "focus") == {"footprint": "box"}


# ------------------------------------------------------------------------------- the restatement
ARGS = dict(center=(0, 0, 0), scale=1.0, alpha_u8=128, max_misses=0, min_views=2, sigma0=1.0)


def scene_arrays(scene):
    import fourier_feature_nets as ffn
    cameras, images = scene
    mask = (images[..., 3] >= 128).astype(np.uint8)
    return images, mask, ffn.projection_matrices(cameras)


@pytest.fixture(scope="module")
def ball():
    return scene_arrays(ball_scene())


@pytest.fixture(scope="module")
def rod():
    return scene_arrays(rod_scene())


@pytest.fixture(scope="module")
def flat_ball(ball):
    return {depth: bref.box_flat(*ball, depth=depth, **ARGS) for depth in (4, 5, 6)}


@pytest.mark.parametrize("depth", [5, 6])
def test_box_keeps_a_superset_of_point_with_the_same_rows(ball, flat_ball, depth):
    images, mask, proj = ball
    point, point_data, _ = cref.carve(images, mask, proj, 0, 8 ** (depth - 1), (0, 0, 0), 1.0,
                                      depth, 128, 0, 2, 1.0)
    box, box_data = flat_ball[depth]
    print("depth %d: box keeps %d, point %d of %d" % (depth, len(box), len(point),
                                                      8 ** (depth - 1)))
    assert 0 < len(point) < len(box) < 8 ** (depth - 1)
    where = np.searchsorted(box, point)
    assert (where < len(box)).all() and np.array_equal(box[where], point)
    assert np.array_equal(bits(box_data[where]), bits(point_data))


@pytest.mark.parametrize("depth", [4, 5, 6])
def test_coarse_to_fine_equals_flat(ball, flat_ball, depth):
    flat, flat_data = flat_ball[depth]
    for start in sorted({0, 1, 2, depth - 2}):
        visits = []
        codes, data = bref.box_carve(*ball, depth=depth, start_level=start, visits=visits, **ARGS)
        assert np.array_equal(codes, flat) and np.array_equal(bits(data), bits(flat_data)), start
        assert visits[0] == 8 ** start and len(visits) == depth - start
    # from the root the carve visits fewer cells than there are finest cells, once the pad (one
    # pixel per level, and a 32-pixel image) lets a coarse level reject anything: from depth 5
    visits = []
    bref.box_carve(*ball, depth=depth, start_level=0, visits=visits, **ARGS)
    print("depth %d: visited %d cells of %d finest" % (depth, sum(visits), 8 ** (depth - 1)))
    assert depth < 5 or sum(visits) < 8 ** (depth - 1)


@pytest.mark.parametrize("depth", [4, 5, 6])
def test_the_rod_survives_the_box_carve_and_not_the_point_carve(rod, depth):
    images, mask, proj = rod
    cells = np.unique(codes_of_points(rod_points(), (0, 0, 0), 1.0, depth))
    point, _, _ = cref.carve(images, mask, proj, 0, 8 ** (depth - 1), (0, 0, 0), 1.0, depth, 128, 0,
                             2, 1.0)
    lost = np.setdiff1d(cells, point)
    print("depth %d: the rod passes through %d cells, the point carve loses %d"
          % (depth, len(cells), len(lost)))
    assert len(lost) >= 1                          # the scene discriminates
    for start in (0, depth - 1):
        box, _ = bref.box_carve(images, mask, proj, depth=depth, start_level=start, **ARGS)
        assert len(np.setdiff1d(cells, box)) == 0, start
        assert len(box) < 8 ** (depth - 1)         # and the carve did carve
