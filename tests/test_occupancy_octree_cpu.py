"""K25 without a GPU: the restatement (tests/occupancy_octree_reference.py) keeps its guarantee on
the inputs the GPU tests use, those inputs notice every mutant of the rule, and the host-side
refusals of ``OccupancyGrid.from_octree`` / ``from_silhouettes`` / ``ops.occupancy_from_octree``."""

import numpy as np
import pytest
import torch

from tests import occupancy_octree_helpers as kh
from tests import occupancy_octree_reference as kref
from tests.octree_lattice_helpers import grid_tree, level_cells

F = np.float32
TREES = ("root", "three", "mixed", "fine")


def _cases():
    for name in TREES:
        for place in kh.PLACEMENTS:
            for g in kh.RESOLUTIONS:
                yield name, place, g


# ------------------------------------------------------------------------------ the restatement
def test_no_promised_point_is_missed():
    """Every f32 point with f(lo) <= f(p) < f(hi) for a marking leaf is occupied: interior points,
    lo itself, and the neighbours of lo and hi inside the box."""
    rule = kref.Rule()
    rng = np.random.default_rng(3)
    checked = 0
    for name, place, g in _cases():
        scale, center, box_min, box_size = kh.placement(place)
        ids = kh.tree(name)
        marks, _, _, f_lo, f_hi = rule.plan(ids, scale, center, box_min, box_size, g)
        lo, hi = rule.world_box(scale, center, ids)
        points, leaf = kref.leaf_points(lo, hi, rng)
        keep = kref.promised(rule, points, leaf, marks, f_lo, f_hi, box_min, box_size, g)
        got = kref.occupied_at(kh.reference(name, place, g), points[keep], box_min, box_size, g)
        assert got.all(), (name, place, g, int((~got).sum()))
        checked += int(keep.sum())
    assert checked > 10000


def test_mask_route_equals_cell_by_cell():
    """The word-and-mask route of the restatement against setting the cells one by one."""
    rule = kref.Rule()
    for name, place, g in _cases():
        scale, center, box_min, box_size = kh.placement(place)
        marks, i0, i1, _, _ = rule.plan(kh.tree(name), scale, center, box_min, box_size, g)
        cells = np.zeros((g, g, g), bool)
        for a, b in zip(i0[marks], i1[marks]):
            cells[a[2]:b[2] + 1, a[1]:b[1] + 1, a[0]:b[0] + 1] = True
        assert np.array_equal(kref.words_of(cells), kh.reference(name, place, g)), (name, place, g)
        assert np.array_equal(kref.cells_of(kh.reference(name, place, g), g), cells)


def test_one_bit_per_leaf_on_an_aligned_grid():
    """Bounds cube = root cube (centre 0, scale 1), G = 2^level: every leaf face falls on a cell
    boundary, and the half-open rule marks the leaf's own cell alone."""
    rng = np.random.default_rng(9)
    ids = grid_tree(7, level_cells(6, rng, 2000))[1]
    words = kref.Rule().words(ids, 1.0, (0, 0, 0), (-1, -1, -1), (2, 2, 2), 64)
    assert int(kref.cells_of(words, 64).sum()) == 2000


def test_outside_leaves_mark_nothing():
    """The eight level-1 leaves of the scale-2 cube against boxes beside them: wholly outside, and
    with a face touching the box from outside (f(hi) == 0, f(lo) == G)."""
    ids = np.arange(1, 9, dtype=np.int64)
    rule = kref.Rule()
    for box_min, touching in (((2.0, -2, -2), True), ((-6.0, -2, -2), True), ((2.5, -2, -2), False),
                              ((-2.0, 2.0, -2), True), ((-2.0, -2, -7.0), False)):
        marks, _, _, f_lo, f_hi = rule.plan(ids, 2.0, (0, 0, 0), box_min, (4, 4, 4), 8)
        assert not marks.any()
        assert touching == bool(((f_hi == 0) | (f_lo == 8)).any())
        assert not rule.words(ids, 2.0, (0, 0, 0), box_min, (4, 4, 4), 8).any()
    assert rule.plan(ids, 2.0, (0, 0, 0), (1.5, -2, -2), (4, 4, 4), 8)[0].sum() == 4


# ------------------------------------------------------------------------------ mutants
class ClosedHi(kref.Rule):
    def last_index(self, f_hi, g):
        return np.minimum(np.maximum(np.floor(f_hi), F(0)), F(g - 1)).astype(np.int64)


class OutsideSwapped(kref.Rule):
    def outside(self, f_lo, f_hi, g):
        return (f_hi < F(0)) | (f_lo > F(g))


class CenterIgnored(kref.Rule):
    def world_box(self, scale, center, leaf_index):
        return super().world_box(scale, (0, 0, 0), leaf_index)


class OutsideClamped(kref.Rule):
    def outside(self, f_lo, f_hi, g):
        return np.zeros(f_lo.shape, bool)


class LastWordDropped(kref.Rule):
    def run_masks(self, begin, end):
        return super().run_masks(begin, np.where((end >> 5) > (begin >> 5), (end >> 5 << 5) - 1, end))


class MaskShort(kref.Rule):
    def run_masks(self, begin, end):
        return super().run_masks(begin, np.maximum(begin, end - 1))


class ThresholdStrict(kref.Rule):
    def empty(self, density, sigma_threshold):
        with np.errstate(invalid="ignore"):
            return np.asarray(density, F) < F(sigma_threshold)


class NanDropped(kref.Rule):
    def empty(self, density, sigma_threshold):
        return np.isnan(density) | super().empty(density, sigma_threshold)


def _noticed(rule, with_density):
    for name, place, g in _cases():
        scale, center, box_min, box_size = kh.placement(place)
        ids = kh.tree(name)
        density = kh.densities(len(ids)) if with_density else None
        got = rule.words(ids, scale, center, box_min, box_size, g, density,
                         kh.THRESHOLD if with_density else None)
        if not np.array_equal(got, kh.reference(name, place, g, with_density)):
            return True
    return False


@pytest.mark.parametrize("mutant", [ClosedHi, OutsideSwapped, CenterIgnored, OutsideClamped,
                                    LastWordDropped, MaskShort])
def test_inputs_notice_a_mutant_of_the_geometry(mutant):
    assert _noticed(mutant(), False)


@pytest.mark.parametrize("mutant", [ThresholdStrict, NanDropped])
def test_inputs_notice_a_mutant_of_the_threshold(mutant):
    assert _noticed(mutant(), True)


def test_threshold_rule_on_its_edge_values():
    t = kh.THRESHOLD
    density = np.array([t, np.nextafter(t, F(0)), np.nextafter(t, F(2)), np.nan], F)
    assert kref.Rule().empty(density, t).tolist() == [True, True, False, False]


# ------------------------------------------------------------------------------ host refusals
def _tree(channels=4, center=(0.0, 0.0, 0.0)):
    import fourier_feature_nets as ffn
    nodes, leaves = grid_tree(2, [(1, 0, 0, 0), (1, 1, 0, 1)])
    data = None if channels is None else np.zeros((len(leaves), channels), np.float32)
    tree = ffn.OcTree(1.0, nodes, leaves, data)
    tree._center = center
    return tree


BOUNDS = np.diag([2.0, 2.0, 2.0, 1.0])


def test_from_octree_refuses_by_name():
    import fourier_feature_nets as ffn
    make = ffn.OccupancyGrid.from_octree
    with pytest.raises(ValueError, match="root cube's centre"):
        make(_tree(center=None), BOUNDS)
    with pytest.raises(ValueError, match="three components"):
        make(_tree(), BOUNDS, center=(0, 0))
    with pytest.raises(ValueError, match="sigma_threshold needs a density"):
        make(_tree(channels=3), BOUNDS, sigma_threshold=0.1)
    with pytest.raises(ValueError, match="sigma_threshold needs a density"):
        make(_tree(channels=None), BOUNDS, sigma_threshold=0.1)
    with pytest.raises(ValueError, match="sigma_threshold is NaN"):
        make(_tree(), BOUNDS, sigma_threshold=float("nan"))
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="resolution must lie in 1 .. 1024"):
            make(_tree(), BOUNDS, resolution=bad)
    for bad in (-1, 0.5):
        with pytest.raises(ValueError, match="dilate must be an integer >= 0"):
            make(_tree(), BOUNDS, dilate=bad)
    with pytest.raises(ValueError, match="center must be three finite"):
        make(_tree(), BOUNDS, center=(0, float("inf"), 0))
    words = torch.zeros((kref.num_words(8),), dtype=torch.int32)
    lo, size = ffn.OccupancyGrid.box_of(BOUNDS)
    for out in (ffn.OccupancyGrid(words, lo, size, 16), ffn.OccupancyGrid(words, lo + 0.5, size, 8),
                ffn.OccupancyGrid(words, lo, size * 2, 8), words):
        with pytest.raises(ValueError, match="same box and resolution"):
            make(_tree(), BOUNDS, resolution=8, out=out)


def test_from_silhouettes_refuses_by_name():
    import fourier_feature_nets as ffn
    from tests.carve_helpers import Scene
    scene = Scene(np.zeros((2, 4, 4, 4), np.uint8), [None, None])
    with pytest.raises(ValueError, match="no sampler.bounds; pass bounds"):
        ffn.OccupancyGrid.from_silhouettes(scene)
    for taken in ("center", "scale"):
        with pytest.raises(ValueError, match="%s comes from bounds" % taken):
            ffn.OccupancyGrid.from_silhouettes(scene, BOUNDS, **{taken: 1.0})
    with pytest.raises(ValueError, match="build_from_silhouettes: depth"):
        ffn.OccupancyGrid.from_silhouettes(scene, BOUNDS, depth=0)
    with pytest.raises(ValueError, match="build_from_silhouettes: alpha_threshold"):
        ffn.OccupancyGrid.from_silhouettes(scene, BOUNDS, alpha_threshold=2.0)


def test_op_refuses_by_name():
    from fourier_feature_nets_amd import ops
    ids = torch.arange(1, 9, dtype=torch.int64)
    good = dict(leaf_index=ids, scale=1.0, center=(0, 0, 0), box_min=(-1, -1, -1),
                box_size=(2, 2, 2), resolution=8)
    assert ops.occupancy_from_octree_check(**good) == 16
    rows = torch.zeros((8, 6))
    for change, message in (
            ({"resolution": 0}, "resolution must lie in 1 .. 1024"),
            ({"leaf_index": ids.to(torch.int32)}, "leaf_index must be a"),
            ({"leaf_index": ids[:0]}, "leaf_index must be a"),
            ({"scale": 0.0}, "scale must be finite and positive"),
            ({"scale": float("nan")}, "scale must be finite and positive"),
            ({"box_size": (2, 0, 2)}, "box_size must be positive"),
            ({"box_size": (2, float("inf"), 2)}, "box_size must be three finite"),
            ({"box_min": (0, 0)}, "box_min must be three finite"),
            ({"sigma_threshold": 0.5}, "sigma_threshold needs the leaves' density"),
            ({"rows": rows, "stride": 0}, "stride >= 1"),
            ({"rows": rows, "stride": 6, "sigma_offset": 6}, "sigma_offset < stride"),
            ({"rows": rows, "stride": 4, "sigma_offset": 3}, "rows must be"),
            ({"rows": rows, "stride": 6, "sigma_offset": 5, "sigma_threshold": float("nan")},
             "sigma_threshold is NaN"),
            ({"dilate": -1}, "dilate must be an integer >= 0"),
            ({"out": torch.zeros(15, dtype=torch.int32)}, "out must be the"),
            ({"out": torch.zeros(16, dtype=torch.int64)}, "out must be the")):
        with pytest.raises(ValueError, match=message):
            ops.occupancy_from_octree_check(**dict(good, **change))


def test_cli_flags_exist_and_default_to_off():
    """Without the new flags the drivers' parsers give the values that change nothing."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                    "scripts"))
    try:
        import _cli
    finally:
        sys.path.pop(0)
    parser = _cli.build_parser("t", _cli.TRAIN_COMMON, _cli.SKIP_GRID)
    args = parser.parse_args(["data.npz", "out"])
    assert args.skip_tree is None and args.skip_carve_depth == 0 and args.skip_tree_center is None
    assert args.skip_resolution == 128 and args.skip_dilate == 1

    class Caster:
        train_occupancy = occupancy = train_occupancy_schedule = None

    caster = _cli.apply_skipping(Caster(), args)
    assert caster.train_occupancy is None and caster.occupancy is None
    assert caster.train_occupancy_schedule is None
    args = parser.parse_args(["data.npz", "out", "--skip-tree", "t.npz", "--skip-carve-depth", "6"])
    with pytest.raises(SystemExit, match="two sources of one grid"):
        _cli.apply_skipping(Caster(), args, object())
