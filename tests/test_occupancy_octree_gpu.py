"""K25 on the GPU: ``ffn_occupancy_from_octree`` against the numpy restatement
(tests/occupancy_octree_reference.py), word for word, at the smallest shapes at which the kernels
can go wrong; then through the K9 lookup, the public constructors and ``Raycaster.fit``.

The scan of the row counts works in tiles of 4096 leaves round K9d (one workgroup over the tile
sums): the leaf counts 4095 / 4096 / 4097 and 8193 stand at its tile edges, beside 255 / 256 / 257
(the planning kernel's block edge) and the row totals 2047 / 2048 / 2049.  K9d hands more than one
tile sum to a thread only from 4 194 305 leaves on; that path of K9d is not new here and is left
to the K9 tests that compact more than 2^18 samples."""

import contextlib
import io
import os

import numpy as np
import pytest
import torch

from tests import occupancy_octree_helpers as kh
from tests import occupancy_octree_reference as kref
from tests.octree_lattice_helpers import grid_tree, mixed_tree

pytestmark = pytest.mark.gpu

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scene16.npz")


def dev():
    return torch.device("cuda:0")


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def words(bits):
    return bits.cpu().numpy().view(np.uint32)


def run(ids, place, g, **kwargs):
    from fourier_feature_nets_amd import ops
    scale, center, box_min, box_size = kh.placement(place)
    leaf_index = torch.from_numpy(np.ascontiguousarray(ids)).to(dev())
    return ops.occupancy_from_octree(leaf_index, scale, center, box_min, box_size, g, **kwargs)


# ------------------------------------------------------------------------------ op against restatement
@pytest.mark.parametrize("name", ["root", "three", "mixed", "fine"])
def test_words_equal_the_restatement(name):
    for place in kh.PLACEMENTS:
        for g in kh.RESOLUTIONS + ((4,) if name == "fine" else ()):
            got = words(run(kh.tree(name), place, g))
            assert np.array_equal(got, kh.reference(name, place, g)), (name, place, g)
    assert kh.reference(name, "cube", 64).any()


def test_many_fine_leaves_hit_one_word():
    """300 level-7 leaves under G = 4: two words in all, every leaf one bit of them."""
    want = kh.reference("fine", "cube", 4)
    assert len(want) == 2 and bin(int(want[0])).count("1") + bin(int(want[1])).count("1") > 30
    assert np.array_equal(words(run(kh.tree("fine"), "cube", 4)), want)


@pytest.mark.parametrize("name", ["count255", "count256", "count257", "count4095", "count4096",
                                  "count4097", "count8193", "rows2047", "rows2048", "rows2049"])
def test_block_and_scan_edges(name):
    ids = kh.tree(name)
    rule = kref.Rule()
    scale, center, box_min, box_size = kh.placement("cube")
    marks, i0, i1, _, _ = rule.plan(ids, scale, center, box_min, box_size, 64)
    total = int(rule.rows(marks, i0, i1).sum())
    if name.startswith("count"):
        assert len(ids) == int(name[5:])
    else:
        assert total == int(name[4:])
    for place, g in (("cube", 64), ("small", 33)):
        assert np.array_equal(words(run(ids, place, g)), kh.reference(name, place, g)), (place, g)


def test_root_leaf_fills_a_128_grid():
    """16 384 rows of four whole words."""
    got = words(run(kh.tree("root"), "cube", 128))
    assert got.shape == (65536,) and (got == 0xffffffff).all()
    assert np.array_equal(got, kh.reference("root", "cube", 128))


# ------------------------------------------------------------------------------ density
@pytest.mark.parametrize("stride,offset", [(4, 3), (7, 2), (16, 0)])
def test_density_threshold(stride, offset):
    """Leaves exactly at, just below and just above the threshold, and NaN; the density read at
    ``offset`` of rows of ``stride`` floats (plain and SH device layouts)."""
    ids = kh.tree("mixed")
    density = kh.densities(len(ids))
    assert np.isnan(density).any() and (density == kh.THRESHOLD).any()
    rows = np.random.default_rng(1).random((len(ids), stride)).astype(F) * 4      # decoys
    rows[:, offset] = density
    rows = torch.from_numpy(rows).to(dev())
    for place, g in (("cube", 32), ("small", 33), ("rounded", 31)):
        got = words(run(ids, place, g, rows=rows, stride=stride, sigma_offset=offset,
                        sigma_threshold=float(kh.THRESHOLD)))
        want = kh.reference("mixed", place, g, True)
        assert np.array_equal(got, want), (place, g)
        assert not np.array_equal(want, kh.reference("mixed", place, g))
        # without a threshold the rows are not read
        assert np.array_equal(words(run(ids, place, g, rows=rows, stride=stride, sigma_offset=offset)),
                              kh.reference("mixed", place, g))


# ------------------------------------------------------------------------------ dilation
@pytest.mark.parametrize("dilate", [0, 1, 2, 3])
def test_dilation_lands_in_the_returned_buffer(dilate):
    for name, place, g in (("fine", "cube", 33), ("mixed", "small", 31), ("three", "large", 64)):
        want = kh.reference(name, place, g, False, dilate)
        assert np.array_equal(words(run(kh.tree(name), place, g, dilate=dilate)), want), (name, g)
        if dilate:
            assert not np.array_equal(want, kh.reference(name, place, g, False, dilate - 1))


# ------------------------------------------------------------------------------ accumulation
@pytest.mark.parametrize("dilate", [0, 1, 2])
def test_leaf_halves_fold_into_one_call(dilate):
    ids = kh.tree("mixed")
    for place, g in (("cube", 64), ("small", 33)):
        want = kh.reference("mixed", place, g, False, dilate)
        once = run(ids, place, g, dilate=dilate)
        again = run(ids, place, g, dilate=dilate)
        assert torch.equal(once, again)
        folded = run(ids[::2], place, g, dilate=dilate)
        back = run(ids[1::2], place, g, dilate=dilate, out=folded)
        assert back is folded
        assert np.array_equal(words(folded), want), (place, g)
        assert np.array_equal(words(once), want)


def test_from_octree_folds_and_checks_out():
    import fourier_feature_nets as ffn
    bounds = np.diag([4.0, 4.0, 4.0, 1.0])
    _, nodes, leaves = mixed_tree()
    data = np.zeros((len(leaves), 4), F)
    half = len(leaves) // 2
    parts = []
    for pick in (slice(0, half), slice(half, None)):
        part = ffn.OcTree(2.0, nodes, leaves[pick], data[pick])
        part._center = (0.0, 0.0, 0.0)
        parts.append(part)
    whole = ffn.OcTree(2.0, nodes, leaves, data)
    grid = ffn.OccupancyGrid.from_octree(parts[0], bounds, 32, center=(0, 0, 0))
    assert ffn.OccupancyGrid.from_octree(parts[1], bounds, 32, out=grid) is grid
    want = ffn.OccupancyGrid.from_octree(whole, bounds, 32, center=(0, 0, 0))
    assert torch.equal(grid.bits, want.bits)
    assert np.array_equal(words(want.bits), kh.reference("mixed", "cube", 32, False, 1))
    assert want.fraction_occupied() == kref.cells_of(words(want.bits), 32).mean()
    with pytest.raises(ValueError, match="same box and resolution"):
        ffn.OccupancyGrid.from_octree(parts[1], bounds, 16, out=grid)
    with pytest.raises(ValueError, match="same box and resolution"):
        ffn.OccupancyGrid.from_octree(parts[1], np.diag([4.0, 2.0, 4.0, 1.0]), 32, out=grid)
    with pytest.raises(ValueError, match="root cube's centre"):
        ffn.OccupancyGrid.from_octree(whole, bounds, 32)


def test_from_octree_reads_plain_and_sh_densities():
    """The same densities in an [r, g, b, sigma] tree and in an SH tree (file layout: sigma last;
    device layout: sigma first, padded rows) give the same grid."""
    import fourier_feature_nets as ffn
    _, nodes, leaves = mixed_tree()
    density = kh.densities(len(leaves))
    plain = np.zeros((len(leaves), 4), F)
    plain[:, 3] = density
    sh = np.random.default_rng(2).random((len(leaves), 13)).astype(F)
    sh[:, 12] = density
    bounds = np.diag([4.0, 4.0, 4.0, 1.0])
    want = kh.reference("mixed", "cube", 32, True)
    for tree in (ffn.OcTree(2.0, nodes, leaves, plain), ffn.OcTree(2.0, nodes, leaves, sh, sh_degree=1)):
        grid = ffn.OccupancyGrid.from_octree(tree, bounds, 32, center=(0, 0, 0),
                                             sigma_threshold=float(kh.THRESHOLD), dilate=0)
        assert np.array_equal(words(grid.bits), want)
    shell = ffn.OcTree(2.0, nodes, leaves, plain[:, :3])
    grid = ffn.OccupancyGrid.from_octree(shell, bounds, 32, center=(0, 0, 0), dilate=0)
    assert np.array_equal(words(grid.bits), kh.reference("mixed", "cube", 32))


# ------------------------------------------------------------------------------ through K9
@pytest.mark.parametrize("name", ["root", "three", "mixed", "fine", "count257"])
def test_promised_points_come_back_from_compact(name):
    """Points inside the leaves -- interior, ``lo``, and the neighbours of ``lo`` and ``hi`` -- that
    the guarantee covers all come back from ``grid.compact``; the centre of a cell the
    restatement leaves empty does not."""
    import fourier_feature_nets as ffn
    rule = kref.Rule()
    rng = np.random.default_rng(11)
    ids = kh.tree(name)
    for place in kh.PLACEMENTS:
        scale, center, box_min, box_size = kh.placement(place)
        lo, hi = rule.world_box(scale, center, ids)
        for g in (5, 32, 33):
            grid = ffn.OccupancyGrid(run(ids, place, g), box_min, box_size, g)
            marks, _, _, f_lo, f_hi = rule.plan(ids, scale, center, box_min, box_size, g)
            points, leaf = kref.leaf_points(lo, hi, rng, per_leaf=2)
            keep = kref.promised(rule, points, leaf, marks, f_lo, f_hi, box_min, box_size, g)
            if keep.any():
                sure = torch.from_numpy(points[keep]).to(dev())
                _, _, index = grid.compact(sure, None)
                assert torch.equal(index.cpu(), torch.arange(len(sure), dtype=torch.int32)), (place, g)
            empty = np.argwhere(~kref.cells_of(kh.reference(name, place, g), g))[:, ::-1]
            if len(empty):
                centres = (np.asarray(box_min, np.float64) + (empty + 0.5) * np.asarray(box_size, np.float64) / g)
                centres = torch.from_numpy(np.ascontiguousarray(centres, F)).to(dev())
                assert not kref.occupied_at(kh.reference(name, place, g), centres.cpu().numpy(),
                                            box_min, box_size, g).any()
                assert grid.compact(centres, None)[2].numel() == 0, (place, g)


# ------------------------------------------------------------------------------ the gap
def test_a_leaf_finer_than_a_cell_marks_it_where_cell_centres_miss():
    """One depth-9 leaf (side 1/128 of the cube) off the centre of its G = 16 cell: K25 marks the
    cell; sampling the tree at the cell centres, the composition of public pieces, does not."""
    import fourier_feature_nets as ffn
    nodes, leaves = grid_tree(9, [(8, 3, 70, 201)])
    tree = ffn.OcTree(1.0, nodes, leaves, np.ones((1, 4), F))
    tree._center = (0.0, 0.0, 0.0)
    tree._device = dev()
    bounds = np.diag([2.0, 2.0, 2.0, 1.0])
    g = 16
    grid = ffn.OccupancyGrid.from_octree(tree, bounds, g, dilate=0)
    cells = kref.cells_of(words(grid.bits), g)
    assert cells.sum() == 1 and cells[201 // 16, 70 // 16, 3 // 16]
    centres = ffn.OccupancyGrid.cell_centres(bounds, g, dev())
    hit = tree.query(centres) >= 0
    logits = torch.full((g ** 3, 4), -100.0, device=dev())
    logits[hit, 3] = 100.0
    sampled = ffn.OccupancyGrid.from_logits(logits, bounds, g, 0.01, dilate=False)
    assert not words(sampled.bits).any()


# ------------------------------------------------------------------------------ wiring
def test_fit_trains_under_train_occupancy_from_step_0(golden):
    import fourier_feature_nets_amd as ffn
    from tests.test_pipeline_gpu import _small_model
    torch.manual_seed(5)
    np.random.seed(5)
    model = _small_model(golden("training"))
    train = quiet(ffn.ImageDataset.load, SCENE, "train", 16, True, True, device=dev())
    val = quiet(ffn.ImageDataset.load, SCENE, "val", 16, True, False, device=dev())
    bounds = train.sampler.bounds
    lo, size = ffn.OccupancyGrid.box_of(bounds)
    # five of the eight octants of the box's cube
    nodes, leaves = grid_tree(2, [(1, 0, 0, 0), (1, 1, 0, 1), (1, 1, 1, 1), (1, 0, 1, 0), (1, 1, 1, 0)])
    tree = ffn.OcTree(0.5 * float(size.max()), nodes, leaves)
    grid = ffn.OccupancyGrid.from_octree(tree, bounds, 16, center=tuple(lo + 0.5 * size), dilate=0)
    assert 0.0 < grid.fraction_occupied() < 1.0
    caster = ffn.Raycaster(model)
    assert caster.train_occupancy is None
    caster.train_occupancy = grid
    log = quiet(caster.fit, train, val, 64, 5e-4, 3, 0, 3, 0.1, 25000, 0.0, [])
    assert all(np.isfinite(e.val_psnr) for e in log)
    assert caster.engine.occupancy is grid
    assert 0.0 < caster.engine.last_evaluated_fraction < 1.0
    assert caster.occupancy is None                      # rendering is the caller's to set


def test_from_silhouettes_is_the_carve_then_from_octree():
    import fourier_feature_nets as ffn
    from tests.carve_helpers import AXIS_EYES, OBLIQUE_EYES, Scene, ball_images, rig
    cameras = rig(AXIS_EYES + OBLIQUE_EYES, 4.0, 48, 48)
    scene = Scene(ball_images(cameras, 0.6), cameras)
    bounds = np.array([[2.0, 0, 0, 0.1], [0, 1.6, 0, 0], [0, 0, 2.0, -0.1], [0, 0, 0, 1]])
    grid = ffn.OccupancyGrid.from_silhouettes(scene, bounds, resolution=32, depth=5, min_views=3)
    assert 0.0 < grid.fraction_occupied() < 1.0
    tree = ffn.OcTree.build_from_silhouettes(scene, 5, (0.1, 0.0, -0.1), 1.0, min_views=3)
    again = ffn.OccupancyGrid.from_octree(tree, bounds, 32)
    assert torch.equal(grid.bits, again.bits)
    assert grid.box_min == again.box_min and grid.resolution == 32
    # the ball's centre is inside the hull
    _, _, index = grid.compact(torch.zeros((1, 3), device=dev()), None)
    assert index.numel() == 1
