"""K24 on the device: ``ops.octree_visible_votes`` against the numpy restatement
(tests/visible_reference.py) on the decided pairs, votes equal as integers, at the shapes where the
kernel can go wrong (leaf counts round the 64-lane workgroup, camera counts, image sizes, alpha
thresholds, tree depths, transmittance thresholds), the hand cases, exactness over split calls, SH
rows, ``OcTree.color_from_images``, ``OcTree.build_from_silhouettes(color=...)`` and the two programs."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import visible_reference as vref
from tests.carve_helpers import (AXIS_EYES, OBLIQUE_EYES, Scene, ball_images, rig, seeded_images,
                                 turned_away)
from tests.helpers import look_at_camera
from tests.octree_lattice_helpers import grid_tree, level_cells
from tests.visible_helpers import (constant_images, densities, depth_of, grid_scene, mixed_scene,
                                   two_in_a_row)

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NINE = AXIS_EYES + OBLIQUE_EYES


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to("cuda").contiguous()


def plain_rows(density):
    rows = np.zeros((len(density), 4), F)
    rows[:, :3] = 0.5
    rows[:, 3] = density
    return rows


def arrays(cameras, center=(0, 0, 0)):
    import fourier_feature_nets as ffn
    return ffn.projection_matrices(cameras, origin=center), ffn.eye_positions(cameras, center)


def kernel(scale, nodes, ids, rows, images, proj, eyes, alpha_u8, tau, stride=4, offset=3,
           out=None):
    from fourier_feature_nets_amd import ops
    leaf_index = dev(np.asarray(ids, np.int64))
    centers, _ = ops.octree_leaf_geometry(leaf_index, float(scale))
    votes = ops.octree_visible_votes(centers, float(scale), depth_of(ids),
                                     dev(np.asarray(nodes, np.int64)), leaf_index, dev(rows), stride,
                                     offset, dev(images), dev(proj), dev(eyes), alpha_u8, tau,
                                     out=out)
    assert votes.dtype == torch.uint32 and votes.shape == (len(ids), 4)
    return votes


def against_reference(scale, nodes, ids, density, images, cameras, alpha_u8, tau):
    """The kernel's votes equal the restatement's, as integers, on every leaf none of whose pairs
    is undecided; at most 1 % of the pairs are undecided."""
    proj, eyes = arrays(cameras)
    want = vref.visible(scale, nodes, ids, density, images, proj, eyes, alpha_u8, tau)
    got = kernel(scale, nodes, ids, plain_rows(density), images, proj, eyes, alpha_u8,
                 tau).cpu().numpy().astype(np.int64)
    undecided = int(want["undecided"].sum())
    print("%d leaves x %d cameras: %d undecided, %d candidates, %d visible"
          % (len(ids), len(cameras), undecided, int(want["candidate"].sum()),
             int(want["visible"].sum())))
    assert undecided <= 0.01 * want["pairs"]
    sure = ~want["undecided"].any(1)
    assert np.array_equal(got[sure], want["votes"][sure])
    # an undecided pair may go either way, and only that pair
    lo = want["votes"][~sure][:, 3]
    assert ((got[~sure][:, 3] >= lo) & (got[~sure][:, 3] <= lo + want["undecided"][~sure].sum(1))).all()
    return want, got


@functools.lru_cache(maxsize=None)
def grid_case(leaves):
    scale, nodes, ids = grid_scene(leaves, seed=leaves)
    return scale, nodes, ids, densities(scale, 4, leaves, 7)


# ------------------------------------------------------------------------------- the shapes
@pytest.mark.parametrize("leaves", [1, 63, 64, 65, 257])
def test_leaf_counts_round_the_workgroup(leaves):
    scale, nodes, ids, density = grid_case(leaves)
    cameras = rig(NINE, 4.0, 32, 32, fov_deg=90.0)
    want, _ = against_reference(scale, nodes, ids, density, seeded_images(9, 32, 32, leaves),
                                cameras, 128, 0.3)
    if leaves > 1:
        assert 0 < want["visible"].sum() < want["candidate"].sum() < want["pairs"]


def test_a_tree_with_leaves_of_three_sizes():
    scale, nodes, ids = mixed_scene()
    density = densities(scale, 5, len(ids), 3)
    cameras = rig(NINE, 6.0, 32, 32, fov_deg=90.0)
    want, _ = against_reference(scale, nodes, ids, density, seeded_images(9, 32, 32, 2), cameras,
                                128, 0.3)
    assert 0.1 < want["visible"].sum() / want["candidate"].sum() < 0.9


@pytest.mark.parametrize("count", [1, 3, 9])
def test_camera_counts(count):
    scale, nodes, ids, density = grid_case(65)
    cameras = rig(NINE[:count], 4.0, 32, 32, fov_deg=90.0)
    against_reference(scale, nodes, ids, density, seeded_images(count, 32, 32, 11), cameras, 128, 0.3)


@pytest.mark.parametrize("height,width", [(1, 1), (5, 7), (32, 32)])
def test_image_sizes(height, width):
    scale, nodes, ids, density = grid_case(65)
    cameras = rig(NINE, 4.0, width, height, fov_deg=90.0)
    want, _ = against_reference(scale, nodes, ids, density, seeded_images(9, height, width, 13),
                                cameras, 128, 0.3)
    assert want["candidate"].any()


@pytest.mark.parametrize("alpha_u8", [100, 101, 255])
def test_alpha_thresholds(alpha_u8):
    """``seeded_images`` holds alphas 0, 100 and 255: 100 takes the middle kind in, 101 does not."""
    scale, nodes, ids, density = grid_case(65)
    cameras = rig(NINE, 4.0, 32, 32, fov_deg=90.0)
    images = seeded_images(9, 32, 32, 17)
    want, _ = against_reference(scale, nodes, ids, density, images, cameras, alpha_u8, 0.3)
    # a candidate is a pair whose pixel reaches the threshold: alpha 100 counts at 100 alone
    proj, _ = arrays(cameras)
    reach = np.zeros((65, 9), bool)
    for c in range(9):
        ok, col, row = vref.project(vref.centers_of(scale, ids), proj[c], 32, 32)
        reach[:, c] = ok & (images[c, row, col, 3] >= (100 if alpha_u8 == 100 else 255))
    assert np.array_equal(want["candidate"], reach) and reach.any() and not reach.all()


@pytest.mark.parametrize("depth", [1, 2, 5])
def test_tree_depths(depth):
    if depth == 1:
        scale, nodes, ids = F(1.0), np.zeros(0, np.int64), np.zeros(1, np.int64)
    elif depth == 2:
        nodes, ids = grid_tree(2, level_cells(1))
        scale = F(1.0)
    else:
        scale, nodes, ids = mixed_scene()
    density = densities(scale, depth, len(ids), 19)
    cameras = rig(NINE, 3.0 * float(scale), 32, 32, fov_deg=90.0)
    against_reference(scale, nodes, ids, density, seeded_images(9, 32, 32, 23, fill=0.9), cameras,
                      128, 0.3)


@pytest.mark.parametrize("tau", [0.0, 0.3, 0.9])
def test_transmittance_thresholds(tau):
    scale, nodes, ids, density = grid_case(257)
    cameras = rig(NINE[:3], 4.0, 32, 32, fov_deg=90.0)
    images = constant_images([[9, 8, 7], [1, 2, 3], [250, 251, 252]], 32, 32)
    want, _ = against_reference(scale, nodes, ids, density, images, cameras, 128, tau)
    assert want["candidate"].all() and 0 < want["visible"].sum() < want["pairs"]


# ------------------------------------------------------------------------------- hand cases
@pytest.mark.parametrize("front,occludes", [(50.0, True), (0.0, False), (-3.0, False),
                                            (float("nan"), False)])
def test_two_leaves_in_a_row(front, occludes):
    scale, nodes, ids, density, cameras = two_in_a_row(front)
    proj, eyes = arrays(cameras)
    images = constant_images([[7, 8, 9]], 16, 16)
    got = kernel(scale, nodes, ids, plain_rows(density), images, proj, eyes, 1, 0.3).cpu().numpy()
    assert got.tolist() == [[7, 8, 9, 1], [0, 0, 0, 0] if occludes else [7, 8, 9, 1]]
    if occludes:        # exp(-50.6) rounds f32's a to exactly 1: T is 0, occluded at tau = 0 too
        got = kernel(scale, nodes, ids, plain_rows(density), images, proj, eyes, 1, 0.0)
        assert got.cpu().numpy().tolist() == [[7, 8, 9, 1], [0, 0, 0, 0]]


def axis_camera(cx, cy, width, height):
    """At (0, 0, -4) looking along +z, the principal point moved to (cx, cy): the origin projects
    to exactly (cx, cy), so fu = cx + 0.5 and fv = cy + 0.5 with no rounding."""
    import fourier_feature_nets as ffn
    intr, pose = look_at_camera((0, 0, -4), width, height)
    intr = np.array(intr, F)
    intr[0, 2], intr[1, 2] = cx, cy
    return ffn.CameraInfo.create("axis", ffn.Resolution(width, height), intr, pose)


def test_a_centre_that_projects_exactly_onto_a_border():
    """fu = 0 is the first column and fu = W is outside, fv likewise: ``0 <= fu < W``."""
    width, height = 6, 4
    nodes, ids, rows = np.zeros(0, np.int64), np.zeros(1, np.int64), plain_rows(np.ones(1, F))
    images = np.zeros((1, height, width, 4), np.uint8)
    images[0, :, :, 0] = np.arange(width)[None, :] + 1
    images[0, :, :, 1] = np.arange(height)[:, None] + 1
    images[..., 3] = 255
    for cx, cy, want in ((-0.5, -0.5, [1, 1, 0, 1]), (width - 1.5, height - 1.5, [width, height, 0, 1]),
                         (width - 0.5, 1.0, [0, 0, 0, 0]), (1.0, height - 0.5, [0, 0, 0, 0]),
                         (-0.75, 1.0, [0, 0, 0, 0]), (1.0, -0.75, [0, 0, 0, 0])):
        cameras = [axis_camera(cx, cy, width, height)]
        proj, eyes = arrays(cameras)
        ref = vref.visible(1.0, nodes, ids, [1.0], images, proj, eyes, 128, 0.3)
        assert ref["votes"][0].tolist() == want, (cx, cy)
        got = kernel(1.0, nodes, ids, rows, images, proj, eyes, 128, 0.3).cpu().numpy()
        assert got[0].tolist() == want, (cx, cy)


def test_a_camera_inside_the_target_leaf_and_one_behind_it():
    scale, nodes, ids, density, cameras = two_in_a_row(50.0)
    inside = rig([(-1, -1, -1)], 0.9 * np.sqrt(3.0), 32, 32, fov_deg=100.0)[0]
    cameras = [inside, turned_away(cameras[0]), turned_away(inside)]
    proj, eyes = arrays(cameras)
    images = constant_images([[40, 50, 60], [1, 1, 1], [2, 2, 2]], 32, 32)
    got = kernel(scale, nodes, ids, plain_rows(density), images, proj, eyes, 255, 0.3).cpu().numpy()
    assert got.tolist() == [[40, 50, 60, 1], [0, 0, 0, 0]]
    density[0] = 0.0
    got = kernel(scale, nodes, ids, plain_rows(density), images, proj, eyes, 255, 0.3).cpu().numpy()
    assert got.tolist() == [[40, 50, 60, 1], [40, 50, 60, 1]]


# ------------------------------------------------------------------------------- exactness
def test_split_calls_fold_to_the_bits_of_one_call_and_calls_repeat():
    scale, nodes, ids, density = grid_case(257)
    cameras = rig(NINE, 4.0, 32, 32, fov_deg=90.0)
    proj, eyes = arrays(cameras)
    images, rows = seeded_images(9, 32, 32, 29), plain_rows(density)
    whole = kernel(scale, nodes, ids, rows, images, proj, eyes, 128, 0.3).cpu().numpy()
    again = kernel(scale, nodes, ids, rows, images, proj, eyes, 128, 0.3).cpu().numpy()
    assert np.array_equal(whole, again) and whole[:, 3].max() > 1
    out = kernel(scale, nodes, ids, rows, images[5:], proj[5:], eyes[5:], 128, 0.3)
    assert not np.array_equal(out.cpu().numpy(), whole)
    folded = kernel(scale, nodes, ids, rows, images[:5], proj[:5], eyes[:5], 128, 0.3, out=out)
    assert folded is out and np.array_equal(out.cpu().numpy(), whole)


def test_sh_rows_give_the_votes_of_the_plain_tree():
    import fourier_feature_nets as ffn
    scale, nodes, ids, density = grid_case(65)
    cameras = rig(NINE, 4.0, 32, 32, fov_deg=90.0)
    scene = Scene(seeded_images(9, 32, 32, 31), cameras)
    plain = ffn.OcTree(float(scale), nodes, ids, plain_rows(density))
    want = plain.visible_votes(scene, (0, 0, 0))
    assert want.dtype == np.uint32 and want.shape == (65, 4) and (want[:, 3] > 0).any()
    rng = np.random.default_rng(37)
    for degree in (1, 2):
        data = rng.standard_normal((65, 3 * (degree + 1) ** 2 + 1)).astype(F)
        data[:, -1] = density
        tree = ffn.OcTree(float(scale), nodes, ids, data, sh_degree=degree)
        assert np.array_equal(tree.visible_votes(scene, (0, 0, 0)), want)
    # and the method is the op
    proj, eyes = arrays(cameras)
    got = kernel(scale, nodes, ids, plain_rows(density), scene.images, proj, eyes, 128, 0.3)
    assert np.array_equal(got.cpu().numpy(), want)


# ------------------------------------------------------------------------------- the methods
def test_color_from_images():
    import fourier_feature_nets as ffn
    scale, nodes, ids, density = grid_case(257)
    center = (0.25, -0.5, 0.125)
    cameras = rig(NINE, 4.0, 32, 32, fov_deg=90.0)       # they look at the origin, not the centre
    scene = Scene(seeded_images(9, 32, 32, 41), cameras)
    rng = np.random.default_rng(43)
    rows = plain_rows(density)
    rows[:, :3] = rng.random((257, 3)).astype(F)
    tree = ffn.OcTree(float(scale), nodes, ids, rows)
    tree._center = center
    votes = tree.visible_votes(scene)
    assert np.array_equal(votes, tree.visible_votes(scene, center))
    assert not np.array_equal(votes, tree.visible_votes(scene, (0, 0, 0)))
    colored, counts = tree.color_from_images(scene)
    assert counts.dtype == np.uint32 and np.array_equal(counts, votes[:, 3])
    seen = counts > 0
    assert 20 < seen.sum() < 257
    data = colored.leaf_data()
    assert data.dtype == F and data.shape == (257, 4)
    assert np.array_equal(bits(data[:, :3]), bits(vref.colors(votes, rows[:, :3])))
    assert np.array_equal(bits(data[~seen]), bits(rows[~seen]))                # untouched
    assert np.array_equal(bits(data[:, 3]), bits(rows[:, 3]))                  # densities
    assert np.array_equal(bits(tree.leaf_data()), bits(rows))                  # the tree itself
    for key in ("node_index", "leaf_index", "scale"):
        assert np.array_equal(colored.state_dict[key], tree.state_dict[key])
    assert colored.center == center and colored._device == tree._device
    # the restatement agrees on the shifted cube too
    proj, eyes = arrays(cameras, center)
    want = vref.visible(scale, nodes, ids, density, scene.images, proj, eyes, 128, 0.3)
    sure = ~want["undecided"].any(1)
    assert want["undecided"].sum() <= 0.01 * want["pairs"]
    assert np.array_equal(votes[sure].astype(np.int64), want["votes"][sure])


FRONT, BACK = (250, 40, 10), (10, 40, 250)


@functools.lru_cache(maxsize=None)
def two_sided_ball():
    """A ball seen by one camera from +x, where it is FRONT-coloured, and one from -x, where it is
    BACK-coloured."""
    cameras = rig([(1, 0, 0), (-1, 0, 0)], 4.0, 32, 32)
    images = np.concatenate([ball_images(cameras[:1], 0.6, FRONT),
                             ball_images(cameras[1:], 0.6, BACK)])
    return Scene(images, cameras)


def test_build_from_silhouettes_colours_from_the_cameras_that_see():
    """The purpose of K24.  Two cameras face each other across a ball that is red from one side and
    blue from the other.  The hull's cells project into both, so ``color="mean"`` makes every cell
    the average, purple.  With ``color="visible"`` every cell that the front camera sees through the
    hull is seen by it alone and ends on the front colour."""
    import fourier_feature_nets as ffn
    scene = two_sided_ball()
    build = ffn.OcTree.build_from_silhouettes
    mean = build(scene, 5)
    same = build(scene, 5, color="mean")
    for key in ("node_index", "leaf_index"):
        assert np.array_equal(mean.state_dict[key], same.state_dict[key])
    assert np.array_equal(bits(mean.leaf_data()), bits(same.leaf_data()))
    seen_by = [mean.visible_votes(Scene(scene.images[k:k + 1], scene.cameras[k:k + 1]))[:, 3] > 0
               for k in range(2)]
    assert seen_by[0].sum() > 10 and seen_by[1].sum() > 10
    visible = build(scene, 5, color="visible")
    assert np.array_equal(visible.state_dict["leaf_index"], mean.state_dict["leaf_index"])
    assert np.array_equal(bits(visible.leaf_data()[:, 3]), bits(mean.leaf_data()[:, 3]))
    front, back = np.asarray(FRONT, np.float64) / 255, np.asarray(BACK, np.float64) / 255
    off = np.abs(visible.leaf_data()[:, :3].astype(np.float64) - front).max(1)
    print("front camera sees %d leaves, back %d, both %d; largest distance from the front colour "
          "%.5f" % (seen_by[0].sum(), seen_by[1].sum(), (seen_by[0] & seen_by[1]).sum(),
                    off[seen_by[0]].max()))
    assert (off[seen_by[0]] <= 1 / 255).all()
    off_back = np.abs(visible.leaf_data()[:, :3].astype(np.float64) - back).max(1)
    assert (off_back[seen_by[1]] <= 1 / 255).all()
    # the mean tree: most of those same leaves are the average of both sides (the rest project
    # onto the grown rim of one silhouette, where the other camera alone votes)
    off_mean = np.abs(mean.leaf_data()[:, :3].astype(np.float64) - front).max(1)
    assert not (off_mean[seen_by[0]] <= 1 / 255).all()
    assert (off_mean[seen_by[0]] > 0.4).mean() > 0.5
    # a leaf no camera sees keeps the mean
    hidden = ~(seen_by[0] | seen_by[1])
    assert hidden.any()
    assert np.array_equal(bits(visible.leaf_data()[hidden]), bits(mean.leaf_data()[hidden]))
    # merging runs after the colouring
    merged = build(scene, 5, color="visible", merge_tolerance=(0.01, 1e9))
    assert merged.num_leaves < visible.num_leaves


# ------------------------------------------------------------------------------- the programs
def test_the_programs(tmp_path):
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES + OBLIQUE_EYES[:2], 4.0, 32, 32)
    images = np.concatenate([ball_images(cameras[:1], 0.6, FRONT),
                             ball_images(cameras[1:], 0.6, BACK)])
    count = len(cameras)
    data_path, hull_path, tree_path, out_path = [
        str(tmp_path / name) for name in ("data.npz", "hull.npz", "tree.npz", "out.npz")]
    np.savez(data_path, images=images,
             intrinsics=np.stack([np.asarray(c.intrinsics, F) for c in cameras]),
             extrinsics=np.stack([np.asarray(c.extrinsics, F) for c in cameras]),
             bounds=np.diag([2, 2, 2, 1]).astype(F),
             split_counts=np.array([count - 2, 1, 1], np.int32))
    train = Scene(images[:count - 2], cameras[:count - 2])
    program = os.path.join(ROOT, "scripts", "carve_octree.py")
    for path, extra in ((hull_path, []), (tree_path, ["--color", "visible"])):
        res = subprocess.run([sys.executable, program, data_path, path, "--voxel-depth", "5"] + extra,
                             capture_output=True, text=True, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
    want = ffn.OcTree.build_from_silhouettes(train, 5, color="visible")
    tree = ffn.OcTree.load(tree_path)
    assert np.array_equal(tree.state_dict["leaf_index"], want.state_dict["leaf_index"])
    assert np.array_equal(bits(tree.leaf_data()), bits(want.leaf_data()))
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "color_octree.py"), hull_path,
                          data_path, out_path, "--center", "0", "0", "0"], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    hull = ffn.OcTree.load(hull_path)
    colored, counts = hull.color_from_images(train, (0, 0, 0))
    seen = int((counts > 0).sum())
    assert "%d of %d leaves recoloured" % (seen, hull.num_leaves) in res.stdout
    assert "%d that no camera saw" % (hull.num_leaves - seen) in res.stdout
    out = ffn.OcTree.load(out_path)
    assert np.array_equal(bits(out.leaf_data()), bits(colored.leaf_data()))
    # recolouring the unmerged hull is what --color visible does
    assert np.array_equal(bits(out.leaf_data()), bits(tree.leaf_data()))
