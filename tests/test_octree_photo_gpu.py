"""K28 on the device: ``ops.octree_visible_moments`` against the numpy restatement
(tests/photo_reference.py), all eight fields equal as integers on scenes without an undecided pair;
K24's votes inside it bit for bit; folding over camera subsets and orders; the field bound at 66 051
cameras; the hand case; ``OcTree.carve_photo`` on the two-blob scene, sweep for sweep; trees with
nothing to refute; ``build_from_silhouettes(photo_threshold=...)``; ``recolor``; the programs."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import photo_helpers as ph
from tests import photo_reference as pref
from tests.carve_helpers import AXIS_EYES, Scene, ball_images, rig
from tests.helpers import look_at_camera
from tests.visible_helpers import (constant_images, densities, depth_of, grid_scene,
                                   two_in_a_row)

pytestmark = pytest.mark.gpu
F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALPHA_U8 = ph.ALPHA_U8


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


def kernel(scale, nodes, ids, rows, images, proj, eyes, alpha_u8, tau, out=None, votes=False):
    """``ops.octree_visible_moments`` (or, with ``votes``, K24) on host arrays -> device tensor."""
    from fourier_feature_nets_amd import ops
    leaf_index = dev(np.asarray(ids, np.int64))
    centers, _ = ops.octree_leaf_geometry(leaf_index, float(scale))
    op = ops.octree_visible_votes if votes else ops.octree_visible_moments
    got = op(centers, float(scale), depth_of(ids), dev(np.asarray(nodes, np.int64)), leaf_index,
             dev(rows), 4, 3, images if torch.is_tensor(images) else dev(images),
             proj if torch.is_tensor(proj) else dev(proj),
             eyes if torch.is_tensor(eyes) else dev(eyes), alpha_u8, tau, out=out)
    assert got.dtype == torch.uint32 and got.shape == (len(ids), 4 if votes else 8)
    return got


def tree_of(scale, nodes, ids, rows, sh_degree=None):
    import fourier_feature_nets as ffn
    return ffn.OcTree(float(scale), nodes, ids, np.array(rows, F), sh_degree=sh_degree)


def same_tree(a, b):
    return (np.array_equal(a.state_dict["node_index"], b.state_dict["node_index"])
            and np.array_equal(a.state_dict["leaf_index"], b.state_dict["leaf_index"])
            and np.array_equal(bits(a.leaf_data()), bits(b.leaf_data())))


# ------------------------------------------------------------------------------- 1: the reference
@pytest.mark.parametrize("tau", [0.0, 0.3])
@pytest.mark.parametrize("name", ["grid", "mixed"])
def test_moments_equal_the_restatement_in_all_eight_fields(name, tau):
    scale, nodes, ids, density, cameras, images = ph.moment_scene(name)
    assert all((images[..., 3] == a).any() for a in (0, ALPHA_U8 - 1, ALPHA_U8, 255))
    proj, eyes = arrays(cameras)
    want = pref.moments(scale, nodes, ids, density, images, proj, eyes, ALPHA_U8, tau)
    print("%s, tau %.1f: %d leaves x %d cameras, %d undecided, %d candidates, %d visible"
          % (name, tau, len(ids), len(cameras), int(want["undecided"].sum()),
             int(want["candidate"].sum()), int(want["visible"].sum())))
    assert not want["undecided"].any()
    got = kernel(scale, nodes, ids, plain_rows(density), images, proj, eyes, ALPHA_U8, tau)
    got = got.cpu().numpy().astype(np.int64)
    assert np.array_equal(got, want["moments"])
    assert (got[:, 3] > 1).sum() > 50 and not got[:, 7].any()


# ------------------------------------------------------------------------------- 2: K24 inside
@pytest.mark.parametrize("leaves", [1, 63, 64, 65, 200])
def test_the_first_four_fields_are_the_votes_of_k24(leaves):
    scale, nodes, ids = grid_scene(leaves, seed=leaves)
    density = densities(scale, 4, leaves, 7)
    cameras = rig(ph.NINE, 4.0, 24, 20, fov_deg=90.0)
    proj, eyes = arrays(cameras)
    images = ph.rgba_images(9, 20, 24, leaves, ALPHA_U8)
    args = (scale, nodes, ids, plain_rows(density), images, proj, eyes, ALPHA_U8, 0.3)
    moments = kernel(*args).cpu().numpy()
    votes = kernel(*args, votes=True).cpu().numpy()
    assert np.array_equal(moments[:, :4], votes) and votes[:, 3].any()
    assert not moments[:, 7].any()
    if leaves > 1:
        assert (moments[:, 4:7] > moments[:, :3]).any()


def test_the_first_four_fields_are_the_votes_on_a_tree_of_three_leaf_sizes():
    scale, nodes, ids, density, cameras, images = ph.moment_scene("mixed")
    assert len(ids) % 64 != 0
    proj, eyes = arrays(cameras)
    args = (scale, nodes, ids, plain_rows(density), images, proj, eyes, ALPHA_U8, 0.3)
    assert np.array_equal(kernel(*args).cpu().numpy()[:, :4],
                          kernel(*args, votes=True).cpu().numpy())


# ------------------------------------------------------------------------------- 3: folding
def test_camera_subsets_and_orders_fold_to_the_bits_of_one_call():
    scale, nodes, ids, density, cameras, images = ph.moment_scene("grid")
    proj, eyes = arrays(cameras)
    rows = plain_rows(density)
    whole = kernel(scale, nodes, ids, rows, images, proj, eyes, ALPHA_U8, 0.3).cpu().numpy()
    again = kernel(scale, nodes, ids, rows, images, proj, eyes, ALPHA_U8, 0.3).cpu().numpy()
    assert np.array_equal(whole, again) and whole[:, 3].max() > 1
    order = np.array([4, 0, 5, 2, 1, 3])
    mixed = kernel(scale, nodes, ids, rows, images[order], proj[order], eyes[order], ALPHA_U8, 0.3)
    assert np.array_equal(mixed.cpu().numpy(), whole)
    out = None
    for last, part in ((False, order[:1]), (False, order[1:4]), (True, order[4:])):
        folded = kernel(scale, nodes, ids, rows, images[part], proj[part], eyes[part], ALPHA_U8,
                        0.3, out=out)
        assert out is None or folded is out
        out = folded
        assert last or not np.array_equal(out.cpu().numpy(), whole)
    assert np.array_equal(out.cpu().numpy(), whole)


# ------------------------------------------------------------------------------- 4: the bound
def origin_camera():
    """At (0, 0, -4) looking along +z at a 1 x 1 image whose principal point is (0, 0): the origin
    projects to fu = fv = 0.5, the one pixel."""
    import fourier_feature_nets as ffn
    intr, pose = look_at_camera((0, 0, -4), 1, 1)
    intr = np.array(intr, F)
    intr[0, 2], intr[1, 2] = 0.0, 0.0
    return ffn.CameraInfo.create("one", ffn.Resolution(1, 1), intr, pose)


@pytest.mark.parametrize("pixel", [(255, 255, 255, 255), (255, 0, 9, 255)])
def test_the_fields_hold_66051_cameras_without_a_carry(pixel):
    """A root-only tree that every camera sees on the same pixel.  65025 * 66051 = 4 294 966 275 is
    the largest sum of squares below 2^32; with g = 0 a carry out of sq_r would land in sq_g.  Two
    launches: 65 535 cameras and 516."""
    from fourier_feature_nets_amd import ops
    count = ops.OCTREE_MOMENTS_MAX_CAMERAS
    assert count == 66051
    nodes, ids, rows = np.zeros(0, np.int64), np.zeros(1, np.int64), plain_rows(np.ones(1, F))
    proj, eyes = arrays([origin_camera()])
    one = np.array(pixel, np.uint8).reshape(1, 1, 1, 4)
    want = pref.moments(1.0, nodes, ids, [1.0], one, proj, eyes, ALPHA_U8, 0.3)["moments"]
    r, g, b = pixel[:3]
    assert want.tolist() == [[r, g, b, 1, r * r, g * g, b * b, 0]]
    got = kernel(1.0, nodes, ids, rows, dev(one).repeat(count, 1, 1, 1),
                 dev(proj).repeat(count, 1, 1), dev(eyes).repeat(count, 1), ALPHA_U8, 0.3)
    got = got.cpu().numpy().astype(np.int64)
    assert got.tolist() == (want * count).tolist()
    assert got[0, 4] == 65025 * 66051 == 4294966275 and got[0, 3] == count and got[0, 7] == 0
    with pytest.raises(ValueError, match="66052 cameras"):
        kernel(1.0, nodes, ids, rows, dev(one).repeat(count + 1, 1, 1, 1),
               dev(proj).repeat(count + 1, 1, 1), dev(eyes).repeat(count + 1, 1), ALPHA_U8, 0.3)


# ------------------------------------------------------------------------------- 5: by hand
@pytest.mark.parametrize("front,occludes", [(50.0, True), (0.0, False)])
def test_two_cameras_on_two_leaves_in_a_row(front, occludes):
    """Both cameras meet leaf 0 first; leaf 1 lies behind about one unit of leaf 0 for both."""
    scale, nodes, ids, density, _ = two_in_a_row(front)
    cameras = rig([(-1, 0, 0), (-1, -0.5, -0.5)], 4.0, 16, 16)
    proj, eyes = arrays(cameras)
    images = constant_images([[7, 8, 9], [100, 50, 200]], 16, 16)
    hand = [107, 58, 209, 2, 49 + 10000, 64 + 2500, 81 + 40000, 0]
    want = [hand, [0] * 8 if occludes else hand]
    ref = pref.moments(scale, nodes, ids, density, images, proj, eyes, 1, 0.3)
    assert ref["moments"].tolist() == want and not ref["undecided"].any()
    got = kernel(scale, nodes, ids, plain_rows(density), images, proj, eyes, 1, 0.3)
    assert got.cpu().numpy().tolist() == want


# ------------------------------------------------------------------------------- 6, 8: phantoms
def rendered(tree, cameras):
    """The images of ``cameras`` by ``OcTree.render``: the hit leaf's colour, alpha from the hit."""
    def render(starts, directions):
        out = tree.render(starts, directions)
        return out.color, out.alpha
    return ph.images_of(render, cameras)


@functools.lru_cache(maxsize=None)
def blob_case():
    """The two-blob scene with its images rendered on the device, and the restatement's loop on
    those images."""
    scene = ph.blob_scene()
    true = tree_of(scene["scale"], *scene["true"])
    images = rendered(true, scene["cameras"])
    nodes, ids, rows = scene["true"]
    exact = ph.images_of(ph.reference_render(scene["scale"], nodes, ids, rows[:, :3]),
                         scene["cameras"])
    print("pixels that differ from the float64 first hit: %d" % int((images != exact).any(-1).sum()))
    _, ids, rows = scene["start"]
    proj, eyes = arrays(scene["cameras"])
    want = pref.carve(scene["scale"], ids, dict(zip(ids.tolist(), rows[:, 3].tolist())), images,
                      proj, eyes, ALPHA_U8, 0.3, 0.1)
    return scene, Scene(images, scene["cameras"]), want


def test_carve_photo_drops_exactly_the_phantoms_sweep_for_sweep():
    scene, data, want = blob_case()
    sweeps = want["sweeps"]
    print("restatement:", [(len(s["leaf_index"]), s["seen"], s["judged"], len(s["dropped"]),
                            s["undecided"]) for s in sweeps])
    assert all(s["undecided"] == 0 for s in sweeps) and want["converged"]
    assert np.array_equal(want["leaf_index"], scene["true"][1])
    start = tree_of(scene["scale"], *scene["start"])
    tree, report = start.carve_photo(data, (0, 0, 0), threshold=0.1)
    assert report.converged and len(report) == len(sweeps) == 4
    assert [tuple(s) for s in report] == [(len(s["leaf_index"]), s["seen"], s["judged"],
                                           len(s["dropped"])) for s in sweeps]
    assert np.array_equal(tree.state_dict["leaf_index"], scene["true"][1])
    assert np.array_equal(tree.state_dict["node_index"], scene["true"][0])
    gone = np.setdiff1d(scene["start"][1], tree.state_dict["leaf_index"])
    assert np.array_equal(gone, scene["phantom_ids"])
    # the rows of what is left are the start tree's, the start tree is untouched
    kept = np.isin(scene["start"][1], tree.state_dict["leaf_index"])
    assert np.array_equal(bits(tree.leaf_data()), bits(scene["start"][2][kept]))
    assert start.num_leaves == len(scene["start"][1])
    assert tree.sh_degree is None and tree.scale == start.scale
    # leaf set for leaf set: k sweeps leave what the restatement has after k
    for k in (1, 2, 3):
        part, short = start.carve_photo(data, (0, 0, 0), threshold=0.1, max_sweeps=k)
        assert len(short) == k and not short.converged
        assert np.array_equal(part.state_dict["leaf_index"], sweeps[k]["leaf_index"])
        assert [tuple(s) for s in short] == [tuple(s) for s in report[:k]]
    # and the moments of every sweep's tree
    for s in sweeps:
        nodes, ids = pref.tree_of(s["leaf_index"])
        rows = scene["start"][2][np.isin(scene["start"][1], ids)]
        got = tree_of(scene["scale"], nodes, ids, rows).visible_moments(data, (0, 0, 0))
        assert got.dtype == np.uint32 and np.array_equal(got.astype(np.int64), s["moments"])


def test_a_drop_exposes_leaves_that_the_next_sweep_judges():
    scene, data, want = blob_case()
    first, second = want["sweeps"][:2]
    before = dict(zip(first["leaf_index"].tolist(), first["moments"][:, 3].tolist()))
    newly = [i for i, n in zip(second["leaf_index"].tolist(), second["moments"][:, 3].tolist())
             if n >= 2 and before[i] < 2]
    assert len(newly) >= 4 and set(newly) & set(second["dropped"].tolist())
    start = tree_of(scene["scale"], *scene["start"])
    tree, report = start.carve_photo(data, (0, 0, 0), threshold=0.1, max_sweeps=2)
    assert np.array_equal(tree.state_dict["leaf_index"], want["sweeps"][2]["leaf_index"])
    assert not set(newly) & set(first["dropped"].tolist())
    assert report[1].dropped == len(second["dropped"]) > 0


# ------------------------------------------------------------------------------- 7: nothing to refute
def test_a_tree_of_one_colour_is_returned_bit_for_bit():
    scene = ph.blob_scene()
    nodes, ids, rows = scene["true"]
    rows = rows.copy()
    rows[:, :3] = F([200, 120, 40]) / F(255)
    true = tree_of(scene["scale"], nodes, ids, rows)
    data = Scene(rendered(true, scene["cameras"]), scene["cameras"])
    assert set(map(tuple, data.images[data.images[..., 3] > 0][:, :3])) == {(200, 120, 40)}
    tree, report = true.carve_photo(data, (0, 0, 0), threshold=0.0)
    assert same_tree(tree, true) and tree is not true
    assert len(report) == 1 and report.converged
    assert report[0].leaves == 16 and report[0].dropped == 0 and report[0].judged >= 8
    tree, report = true.carve_photo(data, (0, 0, 0), threshold=0.0, max_sweeps=0)
    assert same_tree(tree, true) and tree is not true and report == [] and not report.converged
    # a transparent tree under seeded noise: every leaf is seen by two or more cameras that differ
    # (the restatement drops all 16), and a sweep that would leave no leaf is refused
    noise = ph.rgba_images(9, 20, 24, 5, 1)
    clear = np.zeros(16, F)
    proj, eyes = arrays(scene["cameras"])
    ref = pref.moments(scene["scale"], nodes, ids, clear, noise, proj, eyes, 1, 0.0)
    assert (pref.actions(ref["moments"], 0.0) == pref.DROP).all() and not ref["undecided"].any()
    with pytest.raises(ValueError, match="threshold"):
        tree_of(scene["scale"], nodes, ids, plain_rows(clear)).carve_photo(
            Scene(noise, scene["cameras"]), (0, 0, 0), threshold=0.0, alpha_threshold=0.0,
            min_transmittance=0.0)


# ------------------------------------------------------------------------------- 9: the builder
def test_build_from_silhouettes_without_a_threshold_is_the_parent_method():
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES, 4.0, 32, 32)
    scene = Scene(ball_images(cameras, 0.6), cameras)
    build = ffn.OcTree.build_from_silhouettes
    for kwargs in ({}, {"color": "visible"}, {"footprint": "box"}):
        parent = build(scene, 4, **kwargs)
        assert same_tree(build(scene, 4, photo_threshold=None, **kwargs), parent)
        assert same_tree(build(scene, 4, photo_threshold=None, photo_min_views=5,
                               photo_max_sweeps=0, **kwargs), parent)


def test_build_from_silhouettes_with_a_threshold_is_the_composition_by_hand():
    """Four of the two-blob scene's cameras: their hull is fat enough to hold cells that two of
    them see in front of different blobs (the restatement, on the float64 first hit's images: 120
    cells, sweeps that drop 12, 4 and 0)."""
    import fourier_feature_nets as ffn
    _, whole, _ = blob_case()
    few = [0, 1, 2, 8]
    data = Scene(whole.images[few], [whole.cameras[k] for k in few])
    build = ffn.OcTree.build_from_silhouettes
    hull = build(data, 4)
    thin, want_report = hull.carve_photo(data, threshold=0.1, min_transmittance=0.3)
    print("hull %d leaves, thinned %d; sweeps %s" % (hull.num_leaves, thin.num_leaves,
                                                      [tuple(s) for s in want_report]))
    assert thin.num_leaves < hull.num_leaves and want_report.converged and len(want_report) == 3
    assert np.isin(ph.blob_scene()["true"][1], thin.state_dict["leaf_index"]).all()
    report = ffn.PhotoReport()
    got = build(data, 4, photo_threshold=0.1, photo_report=report)
    assert same_tree(got, thin) and got.center == hull.center
    assert [tuple(s) for s in report] == [tuple(s) for s in want_report] and report.converged
    # the votes of color="visible" come from the thinned tree
    colored, _ = thin.color_from_images(data, min_transmittance=0.3)
    got = build(data, 4, photo_threshold=0.1, color="visible")
    assert same_tree(got, colored)
    # another transmittance and another sweep count reach the sweeps
    other, _ = hull.carve_photo(data, threshold=0.1, min_transmittance=0.6, max_sweeps=1)
    assert same_tree(build(data, 4, photo_threshold=0.1, photo_max_sweeps=1,
                           visible_transmittance=0.6), other)
    # and the merge passes run last, on the coloured cells
    codes = torch.from_numpy(colored.state_dict["leaf_index"] - (8 ** 3 - 1) // 7).to(
        device="cuda", dtype=torch.int32)
    merged = ffn.OcTree._from_cells(codes, dev(colored.leaf_data()), 4, 1.0, (0.0, 0.0, 0.0),
                                    (0.01, 1e9), torch.device("cuda"))
    got = build(data, 4, photo_threshold=0.1, color="visible", merge_tolerance=(0.01, 1e9))
    assert same_tree(got, merged)


# ------------------------------------------------------------------------------- 10: recolour
def test_recolor_takes_the_means_of_the_final_tree():
    """The start tree all grey: a leaf that some camera sees turns red or blue, the rest stay."""
    scene, data, want = blob_case()
    nodes, ids, grey = scene["start"]
    grey = grey.copy()
    grey[:, :3] = 0.5
    start = tree_of(scene["scale"], nodes, ids, grey)
    tree, report = start.carve_photo(data, (0, 0, 0), threshold=0.1, recolor=True)
    plain, _ = start.carve_photo(data, (0, 0, 0), threshold=0.1)
    last = want["sweeps"][-1]["moments"]                      # the final tree's: nothing dropped
    assert np.array_equal(bits(tree.leaf_data()[:, :3]),
                          bits(pref.colors(last, plain.leaf_data()[:, :3])))
    assert np.array_equal(bits(tree.leaf_data()[:, 3]), bits(plain.leaf_data()[:, 3]))
    seen = last[:, 3] > 0
    assert seen.sum() >= 8 and (tree.leaf_data()[seen, :3] != 0.5).all()
    assert np.array_equal(bits(tree.leaf_data()[~seen]), bits(plain.leaf_data()[~seen]))
    # a loop cut short: the colours come from one more call, on the tree that is left
    tree, report = start.carve_photo(data, (0, 0, 0), threshold=0.1, max_sweeps=2, recolor=True)
    assert not report.converged
    final = want["sweeps"][2]
    rows = grey[np.isin(ids, final["leaf_index"])]
    assert np.array_equal(bits(tree.leaf_data()[:, :3]),
                          bits(pref.colors(final["moments"], rows[:, :3])))
    # max_sweeps = 0 is color_from_images
    tree, _ = start.carve_photo(data, (0, 0, 0), max_sweeps=0, recolor=True)
    assert same_tree(tree, start.color_from_images(data, (0, 0, 0))[0])


def test_an_sh_tree_is_carved_and_not_recoloured():
    scene, data, want = blob_case()
    nodes, ids, rows = scene["start"]
    sh_rows = np.random.default_rng(3).standard_normal((len(ids), 13)).astype(F)
    sh_rows[:, -1] = rows[:, 3]
    tree = tree_of(scene["scale"], nodes, ids, sh_rows, sh_degree=1)
    with pytest.raises(ValueError, match="coefficients, not a colour"):
        tree.carve_photo(data, (0, 0, 0), recolor=True)
    carved, report = tree.carve_photo(data, (0, 0, 0))
    assert np.array_equal(carved.state_dict["leaf_index"], scene["true"][1])
    assert carved.sh_degree == 1 and report.converged
    kept = np.isin(ids, scene["true"][1])
    assert np.array_equal(bits(carved.leaf_data()), bits(sh_rows[kept]))
    plain = tree_of(scene["scale"], nodes, ids, rows)
    assert np.array_equal(tree.visible_moments(data, (0, 0, 0)), plain.visible_moments(data, (0, 0, 0)))


# ------------------------------------------------------------------------------- the programs
def test_the_programs(tmp_path):
    import fourier_feature_nets as ffn
    scene, data, _ = blob_case()
    cameras, images = data.cameras, data.images
    count = len(cameras)
    data_path, start_path, out_path, tree_path = [
        str(tmp_path / name) for name in ("data.npz", "start.npz", "out.npz", "tree.npz")]
    np.savez(data_path, images=images,
             intrinsics=np.stack([np.asarray(c.intrinsics, F) for c in cameras]),
             extrinsics=np.stack([np.asarray(c.extrinsics, F) for c in cameras]),
             bounds=np.diag([2, 2, 2, 1]).astype(F),
             split_counts=np.array([count - 2, 1, 1], np.int32))
    train = Scene(images[:count - 2], cameras[:count - 2])
    start = tree_of(scene["scale"], *scene["start"])
    start.save(start_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "photo_carve_octree.py"),
                          start_path, data_path, out_path, "--center", "0", "0", "0",
                          "--threshold", "0.1", "--recolor"], capture_output=True, text=True,
                         cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    want, report = start.carve_photo(train, (0, 0, 0), threshold=0.1, recolor=True)
    assert same_tree(ffn.OcTree.load(out_path), want)
    for number, sweep in enumerate(report, 1):
        assert "photo sweep %d: %d leaves, %d seen, %d judged, %d dropped" % (
            (number,) + tuple(sweep)) in res.stdout
    assert "%d of %d leaves left" % (want.num_leaves, start.num_leaves) in res.stdout
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "carve_octree.py"), data_path,
                          tree_path, "--voxel-depth", "4", "--photo-threshold", "0.1",
                          "--photo-max-sweeps", "3"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    report = ffn.PhotoReport()
    want = ffn.OcTree.build_from_silhouettes(train, 4, photo_threshold=0.1, photo_max_sweeps=3,
                                             photo_report=report)
    assert same_tree(ffn.OcTree.load(tree_path), want)
    assert "photo sweep 1: %d leaves" % report[0].leaves in res.stdout
    assert ("converged" if report.converged else "did not converge") in res.stdout
