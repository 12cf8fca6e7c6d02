"""The K14 first-hit render on the GPU (``OcTree.first_hit`` / ``render`` / ``render_image``,
``scripts/render_octree.py``) against the float64 restatement of its contract
(tests/octree_render_reference.py on top of tests/octree_walk_reference.py), against K13 itself
bit for bit, and on a voxelized scene.  No reference file is read.

``leaf`` and ``face`` are compared for EQUALITY, ``t`` within the f32 rounding of its own plane
crossing (``budgets``), on every ray that has a single right answer.  Left out are: rays whose
margin (the shortest chord of a region, near misses included) is within the per-ray budget
(``ray_budget``, the expression of the K13 tests); rays with a leaf that ends within that budget of
``t_min`` (the leaf may or may not count); and, for ``face`` only, rays that enter their leaf
through an edge (the two largest entry crossings within the budget).  Together at most 2 % of a
case -- asserted."""

import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_render_reference as rref
from tests import octree_walk_reference as wref
from tests.octree_render_helpers import (LEFT_OUT_CAP, SCENE, TREES, big_cloud, camera_rays,
                                         golden_rays, load_tree, random_colors, ray_budget)
from tests.octree_walk_helpers import opaque_ball, two_level_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MINS = [0.0, float(np.float32(0.7))]


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_first_hit(what, state, starts, directions, t_min, got, w=None, every_ray=False):
    """Asserts ``got`` (a ``Hit`` of numpy arrays) against the restatement; -> (w, want, ok).
    ``every_ray``: rays whose crossings are exact in f32 (tests/octree_lattice_helpers.py) and that
    the caller has found free of ties, where no budget is needed to have a single right answer."""
    scale, nodes, leaves = state["scale"], state["node_index"], state["leaf_index"]
    if w is None:
        w = wref.walk(scale, nodes, leaves, starts, directions)
    want = rref.first_hit(w, scale, leaves, starts, directions, t_min)
    entry, _, _ = wref.budgets(w, scale, starts, directions)
    budget = ray_budget(w, scale, starts, directions)
    count = len(budget)
    near_t_min = np.zeros(count, bool)
    close = (w["leaf"] >= 0) & (np.abs(w["t_out"] - t_min) <= budget[w["ray"]])
    near_t_min[w["ray"][close]] = True
    ok = (~w["hit"] | (w["margin"] > budget)) & ~near_t_min
    edge = want["edge_gap"] <= budget
    if every_ray:
        ok[:] = True
        edge[:] = False
    left_out = 1.0 - (ok & ~edge).mean()
    same_leaf = got.leaves == want["leaf"]
    same_face = got.faces == want["face"]
    print("%s t_min=%.2f: %d rays, %d hit, %.4f left out (%d edge entries); among those %d "
          "leaves and %d faces differ" % (what, t_min, count, (want["leaf"] >= 0).sum(), left_out,
                                          (edge & ok).sum(), (~same_leaf & ~ok).sum(),
                                          (~same_face & ~(ok & ~edge)).sum()))
    assert got.leaves.dtype == np.int64 and got.t.dtype == np.float32
    assert got.faces.dtype == np.int8
    assert got.leaves.shape == got.t.shape == got.faces.shape == (count,)
    assert left_out <= LEFT_OUT_CAP
    assert same_leaf[ok].all()
    assert same_face[ok & ~edge].all()
    found = ok & (want["leaf"] >= 0)
    clamped = found & want["clamped"]
    free = found & ~want["clamped"]
    assert (bits(got.t[clamped]) == bits(np.float32(t_min))).all()
    err = np.abs(got.t.astype(np.float64) - want["t"])
    allowed = np.zeros(count)
    allowed[want["crossing"] >= 0] = entry[want["crossing"][want["crossing"] >= 0]]
    if free.any():
        print("   worst entry error / budget %.3f" % (err[free] / allowed[free]).max())
    assert (err <= allowed)[free].all()
    miss = got.leaves < 0
    assert (got.t[miss] == 0).all() and (got.faces[miss] == -1).all()
    assert (got.faces[~miss] >= 0).all() and (got.faces[~miss] <= 6).all()
    assert (got.leaves[~w["hit"]] == -1).all()
    return w, want, ok


@functools.lru_cache(maxsize=None)
def golden_case(name):
    tree = load_tree(name)
    starts, directions = golden_rays(name)
    state = tree.state_dict
    w = wref.walk(state["scale"], state["node_index"], state["leaf_index"], starts, directions)
    return tree, starts, directions, w


@functools.lru_cache(maxsize=None)
def cloud_case(depth):
    import fourier_feature_nets as ffn
    tree = ffn.OcTree.build_from_samples(torch.from_numpy(big_cloud(depth)).cuda(), depth, 4)
    starts, directions = camera_rays(np.random.default_rng(depth), 100000, np.float32(tree.scale))
    state = tree.state_dict
    w = wref.walk(state["scale"], state["node_index"], state["leaf_index"], starts, directions)
    return tree, starts, directions, w


def test_hand_worked_cases_on_the_device():
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    tree = ffn.OcTree(float(scale), nodes, leaves)
    starts = np.float32([[-2, -0.5, -0.5], [0.25, 0.3, -3], [0.2, 0.3, 0.1], [3, 0.75, 0.8]])
    dirs = np.float32([[2, 0, 0], [0, 0, 1], [0, 0, -0.5], [-1, 0, 0]])
    hit = tree.first_hit(starts, dirs)
    assert type(hit).__name__ == "Hit" and hit._fields == ("leaves", "t", "faces")
    assert list(hit.leaves) == [0, 1, 1, 2] and list(hit.faces) == [0, 4, 6, 1]
    assert list(hit.t) == [0.5, 3.0, 0.0, 2.0]
    check_first_hit("two levels", tree.state_dict, starts, dirs, 0.0, hit)
    late = tree.first_hit(starts, dirs, t_min=0.5)
    assert list(late.leaves) == [0, 1, -1, 2] and list(late.faces) == [0, 4, -1, 1]
    assert list(late.t) == [0.5, 3.0, 0.0, 2.0]
    inside = tree.first_hit(starts, dirs, t_min=3.25)             # inside leaf 1 on ray 1
    assert list(inside.leaves) == [-1, 1, -1, -1] and list(inside.faces) == [-1, 6, -1, -1]
    assert bits(inside.t[1]) == bits(np.float32(3.25))
    one = tree.first_hit(starts[1], dirs[1])                        # a single (3,) ray
    assert one.leaves.shape == (1,) and one.leaves[0] == 1 and one.faces[0] == 4
    root = ffn.OcTree(2.0, np.zeros(0, np.int64), np.array([0], np.int64))
    hit = root.first_hit(np.float32([[0, 0, 0], [-4, 0.5, 0.5]]), np.float32([[0, 0, 4], [1, 0, 0]]))
    assert list(hit.leaves) == [0, 0] and list(hit.t) == [0.0, 2.0] and list(hit.faces) == [6, 0]


@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", TREES)
def test_first_hit_equals_the_restatement_on_the_golden_trees(name, t_min):
    tree, starts, directions, w = golden_case(name)
    keep_s, keep_d = starts.copy(), directions.copy()
    hit = tree.first_hit(starts, directions, t_min)
    assert np.array_equal(starts, keep_s) and np.array_equal(directions, keep_d)
    _, want, _ = check_first_hit(name, tree.state_dict, starts, directions, t_min, hit, w)
    assert (hit.leaves >= 0).sum() >= 100 and (hit.leaves < 0).any()
    assert (hit.faces == 6).any() and len(np.unique(hit.faces[hit.faces >= 0])) >= 6


@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("depth", [6, 10])
def test_first_hit_on_large_random_clouds(depth, t_min):
    tree, starts, directions, w = cloud_case(depth)
    assert tree.depth == depth and len(np.unique(tree.leaf_depths())) >= 2
    hit = tree.first_hit(starts, directions, t_min)
    check_first_hit("depth %d" % depth, tree.state_dict, starts, directions, t_min, hit, w)
    assert set(np.unique(hit.faces)) == {-1, 0, 1, 2, 3, 4, 5, 6}


@pytest.mark.parametrize("t_min", T_MINS)
def test_first_hit_is_the_first_qualifying_stop_of_k13(t_min):
    """Bit for bit, on every ray: no rays are left out here, both sides are the same kernel."""
    tree, starts, directions, _ = cloud_case(6)
    dev_s, dev_d = torch.from_numpy(starts).cuda(), torch.from_numpy(directions).cuda()
    hit = tree.first_hit(dev_s, dev_d, t_min)
    assert all(torch.is_tensor(x) and x.is_cuda for x in hit)
    t_in, _, flag = tree.spans(dev_s, dev_d, t_min, pad=0)
    found = hit.leaves >= 0
    assert torch.equal(found, flag)
    assert torch.equal(hit.t[found].view(torch.int32), t_in[found].view(torch.int32))
    length = 3 * 2 ** (tree.depth - 1) + 2                      # nothing is truncated
    path = tree.walk(dev_s, dev_d, length)
    # stop k ends where stop k + 1 begins (the last one at the fill, the cube's exit)
    t_exit = path.t_stops[:, 1:]
    takes = (path.leaves[:, :-1] >= 0) & (t_exit > np.float32(t_min))
    assert torch.equal(takes.any(1), found)
    k = takes.float().argmax(1)
    rows = torch.arange(len(k), device="cuda")
    assert torch.equal(path.leaves[rows, k][found], hit.leaves[found])
    free = found & (hit.faces != 6)
    assert free.sum().item() > 1000 and (found & ~free).sum().item() > 100
    assert torch.equal(path.t_stops[rows, k][free].view(torch.int32), hit.t[free].view(torch.int32))
    assert (path.t_stops[rows, k][found & ~free] < np.float32(t_min)).all()


def test_render_shades_the_first_hit():
    from fourier_feature_nets_amd import ops
    _, starts, directions, _ = golden_case("shell")
    data = random_colors(load_tree("shell").num_leaves, 3)
    tree = load_tree("shell", data)
    t_min = T_MINS[1]
    keep_s, keep_d = starts.copy(), directions.copy()
    hit = tree.first_hit(starts, directions, t_min)
    found = hit.leaves >= 0
    assert found.sum() >= 100 and (~found).sum() >= 20
    bg = (0.25, 0.5, 0.125)
    out = tree.render(starts, directions, t_min, background=bg)
    assert type(out).__name__ == "RenderResult" and out._fields == ("color", "alpha", "depth")
    assert np.array_equal(starts, keep_s) and np.array_equal(directions, keep_d)
    assert out.color.shape == (len(starts), 3) and out.color.dtype == np.float32
    want = np.where(found[:, None], data[np.maximum(hit.leaves, 0)], np.float32(bg)[None, :])
    assert np.array_equal(bits(out.color), bits(want))
    assert np.array_equal(out.alpha, found.astype(np.float32))
    assert np.array_equal(bits(out.depth), bits(hit.t))
    # defaults: a black background, t_min = 0
    plain = tree.render(starts, directions)
    hit0 = tree.first_hit(starts, directions)
    assert (plain.color[hit0.leaves < 0] == 0).all() and np.array_equal(bits(plain.depth), bits(hit0.t))
    # "faces": one f32 multiply per channel by the declared table
    k = ops.octree_face_shade()
    assert k.dtype == np.float32 and k.shape == (7,) and k[6] == 1.0
    faces = tree.render(starts, directions, t_min, background=bg, shading="faces")
    shaded = np.where(found[:, None], data[np.maximum(hit.leaves, 0)] * k[np.maximum(hit.faces, 0)][:, None],
                      np.float32(bg)[None, :]).astype(np.float32)
    assert np.array_equal(bits(faces.color), bits(shaded))
    assert (faces.color != out.color).any()
    assert np.array_equal(faces.alpha, out.alpha) and np.array_equal(bits(faces.depth), bits(out.depth))
    # four channels, and float64 as a tree the reference saved holds it
    wide = np.concatenate([data, random_colors(len(data), 1, seed=6)], 1)
    four = load_tree("shell", wide).render(starts, directions, t_min, background=bg)
    assert np.array_equal(bits(four.color), bits(out.color))
    fine = data.astype(np.float64) + 1e-9
    double = load_tree("shell", fine)
    want64 = np.where(found[:, None], fine.astype(np.float32)[np.maximum(hit.leaves, 0)],
                      np.float32(bg)[None, :])
    assert np.array_equal(bits(double.render(starts, directions, t_min, background=bg).color),
                          bits(want64))
    assert double.leaf_data().dtype == np.float64               # the tree's own data is untouched
    # tensors in, tensors out, the same bits, inputs unchanged
    dev_s, dev_d = torch.from_numpy(starts).cuda(), torch.from_numpy(directions).cuda()
    was_s, was_d = dev_s.clone(), dev_d.clone()
    dev = tree.render(dev_s, dev_d, t_min, background=bg, shading="faces")
    assert all(torch.is_tensor(x) and x.is_cuda for x in dev)
    assert torch.equal(dev_s, was_s) and torch.equal(dev_d, was_d)
    for a, b in zip(dev, faces):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))
    dev_hit = tree.first_hit(dev_s, dev_d, t_min)
    assert dev_hit.leaves.dtype == torch.int64 and dev_hit.faces.dtype == torch.int8
    for a, b in zip(dev_hit, hit):
        assert np.array_equal(a.cpu().numpy(), b)
    # rays no walk can follow are misses
    s = float(tree.scale)
    bad_s = np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [0, 0, 0], [2 * s, 0, 0],
                        [np.inf, 0, 0], [0, 0, 0]])
    bad_d = np.float32([[0, 0, 0], [1, 1, 1], [np.nan, 1, 0], [np.nan] * 3, [0, 1, 1],
                        [1, 0, 0], [np.inf, 1, 1]])
    bad = tree.first_hit(bad_s, bad_d)
    assert (bad.leaves == -1).all() and (bad.t == 0).all() and (bad.faces == -1).all()
    bad = tree.render(bad_s, bad_d, background=bg)
    assert (bad.color == np.float32(bg)[None, :]).all() and (bad.alpha == 0).all()
    assert (bad.depth == 0).all()
    with pytest.raises(Exception, match="t_min"):
        tree.first_hit(starts, directions, float("nan"))


def test_voxelized_scene():
    """scene16 with the opaque ball, voxelized as test_clip_to_octree_on_a_voxelized_scene does
    (depth 5, min_leaf_size 1), here with the colours: the first hit cannot start behind the
    surface point that built the leaf.

    The case is EVERY ray of the sampler, as ``render_image`` casts them: the octree is the
    geometry and the sampler's validity mask is not applied.  (The rig is symmetric: one pixel
    column of two cameras runs through the tree's x = 0 / z = 0 edges, and one column of the camera
    on the x axis has a z component of 4e-16, which the per-ray budget divides by; those 20 rays
    have no single answer.)"""
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    model = opaque_ball().to("cuda")
    dataset = ffn.ImageDataset.load(SCENE, "train", 64, True, False, None, device="cuda")
    sampler = dataset.sampler
    caster = ffn.Raycaster(model)
    index = sampler.valid_index(torch.arange(len(sampler), device="cuda"))
    with torch.no_grad():
        color, alpha, depth = caster.render(sampler.sample(index, None), True)
    starts, dirs = sampler.starts[index].contiguous(), sampler.directions[index].contiguous()
    positions, kept, count = ops.octree_surface_points(alpha.contiguous(), depth.contiguous(),
                                                       starts, dirs, 0.3, color.contiguous())
    count = int(count.item())
    assert count > 50
    tree = ffn.OcTree.build_from_samples(positions[:count].contiguous(), 5, 1,
                                         kept[:count].contiguous())
    assert tree.point_leaf_ids.min().item() >= 0
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    o = (sampler.starts - shift).cpu().numpy()
    d = sampler.directions.cpu().numpy()
    hit = tree.first_hit(o, d)
    w, want, ok = check_first_hit("scene16", tree.state_dict, o, d, 0.0, hit)
    surface = np.zeros(len(o), bool)
    surface[index[alpha > 0.3].cpu().numpy()] = True
    assert surface.sum() == count
    depth_of = np.zeros(len(o), np.float32)
    depth_of[index.cpu().numpy()] = depth.cpu().numpy()
    assert (hit.leaves[surface & ok] >= 0).all()
    # t_hit <= depth + the ray's budget + the rounding of the surface point o + d * depth (the
    # product and the sum, half an ulp each) over the ray's smallest nonzero |d|
    depth64 = depth_of.astype(np.float64)
    product = np.abs(d.astype(np.float64) * depth64[:, None]).max(1)
    point = np.abs(positions.cpu().numpy().astype(np.float64)).max()
    d_abs = np.abs(d.astype(np.float64))
    d_min = np.where(d_abs > 0, d_abs, np.inf).min(1)
    rounding = 0.5 * (np.spacing(product.astype(np.float32)).astype(np.float64)
                      + np.spacing(np.float32(point)).astype(np.float64)) / d_min
    budget = ray_budget(w, tree.scale, o, d)
    rows = surface & ok
    over = hit.t.astype(np.float64) - depth64
    print("scene16: %d surface rays, first hit at most %.3g behind the surface point (allowed "
          ">= %.3g)" % (rows.sum(), over[rows].max(), (budget + rounding)[rows].min()))
    assert (over <= budget + rounding)[rows].all()
    # a frame: hit pixels carry their leaf's colour, the others the background
    bg = (0.0, 0.25, 1.0)
    image, a_map, d_map = tree.render_image(sampler, 1, background=bg, include_depth=True)
    height, width = sampler.image_height, sampler.image_width
    assert image.shape == (height, width, 3) and image.dtype == np.uint8
    assert a_map.shape == d_map.shape == (height, width)
    first = sampler.rays_per_camera
    cam_o = (sampler.starts[first:2 * first] - shift).contiguous()
    cam_d = sampler.directions[first:2 * first].contiguous()
    cam = tree.first_hit(cam_o, cam_d)
    found = cam.leaves >= 0
    assert 0 < found.sum().item() < first
    data = torch.from_numpy(tree.leaf_data()[:, :3]).cuda()
    expect = torch.where(found[:, None], data[cam.leaves.clamp(min=0)],
                         torch.tensor(bg, dtype=torch.float32, device="cuda")[None, :])
    expect = ops.to_image(expect.contiguous(), torch.arange(first, device="cuda"), width, height)
    assert np.array_equal(image, expect.cpu().numpy())
    assert np.array_equal(a_map.reshape(-1), found.float().cpu().numpy())
    assert np.array_equal(bits(d_map.reshape(-1)), bits(cam.t.cpu().numpy()))
    assert np.array_equal(tree.render_image(sampler, 1 + sampler.num_cameras, background=bg), image)
    loaded = ffn.OcTree.load(tree.state_dict)
    with pytest.raises(ValueError):
        loaded.render_image(sampler, 1)
    assert np.array_equal(loaded.render_image(sampler, 1, center=tree.center, background=bg), image)
    # against the model's own frame: reported, not asserted
    frame = caster.render_image(sampler, 1, 4096).astype(np.float64) / 255
    black = tree.render_image(sampler, 1).astype(np.float64) / 255
    print("scene16 camera 1: octree frame vs model frame, PSNR %.2f dB" %
          (-10 * np.log10(max(((frame - black) ** 2).mean(), 1e-12))))


def test_render_octree_program(tmp_path):
    """voxelize_model.py, then render_octree.py with the centre it printed, as programs."""
    from PIL import Image
    model_path, tree_path = str(tmp_path / "voxels.pt"), str(tmp_path / "tree.npz")
    out_dir = str(tmp_path / "frames")
    opaque_ball().save(model_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "voxelize_model.py"),
                          model_path, SCENE, tree_path, "--voxel-depth", "5", "--batch-size", "300",
                          "--min-leaf-size", "2"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    lines = res.stdout.splitlines()
    at = [i for i, line in enumerate(lines) if line.endswith("points in cloud")]
    assert len(at) == 1 and "--center" in lines[at[0] + 1]
    center = lines[at[0] + 1].split("--center", 1)[1].split()
    assert len(center) == 3 and all(re.fullmatch(r"-?\d+\.\d+", c) for c in center)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_octree.py"),
                          tree_path, SCENE, out_dir, "--split", "train", "--num-cameras", "2",
                          "--shading", "faces", "--center"] + center,
                         capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    with np.load(SCENE) as data:
        height, width = data["images"].shape[1:3]
    for camera in range(2):
        with Image.open(os.path.join(out_dir, "frame_%05d.png" % camera)) as image:
            assert image.size == (width, height) and image.mode == "RGB"
    assert not os.path.exists(os.path.join(out_dir, "frame_00002.png"))
    per_camera = [line for line in res.stdout.splitlines() if re.match(r"camera \d+ .*psnr ", line)]
    assert len(per_camera) == 2
    values = [float(line.rsplit(" ", 1)[1]) for line in per_camera]
    mean = [line for line in res.stdout.splitlines() if line.startswith("mean psnr")]
    assert len(mean) == 1 and abs(float(mean[0].rsplit(" ", 1)[1]) - np.mean(values)) < 2e-3
    print("\n".join(per_camera + mean))
