"""The K15 volume render on the GPU (``OcTree.render_volume`` / ``bake`` /
``render_image(mode="volume")``, ``scripts/bake_octree.py``, ``scripts/render_octree.py --mode
volume``) against the float64 restatement of its contract (tests/octree_volume_reference.py on top
of tests/octree_walk_reference.py), against K13's own stops, at its two limits bit for bit, and on
a voxelized scene.  No reference file is read.

Colour and alpha are compared within the per-ray budget of the restatement (derived there, from
the f32 rounding of the plane crossings and of the compositing steps) on every ray whose margin
(the shortest chord of a region, near misses included) exceeds the per-ray budget of the K13 / K14
tests (``ray_budget``); at most 2 % of a case is left out -- asserted.  A leaf that ends within a
rounding of ``t_min`` needs no exclusion here: its chord is that short, and the first term of the
budget covers it."""

import functools
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref
from tests.octree_render_helpers import (LEFT_OUT_CAP, SCENE, big_cloud, camera_rays, golden_rays,
                                         load_tree, ray_budget)
from tests.octree_volume_helpers import hand_case, random_leaf_data
from tests.octree_walk_helpers import opaque_ball

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MINS = [0.0, float(np.float32(0.7))]
BG = (0.25, 0.5, 0.125)
MID_SHARE = 0.30


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def check_volume(what, state, data, starts, directions, t_min, got, w, background=BG,
                 every_ray=False):
    """Asserts ``got`` (a ``RenderResult`` of numpy arrays) against the restatement; -> (v, ok).
    ``every_ray``: rays whose crossings are exact in f32 (tests/octree_lattice_helpers.py), where a
    margin of 0 leaves no doubt."""
    scale = state["scale"]
    v = vref.composite(w, scale, starts, directions, data, t_min, background)
    count = len(w["hit"])
    assert got.color.shape == (count, 3) and got.alpha.shape == got.depth.shape == (count,)
    assert got.color.dtype == got.alpha.dtype == got.depth.dtype == np.float32
    budget = ray_budget(w, scale, starts, directions)
    ok = ~w["hit"] | (w["margin"] > budget)
    if every_ray:
        ok[:] = True
    left_out = 1.0 - ok.mean()
    took = v["count"] > 0
    mid = took & (v["trans"] > 0.05) & (v["trans"] < 0.95)
    share = mid.sum() / max(took.sum(), 1)
    err_c = np.abs(got.color.astype(np.float64) - v["color"]).max(1)
    err_a = np.abs(got.alpha.astype(np.float64) - v["alpha"])
    print("%s t_min=%.2f: %d rays, %d take a leaf (at most %d), %.3f of them end with 0.05 < T < "
          "0.95, %.4f left out; worst error / budget: colour %.3f alpha %.3f" %
          (what, t_min, count, took.sum(), v["count"].max(), share, left_out,
           (err_c / v["budget_c"])[ok].max(), (err_a / v["budget_a"])[ok].max()))
    assert left_out <= LEFT_OUT_CAP
    assert share >= MID_SHARE
    assert (err_c <= v["budget_c"])[ok].all()
    assert (err_a <= v["budget_a"])[ok].all()
    # rays that take nothing: the background, bit for bit
    none = ok & ~took
    assert (bits(got.color[none]) == bits(np.float32(background))[None, :]).all()
    assert (got.alpha[none] == 0).all() and (got.depth[none] == 0).all()
    # depth: the heaviest leaf's t0 where the restatement's pick is beyond doubt
    depth = got.depth.astype(np.float64)
    sure = ok & (v["best"] >= 0) & (v["gap"] > 2 * v["budget_a"])
    clamped = sure & v["clamped"]
    free = sure & ~v["clamped"]
    assert (bits(got.depth[clamped]) == bits(np.float32(t_min))).all()
    allowed = np.zeros(count)
    allowed[v["best"] >= 0] = v["entry"][v["best"][v["best"] >= 0]]
    err_d = np.abs(depth - v["depth"])
    if free.any():
        print("   depth: %d sure (%d clamped), worst entry error / budget %.3f" %
              (sure.sum(), clamped.sum(), (err_d[free] / allowed[free]).max()))
    assert (err_d <= allowed)[free].all()
    # elsewhere: the t0 of SOME taken leaf (0 if no weight stands out from the rounding)
    taken_ray = w["ray"][v["taken"]]
    nearest = np.full(count, np.inf)
    np.minimum.at(nearest, taken_ray, np.abs(depth[taken_ray] - v["t0"]) - v["entry"])
    heaviest = np.zeros(count)
    np.maximum.at(heaviest, taken_ray, v["weights"])
    unsure = ok & took & ~sure
    fine = (nearest <= 0) | ((got.depth == 0) & (heaviest <= 2 * v["budget_a"]))
    assert fine[unsure].all()
    return v, ok


@functools.lru_cache(maxsize=None)
def golden_case(name):
    starts, directions = golden_rays(name)
    bare = load_tree(name)
    state = bare.state_dict
    data = random_leaf_data(state["scale"], state["leaf_index"])
    w = wref.walk(state["scale"], state["node_index"], state["leaf_index"], starts, directions)
    return load_tree(name, data), data, starts, directions, w


@functools.lru_cache(maxsize=None)
def cloud_case():
    import fourier_feature_nets as ffn
    depth = 6
    bare = ffn.OcTree.build_from_samples(torch.from_numpy(big_cloud(depth)).cuda(), depth, 4)
    state = bare.state_dict
    data = random_leaf_data(state["scale"], state["leaf_index"])
    tree = ffn.OcTree(state["scale"], state["node_index"], state["leaf_index"], data)
    starts, directions = camera_rays(np.random.default_rng(depth), 20000, np.float32(tree.scale))
    w = wref.walk(state["scale"], state["node_index"], state["leaf_index"], starts, directions)
    return tree, data, starts, directions, w


def test_hand_worked_cases_on_the_device():
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs = hand_case()
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    out = tree.render_volume(starts, dirs, background=BG)
    assert type(out).__name__ == "RenderResult" and out._fields == ("color", "alpha", "depth")
    assert all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x in out)
    assert out.color.shape == (5, 3) and out.alpha.shape == out.depth.shape == (5,)
    v = vref.composite(w, scale, starts, dirs, data, 0.0, BG)
    # rays 0 .. 2 within the budget; rays 3 and 4 end in the opaque leaf (its density of 1e30
    # makes the budget expression meaningless): alpha is 1 exactly
    for r in range(3):
        assert np.abs(out.color[r] - v["color"][r]).max() <= v["budget_c"][r]
        assert abs(out.alpha[r] - v["alpha"][r]) <= v["budget_a"][r]
    assert list(out.depth) == [0.5, 3.0, 0.0, 1.0, 2.0]
    assert out.alpha[3] == 1.0 and out.alpha[4] == 1.0 and out.alpha[2] == 0.0
    assert np.array_equal(bits(out.color[2]), bits(np.float32(BG)))
    assert np.array_equal(bits(out.color[4]), bits(data[2, :3]))
    assert np.abs(out.color[3] - v["color"][3]).max() <= 8 * 4 * 2.0 ** -24
    # t_min cuts leaf 0 on ray 0; ends it at its exit
    cut = tree.render_volume(starts, dirs, 0.75, BG)
    vc = vref.composite(w, scale, starts, dirs, data, 0.75, BG)
    assert np.abs(cut.color[0] - vc["color"][0]).max() <= vc["budget_c"][0]
    assert bits(cut.depth[0]) == bits(np.float32(0.75))
    gone = tree.render_volume(starts, dirs, 1.0, BG)
    assert np.array_equal(bits(gone.color[0]), bits(np.float32(BG))) and gone.alpha[0] == 0
    # defaults: black background; a single (3,) ray; more channels than four
    plain = tree.render_volume(starts, dirs)
    assert (plain.color[2] == 0).all() and np.array_equal(bits(plain.alpha), bits(out.alpha))
    one = tree.render_volume(starts[1], dirs[1], background=BG)
    assert one.color.shape == (1, 3) and one.alpha.shape == (1,)
    assert np.array_equal(bits(one.color[0]), bits(out.color[1])) and one.depth[0] == 3.0
    wide = np.concatenate([data, np.full((3, 2), 9.0, np.float32)], 1)
    six = ffn.OcTree(float(scale), nodes, leaves, wide).render_volume(starts, dirs, background=BG)
    for a, b in zip(six, out):
        assert np.array_equal(bits(a), bits(b))
    # the length of the directions does not matter (powers of two: the same bits but for t)
    twice = tree.render_volume(starts, dirs * np.float32(4), background=BG)
    assert np.array_equal(bits(twice.color), bits(out.color))
    assert np.array_equal(bits(twice.depth), bits(out.depth / np.float32(4)))
    # the root-only tree: one leaf, the chord of the cube
    root = ffn.OcTree(2.0, np.zeros(0, np.int64), np.array([0], np.int64),
                      np.float32([[0.5, 0.25, 1.0, 0.5]]))
    o, d = np.float32([[0, 0, 0], [-4, 0.5, 0.5], [0, 5, 0]]), np.float32([[0, 0, 4], [1, 0, 0], [1, 0, 0]])
    got = root.render_volume(o, d, background=BG)
    a = 1 - np.exp(-0.5 * np.float64([2.0, 4.0]))
    assert np.allclose(got.alpha[:2], a, rtol=0, atol=16 * 2.0 ** -24) and got.alpha[2] == 0
    assert list(got.depth) == [0.0, 2.0, 0.0]
    with pytest.raises(Exception, match="t_min"):
        tree.render_volume(starts, dirs, float("nan"))


@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", ["shell", "planes"])
def test_volume_equals_the_restatement_on_the_golden_trees(name, t_min):
    tree, data, starts, directions, w = golden_case(name)
    keep_s, keep_d = starts.copy(), directions.copy()
    out = tree.render_volume(starts, directions, t_min, BG)
    assert np.array_equal(starts, keep_s) and np.array_equal(directions, keep_d)
    check_volume(name, tree.state_dict, data, starts, directions, t_min, out, w)


@pytest.mark.parametrize("t_min", T_MINS)
def test_volume_on_a_random_cloud(t_min):
    tree, data, starts, directions, w = cloud_case()
    assert tree.depth == 6 and len(np.unique(tree.leaf_depths())) >= 2
    out = tree.render_volume(starts, directions, t_min, BG)
    check_volume("depth 6", tree.state_dict, data, starts, directions, t_min, out, w)
    # rays no walk can follow give the background
    s = float(tree.scale)
    bad_s = np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [2 * s, 0, 0], [np.inf, 0, 0]])
    bad_d = np.float32([[0, 0, 0], [1, 1, 1], [np.nan, 1, 0], [0, 1, 1], [1, 0, 0]])
    bad = tree.render_volume(bad_s, bad_d, t_min, BG)
    assert (bits(bad.color) == bits(np.float32(BG))[None, :]).all()
    assert (bad.alpha == 0).all() and (bad.depth == 0).all()


def k13_stops(tree, dev_s, dev_d, t_min):
    """The untruncated K13 path as numpy: entry t, exit t (the next stop) and leaf per stop."""
    length = 3 * 2 ** (tree.depth - 1) + 2
    path = tree.walk(dev_s, dev_d, length)
    t = path.t_stops.cpu().numpy()
    leaves = path.leaves.cpu().numpy()[:, :-1]
    t_in, t_out = t[:, :-1], t[:, 1:]
    takes = (leaves >= 0) & (t_out > np.float32(t_min))
    return t_in, t_out, leaves, takes


def f32_norm(d):
    d = np.asarray(d, np.float32)
    return np.sqrt(d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] + d[:, 2] * d[:, 2])


@pytest.mark.parametrize("t_min", T_MINS)
def test_volume_composites_the_stops_of_k13(t_min):
    """Both sides saw the same planes (the same kernel's t-values), so only the compositing
    differs: float64 here, f32 there.  Every ray, none left out, within the rounding term."""
    tree, data, starts, directions, _ = cloud_case()
    dev_s, dev_d = torch.from_numpy(starts).cuda(), torch.from_numpy(directions).cuda()
    was_s, was_d = dev_s.clone(), dev_d.clone()
    out = tree.render_volume(dev_s, dev_d, t_min, BG)
    assert all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in out)
    assert torch.equal(dev_s, was_s) and torch.equal(dev_d, was_d)
    t_in, t_out, leaves, takes = k13_stops(tree, dev_s, dev_d, t_min)
    norm = f32_norm(directions).astype(np.float64)
    trans = np.ones(len(starts))
    color = np.zeros((len(starts), 3))
    steps = takes.sum(1)
    data64 = data.astype(np.float64)
    for k in range(takes.shape[1]):
        rows = np.nonzero(takes[:, k])[0]
        if len(rows) == 0:
            continue
        t0 = np.maximum(t_in[rows, k], np.float32(t_min)).astype(np.float64)
        length = (t_out[rows, k].astype(np.float64) - t0) * norm[rows]
        a = 1.0 - np.exp(-(np.maximum(data64[leaves[rows, k], 3], 0.0) * length))
        weight = trans[rows] * a
        color[rows] += weight[:, None] * data64[leaves[rows, k], :3]
        trans[rows] *= 1.0 - a
    color += trans[:, None] * np.float32(BG).astype(np.float64)[None, :]
    scale_of = max(1.0, float(np.abs(data[:, :3]).max()), float(np.abs(np.float32(BG)).max()))
    rounding = 8.0 * (steps + 1) * 2.0 ** -24
    err_c = np.abs(out.color.cpu().numpy().astype(np.float64) - color).max(1)
    err_a = np.abs(out.alpha.cpu().numpy().astype(np.float64) - (1.0 - trans))
    print("K13 stops t_min=%.2f: worst error / rounding term: colour %.3f alpha %.3f, up to %d "
          "leaves" % (t_min, (err_c / (rounding * scale_of)).max(), (err_a / rounding).max(),
                      steps.max()))
    assert (err_c <= rounding * scale_of).all()
    assert (err_a <= rounding).all()
    host = tree.render_volume(starts, directions, t_min, BG)
    for a, b in zip(out, host):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


def test_limits_bit_for_bit():
    import fourier_feature_nets as ffn
    tree, data, starts, directions, _ = cloud_case()
    state = tree.state_dict
    t_min = T_MINS[1]

    def with_density(values):
        changed = data.copy()
        changed[:, 3] = values
        return ffn.OcTree(state["scale"], state["node_index"], state["leaf_index"], changed)

    count = len(starts)
    empty = with_density(0.0).render_volume(starts, directions, t_min, BG)
    assert (bits(empty.color) == bits(np.float32(BG))[None, :]).all()
    assert (empty.alpha == 0).all() and (empty.depth == 0).all()
    mixed = np.where(np.arange(len(data)) % 2 == 0, np.float32(-1.0), np.float32(np.nan))
    for values in (-5.0, np.nan, mixed):
        out = with_density(values).render_volume(starts, directions, t_min, BG)
        for a, b in zip(out, empty):
            assert np.array_equal(bits(a), bits(b))
    # opaque: the first-hit render, on every ray whose first qualifying stop has a chord > 0
    solid = with_density(1e30)
    out = solid.render_volume(starts, directions, t_min, BG)
    flat = solid.render(starts, directions, t_min, BG)
    hit = solid.first_hit(starts, directions, t_min)
    dev_s, dev_d = torch.from_numpy(starts).cuda(), torch.from_numpy(directions).cuda()
    t_in, t_out, _, takes = k13_stops(solid, dev_s, dev_d, t_min)
    found = takes.any(1)
    assert np.array_equal(found, hit.leaves >= 0)
    k = takes.argmax(1)
    rows = np.arange(count)
    chord = t_out[rows, k] - np.maximum(t_in[rows, k], np.float32(t_min))      # f32
    sound = ~found | (chord > 0)
    print("limits: %d rays, %d hit, %d with a first chord <= 0" % (count, found.sum(), (~sound).sum()))
    assert sound.mean() >= 0.99 and found.sum() > 1000 and (~found).sum() > 100
    assert np.array_equal(bits(out.color[sound]), bits(flat.color[sound]))
    assert np.array_equal(out.alpha[sound], found[sound].astype(np.float32))
    assert np.array_equal(bits(out.depth[sound]), bits(hit.t[sound]))


def test_early_termination():
    import fourier_feature_nets as ffn
    tree, data, starts, directions, w = cloud_case()
    state = tree.state_dict
    t_min = 0.0
    # sixteen times the density of the other cases, so that rays do get below the threshold
    dense = data.copy()
    dense[:, 3] *= np.float32(16)
    thick = ffn.OcTree(state["scale"], state["node_index"], state["leaf_index"], dense)
    full = thick.render_volume(starts, directions, t_min, BG)
    early = thick.render_volume(starts, directions, t_min, BG, min_transmittance=1e-2)
    v = vref.composite(w, state["scale"], starts, directions, dense, t_min, BG)
    cut = vref.composite(w, state["scale"], starts, directions, dense, t_min, BG, 1e-2)
    assert (cut["count"] < v["count"]).sum() > 1000              # the threshold does end walks
    bound = max(float(np.abs(data[:, :3]).max()), float(np.abs(np.float32(BG)).max()))
    diff_c = np.abs(early.color.astype(np.float64) - full.color.astype(np.float64)).max(1)
    diff_a = full.alpha.astype(np.float64) - early.alpha.astype(np.float64)
    print("early termination: %d rays end early; colour moves by at most %.3g, alpha by %.3g" %
          ((cut["count"] < v["count"]).sum(), diff_c.max(), diff_a.max()))
    assert (diff_c <= 1e-2 * bound + v["rounding"] * max(1.0, bound)).all()
    assert (diff_a <= 1e-2).all()
    assert (diff_c > 0).sum() > 1000
    # a threshold no ray reaches: the same bits
    thin = tree.render_volume(starts, directions, t_min, BG)
    v = vref.composite(w, state["scale"], starts, directions, data, t_min, BG)
    threshold = float(v["trans"].min()) / 4
    assert 1e-6 < threshold < 1 and (v["trans"] > 2 * threshold).all()
    same = tree.render_volume(starts, directions, t_min, BG, min_transmittance=threshold)
    for a, b in zip(same, thin):
        assert np.array_equal(bits(a), bits(b))
    with pytest.raises(ValueError, match="min_transmittance"):
        tree.render_volume(starts, directions, min_transmittance=1.0)


def bake_contract(logits):
    """float64 sigmoid / softplus (beta 1, threshold 20) of (L,4) logits."""
    x = logits.astype(np.float64)
    soft = np.where(x[:, 3] > 20, x[:, 3], np.log1p(np.exp(np.minimum(x[:, 3], 20.0))))
    return np.concatenate([1.0 / (1.0 + np.exp(-x[:, :3])), soft[:, None]], 1)


@pytest.mark.parametrize("kind", ["voxels", "mlp"])
def test_bake(kind, tmp_path):
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    if kind == "voxels":
        model = opaque_ball().to("cuda")
    else:
        torch.manual_seed(7)
        model = ffn.PositionalFourierMLP(3, 4, 5.5, num_channels=64).to("cuda")
    colours = np.random.default_rng(2).random((load_tree("shell").num_leaves, 3), dtype=np.float32)
    tree = load_tree("shell", colours)
    center = (0.125, -0.25, 0.0625)
    with pytest.raises(ValueError, match="cent"):
        tree.bake(model)
    was_training = model.training
    baked = tree.bake(model, center=center, batch_size=1000)      # three batches, the last short
    assert model.training == was_training
    assert baked is not tree and tree.leaf_data() is colours and tree.center is None
    assert np.array_equal(tree.leaf_data(), colours)
    assert np.array_equal(baked.state_dict["leaf_index"], tree.state_dict["leaf_index"])
    assert np.array_equal(baked.state_dict["node_index"], tree.state_dict["node_index"])
    assert baked.scale == tree.scale and baked.center == center
    data = baked.leaf_data()
    assert data.shape == (tree.num_leaves, 4) and data.dtype == np.float32
    points = torch.from_numpy(tree.leaf_centers()).cuda() + torch.tensor(center, device="cuda")
    with torch.no_grad():
        logits = model(points.contiguous()).reshape(-1, 4).contiguous()
    assert np.array_equal(bits(data), bits(ops.octree_bake(logits).cpu().numpy()))
    want = bake_contract(logits.cpu().numpy())
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    err = np.abs(data.astype(np.float64) - want) / ulp
    print("bake (%s): %d leaves, worst error %.2f ulp, density %.3g .. %.3g" %
          (kind, len(data), err.max(), data[:, 3].min(), data[:, 3].max()))
    assert (err <= 4).all()
    assert (data[:, 3] >= 0).all() and (data[:, :3] >= 0).all() and (data[:, :3] <= 1).all()
    assert np.array_equal(bits(tree.bake(model, center=center).leaf_data()), bits(data))
    # save / load / prune work on the result
    path = str(tmp_path / "baked.npz")
    baked.save(path)
    loaded = ffn.OcTree.load(path)
    assert np.array_equal(bits(loaded.leaf_data()), bits(data)) and loaded.center is None
    assert np.array_equal(loaded.state_dict["leaf_index"], baked.state_dict["leaf_index"])
    with pytest.raises(ValueError, match="cent"):
        loaded.bake(model)
    assert baked.prune().leaf_data().shape[1] == 4
    starts, directions = golden_rays("shell")
    for a, b in zip(loaded.render_volume(starts, directions), baked.render_volume(starts, directions)):
        assert np.array_equal(bits(a), bits(b))


def psnr(a, b):
    err = ((a.astype(np.float64) - b.astype(np.float64)) / 255.0) ** 2
    return float(-10 * np.log10(max(err.mean(), 1e-12)))


def test_voxelized_scene():
    """scene16 with the opaque ball, voxelized as test_octree_render_gpu.test_voxelized_scene does
    (depth 5, min_leaf_size 1), baked, and rendered as a frame."""
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
    tree = ffn.OcTree.build_from_samples(positions[:count].contiguous(), 5, 1,
                                         kept[:count].contiguous())
    colours = tree.leaf_data().copy()
    baked = tree.bake(model)                                   # the centre of the build
    assert baked.center == tree.center and np.array_equal(tree.leaf_data(), colours)
    assert baked.leaf_data().shape == (tree.num_leaves, 4)
    image, a_map, d_map = baked.render_image(sampler, 1, background=BG, include_depth=True,
                                             mode="volume")
    height, width = sampler.image_height, sampler.image_width
    assert image.shape == (height, width, 3) and image.dtype == np.uint8
    assert a_map.shape == d_map.shape == (height, width)
    assert a_map.dtype == d_map.dtype == np.float32
    first = sampler.rays_per_camera
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    cam_o = (sampler.starts[first:2 * first] - shift).contiguous()
    cam_d = sampler.directions[first:2 * first].contiguous()
    out = baked.render_volume(cam_o, cam_d, background=BG)
    expect = ops.to_image(out.color.contiguous(), torch.arange(first, device="cuda"), width, height)
    assert np.array_equal(image, expect.cpu().numpy())
    assert np.array_equal(bits(a_map.reshape(-1)), bits(out.alpha.cpu().numpy()))
    assert np.array_equal(bits(d_map.reshape(-1)), bits(out.depth.cpu().numpy()))
    assert 0 < (a_map > 0.5).sum() < first
    loaded = ffn.OcTree.load(baked.state_dict)
    with pytest.raises(ValueError, match="cent"):
        loaded.render_image(sampler, 1, mode="volume")
    assert np.array_equal(loaded.render_image(sampler, 1, center=tree.center, background=BG,
                                              mode="volume"), image)
    with pytest.raises(ValueError, match="shading"):
        baked.render_image(sampler, 1, shading="faces", mode="volume")
    # the defaults are the first-hit frame of today
    assert np.array_equal(baked.render_image(sampler, 1, background=BG),
                          baked.render_image(sampler, 1, background=BG, mode="first_hit"))
    assert np.array_equal(tree.render_image(sampler, 1), tree.render_image(sampler, 1, None, 0.0,
                                                                           (0, 0, 0), "flat", False))
    # against the model's own frame: reported, not asserted
    frame = caster.render_image(sampler, 1, 4096)
    print("scene16 camera 1 vs the model's frame: first hit %.2f dB, volume %.2f dB" %
          (psnr(tree.render_image(sampler, 1), frame),
           psnr(baked.render_image(sampler, 1, mode="volume"), frame)))


def test_bake_and_render_programs(tmp_path):
    """voxelize_model.py, bake_octree.py, then render_octree.py --mode volume, as programs, with
    the centre the first one printed."""
    from PIL import Image
    model_path, tree_path = str(tmp_path / "voxels.pt"), str(tmp_path / "tree.npz")
    baked_path, out_dir = str(tmp_path / "baked.npz"), str(tmp_path / "frames")
    opaque_ball().save(model_path)

    def run(script, *args):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + list(args),
                             capture_output=True, text=True, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        return res.stdout.splitlines()

    lines = run("voxelize_model.py", model_path, SCENE, tree_path, "--voxel-depth", "5",
                "--batch-size", "300", "--min-leaf-size", "2")
    at = [i for i, line in enumerate(lines) if line.endswith("points in cloud")]
    assert len(at) == 1 and "--center" in lines[at[0] + 1]
    center = lines[at[0] + 1].split("--center", 1)[1].split()
    assert len(center) == 3
    lines = run("bake_octree.py", tree_path, model_path, baked_path, "--batch-size", "50",
                "--center", *center)
    with np.load(baked_path) as baked, np.load(tree_path) as tree:
        assert np.array_equal(baked["leaf_index"], tree["leaf_index"])
        data = baked["leaf_data"]
        assert data.shape == (len(tree["leaf_index"]), 4) and data.dtype == np.float32
    told = [line for line in lines if line.endswith("leaves baked")]
    assert len(told) == 1 and int(told[0].split()[0]) == len(data)
    density = [line for line in lines if line.startswith("density min")]
    assert len(density) == 1
    words = density[0].split()
    assert [words[1], words[3], words[5]] == ["min", "median", "max"]
    assert np.allclose([float(words[2]), float(words[4]), float(words[6])],
                       [data[:, 3].min(), np.median(data[:, 3]), data[:, 3].max()], rtol=1e-5)
    lines = run("render_octree.py", baked_path, SCENE, out_dir, "--split", "train",
                "--num-cameras", "2", "--mode", "volume", "--min-transmittance", "1e-3",
                "--center", *center)
    with np.load(SCENE) as scene:
        height, width = scene["images"].shape[1:3]
    for camera in range(2):
        with Image.open(os.path.join(out_dir, "frame_%05d.png" % camera)) as image:
            assert image.size == (width, height) and image.mode == "RGB"
    assert not os.path.exists(os.path.join(out_dir, "frame_00002.png"))
    per_camera = [line for line in lines if re.match(r"camera \d+ .*psnr ", line)]
    assert len(per_camera) == 2
    values = [float(line.rsplit(" ", 1)[1]) for line in per_camera]
    mean = [line for line in lines if line.startswith("mean psnr")]
    assert len(mean) == 1 and abs(float(mean[0].rsplit(" ", 1)[1]) - np.mean(values)) < 2e-3
    print("\n".join(per_camera + mean))
