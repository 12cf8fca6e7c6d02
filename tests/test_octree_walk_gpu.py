"""The K13 ray walk on the GPU (``OcTree.walk`` / ``spans`` / ``RaySampler.clip_to_octree``)
against the float64 restatement of its contract (tests/octree_walk_reference.py, itself pinned to
the reference's recorded paths by tests/test_octree_walk_cpu.py).  No reference file is read.

Leaf sequences are compared for EQUALITY on every ray whose margin (the shortest chord of a
region, near misses included) exceeds the f32 rounding of the kernel's plane crossings,
``4 (ulp(|plane| + |o|) / |d_axis| + ulp(t))`` from operand magnitudes (``budgets``); a ray below
it has no single right answer.  Such rays may be at most 2 % of a case -- asserted.

Two budgets are in use.  Entry t of every stop is held to the formula above on that stop's own
plane and axis.  Whether a ray is left out, and the fill values and spans, use the wider per-ray
``ray_budget``: the largest of the ray's crossing budgets and the same expression with the cube's
extent over the ray's smallest nonzero ``|d|`` -- the planes of near misses never show up as
crossings but the walk decides on them too.  The wider budget can only enlarge the set of rays
left out, which the 2 % cap bounds."""

import os

import numpy as np
import pytest
import torch

from tests import octree_walk_reference as wref
from tests.octree_walk_helpers import (LEFT_OUT_CAP, check_walk, opaque_ball, ray_budget,
                                       two_level_tree)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
SCENE = os.path.join(HERE, "golden", "scene16.npz")
TREES = ["shell", "planes", "nodata"]


def load_tree(name):
    import fourier_feature_nets as ffn
    with np.load(os.path.join(HERE, "golden", "octree.npz")) as g:
        return ffn.OcTree(float(g[name + "/scale"]), g[name + "/node_index"],
                          g[name + "/leaf_index"])


def golden_rays(name):
    """The rays of the recorded fixture (its inputs only; the answers are the restatement's)."""
    with np.load(os.path.join(HERE, "golden", "octree_walk.npz")) as g:
        return g[name + "/starts"], g[name + "/directions"]


@pytest.mark.parametrize("length", [64, 6])
@pytest.mark.parametrize("name", TREES)
def test_walk_equals_the_restatement_on_the_golden_trees(name, length):
    tree = load_tree(name)
    starts, directions = golden_rays(name)
    keep_s, keep_d = starts.copy(), directions.copy()
    path = tree.walk(starts, directions, length)
    assert type(path).__name__ == "Path" and path._fields == ("t_stops", "leaves")
    assert np.array_equal(starts, keep_s) and np.array_equal(directions, keep_d)
    w, _ = check_walk(name, tree.state_dict, starts, directions, length, path.t_stops, path.leaves)
    assert (path.leaves >= 0).any() and (~w["hit"]).any()


def big_cloud(depth, count=1 << 18):
    """Dense at the centre, sparse towards the faces: leaves at several depths."""
    rng = np.random.default_rng(1000 + depth)
    pos = (rng.random((count, 3), dtype=np.float32) * np.float32(2) - np.float32(1)) ** 5
    return pos


def camera_rays(rng, count, scale):
    """Pinhole-like rays from a few eyes around the cube (|o| 1.5 .. 2.5 scales) towards points
    inside it, and a tenth of them from inside."""
    eyes = rng.normal(size=(16, 3))
    eyes = eyes / np.linalg.norm(eyes, axis=1, keepdims=True) * rng.uniform(1.5, 2.5, (16, 1))
    o = eyes[rng.integers(0, 16, count)] * scale
    target = (rng.random((count, 3)) * 2 - 1) * scale * 1.1        # some pass by
    inside = rng.random(count) < 0.1
    o[inside] = (rng.random((int(inside.sum()), 3)) * 2 - 1) * scale * 0.9
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return o.astype(np.float32), d.astype(np.float32)


@pytest.mark.parametrize("depth", [6, 8, 10])
def test_walk_on_large_random_clouds(depth):
    import fourier_feature_nets as ffn
    pos = big_cloud(depth)
    tree = ffn.OcTree.build_from_samples(torch.from_numpy(pos).cuda(), depth, 4)
    assert tree.depth == depth and len(np.unique(tree.leaf_depths())) >= 2
    assert tree.center is not None and len(tree.center) == 3
    starts, directions = camera_rays(np.random.default_rng(depth), 100000, np.float32(tree.scale))
    path = tree.walk(starts, directions, 64)
    w, ok = check_walk("depth %d" % depth, tree.state_dict, starts, directions, 64, path.t_stops,
                       path.leaves)
    assert (np.diff(w["offsets"]) >= 63).any() or depth < 10       # the cap of 63 stops bites
    # spans, from the same restatement
    for t_min, pad in [(0.0, 0.0), (0.0, 1.0), (0.7, 2.5)]:
        t_in, t_out, hit = tree.spans(starts, directions, t_min, pad)
        assert t_in.dtype == np.float32 and hit.dtype == np.bool_
        want_in, want_out, want_hit = wref.spans(w, tree.scale, tree.depth, directions, t_min, pad)
        budget = ray_budget(w, tree.scale, starts, directions)
        # a leaf that ends within the budget of t_min may or may not count
        near_t_min = np.zeros(len(ok), bool)
        close = (w["leaf"] >= 0) & (np.abs(w["t_out"] - t_min) <= budget[w["ray"]])
        near_t_min[w["ray"][close]] = True
        rows = ok & ~near_t_min
        assert (1.0 - rows.mean()) <= LEFT_OUT_CAP
        assert np.array_equal(hit[rows], want_hit[rows])
        both = rows & want_hit
        width = np.abs(want_out - want_in) * 2.0 ** -22          # pad: one multiply, one add
        assert (np.abs(t_in - want_in) <= budget + width)[both].all()
        assert (np.abs(t_out - want_out) <= budget + width)[both].all()
        assert (t_in[~hit] == 0).all() and (t_out[~hit] == 0).all()
        print("depth %d spans(t_min %.1f, pad %.1f): %d of %d rays hit" %
              (depth, t_min, pad, hit.sum(), len(hit)))
    # pad widens by exactly pad finest-cell sides along the ray
    a_in, a_out, a_hit = tree.spans(starts, directions, 0.0, 0.0)
    b_in, b_out, b_hit = tree.spans(starts, directions, 0.0, 3.0)
    assert np.array_equal(a_hit, b_hit)
    side = 2.0 * np.float64(np.float32(tree.scale)) / 2 ** (tree.depth - 1)
    width = 3.0 * side / np.linalg.norm(directions.astype(np.float64), axis=1)
    slack = 4 * np.spacing(np.maximum(np.abs(b_in), np.abs(b_out)).astype(np.float32)) + 2.0 ** -22 * width
    assert (np.abs((a_in.astype(np.float64) - b_in) - width) <= slack)[a_hit].all()
    assert (np.abs((b_out.astype(np.float64) - a_out) - width) <= slack)[a_hit].all()


def test_input_forms_agree_and_bad_rays_terminate():
    tree = load_tree("shell")
    starts, directions = golden_rays("shell")
    host = tree.walk(starts, directions, 32)
    dev_s, dev_d = torch.from_numpy(starts).cuda(), torch.from_numpy(directions).cuda()
    keep_s, keep_d = dev_s.clone(), dev_d.clone()
    dev = tree.walk(dev_s, dev_d, 32)
    assert torch.is_tensor(dev.t_stops) and dev.t_stops.is_cuda and dev.leaves.dtype == torch.int64
    assert torch.equal(dev_s, keep_s) and torch.equal(dev_d, keep_d)
    assert np.array_equal(dev.leaves.cpu().numpy(), host.leaves)
    assert dev.t_stops.cpu().numpy().tobytes() == host.t_stops.tobytes()
    one = tree.walk(starts[0], directions[0], 32)                    # a single (3,) ray
    assert one.leaves.shape == (1, 32) and np.array_equal(one.leaves[0], host.leaves[0])
    spans_host = tree.spans(starts, directions)
    spans_dev = tree.spans(dev_s, dev_d)
    for a, b in zip(spans_host, spans_dev):
        assert b.is_cuda and np.array_equal(a, b.cpu().numpy())
    assert spans_dev[2].dtype == torch.bool
    # rays no walk can follow: they terminate and report a miss
    s = float(tree.scale)
    bad_s = np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [0, 0, 0], [2 * s, 0, 0],
                        [np.inf, 0, 0], [0, 0, 0]])
    bad_d = np.float32([[0, 0, 0], [1, 1, 1], [np.nan, 1, 0], [np.nan] * 3, [0, 1, 1],
                        [1, 0, 0], [np.inf, 1, 1]])
    for length in (2, 64):
        path = tree.walk(bad_s, bad_d, length)
        assert (path.leaves == -1).all()
    t_in, t_out, hit = tree.spans(bad_s, bad_d)
    assert not hit.any()
    # zero components inside their slabs are ordinary rays
    zs = np.float32([[-3 * s, 0.1 * s, 0.2 * s], [0.3 * s, 0.1 * s, -3 * s]])
    zd = np.float32([[1, 0, 0], [0, 0, 2]])
    path = tree.walk(zs, zd, 64)
    check_walk("zero components", tree.state_dict, zs, zd, 64, path.t_stops, path.leaves)


def test_hand_built_and_root_only_trees():
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    tree = ffn.OcTree(float(scale), nodes, leaves)
    starts = np.float32([[-2, -0.5, -0.5], [0.25, 0.3, -3], [0.2, 0.3, 0.1], [-2, -1.7, -1.9]])
    dirs = np.float32([[2, 0, 0], [0, 0, 1], [0, 0, -0.5], [1, 0.9, 1.1]])
    path = tree.walk(starts, dirs, 8)
    assert list(path.leaves[0][:3]) == [0, -1, -1] and np.allclose(path.t_stops[0], [0.5, 1] + [1.5] * 6)
    assert list(path.leaves[1][:4]) == [-1, 1, -1, -1] and np.allclose(path.t_stops[1][:4], [2, 3, 3.5, 4])
    assert list(path.leaves[2][:4]) == [-1, 1, -1, -1]
    assert np.allclose(path.t_stops[2][:4], [-1.8, -0.8, 0.2, 2.2], atol=1e-6)
    check_walk("two levels", tree.state_dict, starts, dirs, 8, path.t_stops, path.leaves)
    short = tree.walk(starts, dirs, 3)                               # at most 2 stops
    assert list(short.leaves[1]) == [-1, 1, -1] and np.allclose(short.t_stops[1], [2, 3, 4])
    root = ffn.OcTree(2.0, np.zeros(0, np.int64), np.array([0], np.int64))
    path = root.walk(np.float32([[-4, 0.5, 0.5], [0, 0, 0]]), np.float32([[1, 0, 0], [0, 0, 4]]), 4)
    assert list(path.leaves[:, 0]) == [0, 0] and (path.leaves[:, 1:] == -1).all()
    assert np.allclose(path.t_stops, [[2, 6, 6, 6], [-0.5, 0.5, 0.5, 0.5]])
    t_in, t_out, hit = root.spans(np.float32([[-4, 0.5, 0.5], [0, 0, 0]]),
                                  np.float32([[1, 0, 0], [0, 0, 4]]), 0.0, 0.0)
    assert hit.all() and np.allclose(t_in, [2, 0]) and np.allclose(t_out, [6, 0.5])


def test_clip_to_octree_on_a_voxelized_scene():
    """scene16 with the opaque ball of tests/test_octree_gpu.py, voxelized as
    test_voxelize_model_end_to_end does: the tree's spans hold the surface points."""
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
    positions, _, count = ops.octree_surface_points(alpha.contiguous(), depth.contiguous(), starts,
                                                    dirs, 0.3)
    count = int(count.item())
    assert count > 50
    surface = index[alpha > 0.3]
    tree = ffn.OcTree.build_from_samples(positions[:count].contiguous(), 5, 1)
    assert tree.point_leaf_ids.min().item() >= 0                     # every point built a leaf
    before = [t.clone() for t in (sampler.starts, sampler.directions, sampler.near_far, sampler.valid)]
    clipped = sampler.clip_to_octree(tree, tree.center)
    for was, now in zip(before, (sampler.starts, sampler.directions, sampler.near_far, sampler.valid)):
        assert torch.equal(was, now)
    assert clipped is not sampler and len(clipped) == len(sampler)
    valid = clipped.valid != 0
    assert (valid <= (sampler.valid != 0)).all() and 0 < valid.sum().item() < (sampler.valid != 0).sum().item()
    assert (clipped.near_far[0] >= sampler.near_far[0])[valid].all()
    assert (clipped.near_far[1] <= sampler.near_far[1])[valid].all()
    assert (clipped.near_far[0] < clipped.near_far[1])[valid].all()
    # the rays whose surface point built the tree are kept, and the point lies inside the span
    assert valid[surface].all()
    d_surface = depth[alpha > 0.3]
    assert (clipped.near_far[0][surface] <= d_surface).all()
    assert (clipped.near_far[1][surface] >= d_surface).all()
    # no hit -> invalid
    shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
    _, _, hit = tree.spans(sampler.starts - shift, sampler.directions)
    assert not valid[~hit].any()
    print("clip_to_octree: %d of %d valid rays kept, mean span %.3f of %.3f" %
          (valid.sum().item(), (sampler.valid != 0).sum().item(),
           (clipped.near_far[1] - clipped.near_far[0])[valid].mean().item(),
           (sampler.near_far[1] - sampler.near_far[0])[valid].mean().item()))
    # through the renderer, unchanged: the voxel model's three-pass path, and the one-launch fused
    # render of an MLP (render_image checks the kernel's own non-finite flag)
    clipped_caster = ffn.Raycaster(model)
    image = clipped_caster.render_image(clipped, 0, 4096)
    assert image.shape == (sampler.image_height, sampler.image_width, 3)
    torch.manual_seed(7)
    mlp = ffn.PositionalFourierMLP(3, 4, 5.5, num_channels=64, embedding_size=48).to("cuda")
    fused = ffn.Raycaster(mlp)
    assert fused._can_fuse(clipped)
    frame = fused.render_image(clipped, 0, 4096)
    full = fused.render_image(sampler, 0, 4096)
    assert frame.shape == full.shape == (sampler.image_height, sampler.image_width, 3)
    assert np.isfinite(frame).all() and np.isfinite(full).all()
    dropped = ~valid[:sampler.rays_per_camera].cpu().numpy()
    assert (frame.reshape(-1, 3)[dropped] == 0).all() and (full.reshape(-1, 3)[dropped] != 0).any()
    with torch.no_grad():
        rendered = fused.render_rays(clipped, clipped.valid_index(surface), include_depth=True)
    assert all(torch.isfinite(x).all() for x in rendered)
    near, far = clipped.near_far[:, clipped.valid_index(surface)]
    assert ((rendered.depth >= near - 1e-5) & (rendered.depth <= far + 1e-5)).all()
    with torch.no_grad():
        got = clipped_caster.render(clipped.sample(clipped.valid_index(surface), None), True)
    assert all(torch.isfinite(x).all() for x in got)
    assert (got[1] > 0.3).float().mean().item() > 0.9               # the ball is still there
