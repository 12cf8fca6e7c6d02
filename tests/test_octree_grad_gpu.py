"""K17 on the GPU: the gradient walk and the per-leaf sums (``ops.octree_render_volume_backward``),
the projection (``ops.octree_project``), ``OctreeField``, ``fit_octree`` and
``scripts/train_octree.py`` against the float64 restatement of the gradient contract
(tests/octree_grad_reference.py).  No reference file is read.

Every leaf's gradient is held against its budget (derived in the restatement).  Rays whose margin
does not exceed the per-ray budget of the K13 - K15 tests (``ray_budget``) are left out of both
sides by giving them a zero upstream gradient; at most 2 % of a case -- asserted."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_grad_reference as gref
from tests import octree_walk_reference as wref
from tests.octree_render_helpers import (LEFT_OUT_CAP, big_cloud, camera_rays, golden_rays,
                                         load_tree, ray_budget)
from tests.octree_volume_helpers import hand_case, random_leaf_data

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T_MINS = [0.0, float(np.float32(0.7))]
MIN_TS = [0.0, 1e-3]
BG = (0.25, 0.5, 0.125)
MID_SHARE = 0.30


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def device_gradient(tree, data, starts, dirs, d_color, d_alpha, t_min=0.0, background=BG,
                    min_t=0.0, workspace=None):
    from fourier_feature_nets_amd import ops
    state = tree.state_dict
    return ops.octree_render_volume_backward(
        cuda(starts), cuda(dirs), float(state["scale"]), tree.depth,
        cuda(state["node_index"], np.int64), cuda(state["leaf_index"], np.int64), cuda(data),
        cuda(d_color), cuda(d_alpha), float(t_min), background, float(min_t), workspace)


def upstream(count, seed, ok=None):
    rng = np.random.default_rng(seed)
    d_color = rng.normal(size=(count, 3)).astype(np.float32)
    d_alpha = rng.normal(size=count).astype(np.float32)
    if ok is not None:
        d_color[~ok] = 0
        d_alpha[~ok] = 0
    return d_color, d_alpha


def check_gradient(what, tree, data, starts, dirs, w, t_min, min_t, seed=9, share=True,
                   every_ray=False):
    """``every_ray``: the hand-worked rays, whose crossings are exact in f32 (the diagonal runs
    through cell corners, where the margin is 0 by construction)."""
    scale = tree.state_dict["scale"]
    ok = ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts, dirs))
    if every_ray:
        ok[:] = True
    left_out = 1.0 - ok.mean()
    d_color, d_alpha = upstream(len(starts), seed, ok)
    g = gref.gradient(w, scale, starts, dirs, data, d_color, d_alpha, t_min, BG, min_t)
    got = device_gradient(tree, data, starts, dirs, d_color, d_alpha, t_min, BG, min_t)
    assert got.shape == (len(data), 4) and got.dtype == torch.float32
    got = got.cpu().numpy()
    v = g["composite"]
    took = v["count"] > 0
    mid = took & (v["trans"] > 0.05) & (v["trans"] < 0.95)
    mid_share = mid.sum() / max(took.sum(), 1)
    err = np.abs(got.astype(np.float64) - g["grad"])
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(g["budget"] > 0, err / g["budget"], np.where(err > 0, np.inf, 0.0))
    print("%s t_min=%.2f min_T=%g: %d rays, %d take a leaf, %.3f of them end with 0.05 < T < 0.95, "
          "%.4f left out; %d of %d leaves taken; worst error / budget: colour %.3f sigma %.3f" %
          (what, t_min, min_t, len(starts), took.sum(), mid_share, left_out,
           (g["taken"] > 0).sum(), len(data), ratio[:, :3].max(), ratio[:, 3].max()))
    assert left_out <= LEFT_OUT_CAP
    if share:
        assert mid_share >= MID_SHARE
    assert np.isfinite(got).all()
    assert (err <= g["budget"]).all()
    assert (bits(got[g["taken"] == 0]) == 0).all()
    return got, g


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
    tree._center = bare.center
    starts, directions = camera_rays(np.random.default_rng(depth), 20000, np.float32(tree.scale))
    w = wref.walk(state["scale"], state["node_index"], state["leaf_index"], starts, directions)
    return tree, data, starts, directions, w


def test_hand_case():
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs = hand_case()
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    finite = data.copy()
    finite[2, 3] = 1.5
    tree = ffn.OcTree(float(scale), nodes, leaves, finite)
    for t_min in (0.0, 0.75):
        check_gradient("hand case", tree, finite, starts, dirs, w, t_min, 0.0, share=False,
                       every_ray=True)
    # the opaque leaf: finite everywhere, and nothing behind it matters -- on the diagonal ray
    # (leaves 0, 1, 2) T_{n+1} is 0, so only what lies BEHIND a leaf moves its density
    d_color, d_alpha = upstream(5, 2)
    solid = ffn.OcTree(float(scale), nodes, leaves, data)
    got = device_gradient(solid, data, starts, dirs, d_color, d_alpha).cpu().numpy()
    assert np.isfinite(got).all()
    assert got[2, 3] == 0                      # d sigma of the opaque leaf itself: T_{k+1} = 0
    only = np.zeros((5, 3), np.float32), np.zeros(5, np.float32)
    only[1][3] = 1.0                           # alpha only, on the diagonal ray: T_{n+1} = 0
    got = device_gradient(solid, data, starts, dirs, *only).cpu().numpy()
    assert (bits(got) == 0).all()


@pytest.mark.parametrize("min_t", MIN_TS)
@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", ["shell", "planes"])
def test_gradient_within_budget_on_the_golden_trees(name, t_min, min_t):
    tree, data, starts, directions, w = golden_case(name)
    check_gradient(name, tree, data, starts, directions, w, t_min, min_t)


@pytest.mark.parametrize("min_t", MIN_TS)
@pytest.mark.parametrize("t_min", T_MINS)
def test_gradient_within_budget_on_a_random_cloud(t_min, min_t):
    tree, data, starts, directions, w = cloud_case()
    check_gradient("depth 6", tree, data, starts, directions, w, t_min, min_t)


def test_forward_identity():
    import fourier_feature_nets as ffn
    tree, data, starts, directions, _ = cloud_case()
    field = ffn.OctreeField(tree)
    assert field.data.shape == (len(data), 4) and field.data.is_cuda and field.data.requires_grad
    dev_s, dev_d = cuda(starts), cuda(directions)
    for t_min, min_t in ((0.0, 0.0), (T_MINS[1], 1e-3)):
        want = tree.render_volume(dev_s, dev_d, t_min, BG, min_t)
        out = field(dev_s, dev_d, t_min, BG, min_t)
        assert type(out).__name__ == "RenderResult"
        for a, b in zip(out, want):
            assert torch.is_tensor(a) and a.is_cuda and np.array_equal(bits(a), bits(b))
    # autograd reaches the kernels
    out = field(dev_s, dev_d, 0.0, BG)
    d_color, d_alpha = upstream(len(starts), 4)
    (out.color * cuda(d_color)).sum().add((out.alpha * cuda(d_alpha)).sum()).backward()
    direct = device_gradient(tree, data, starts, directions, d_color, d_alpha)
    assert np.array_equal(bits(field.data.grad), bits(direct))
    again = field.tree()
    assert again is not tree and again.center == tree.center
    assert np.array_equal(again.state_dict["leaf_index"], tree.state_dict["leaf_index"])
    assert np.array_equal(bits(again.leaf_data()), bits(data))


def test_determinism():
    tree, data, starts, directions, _ = cloud_case()
    d_color, d_alpha = upstream(len(starts), 6)
    first = device_gradient(tree, data, starts, directions, d_color, d_alpha, 0.0, BG, 1e-3)
    second = device_gradient(tree, data, starts, directions, d_color, d_alpha, 0.0, BG, 1e-3)
    assert np.array_equal(bits(first), bits(second))
    # on a side stream, while the default stream renders
    side = torch.cuda.Stream()
    dev_s, dev_d = cuda(starts), cuda(directions)
    torch.cuda.synchronize()
    for _ in range(4):
        tree.render_volume(dev_s, dev_d, 0.0, BG)
    with torch.cuda.stream(side):
        third = device_gradient(tree, data, starts, directions, d_color, d_alpha, 0.0, BG, 1e-3)
    torch.cuda.synchronize()
    assert np.array_equal(bits(first), bits(third))


def test_skew():
    import fourier_feature_nets as ffn
    rng = np.random.default_rng(8)
    # one leaf, every ray through it
    root = ffn.OcTree(2.0, np.zeros(0, np.int64), np.array([0], np.int64),
                      np.float32([[0.5, 0.25, 1.0, 0.2]]))
    starts, dirs = camera_rays(rng, 4096, np.float32(2.0))
    state = root.state_dict
    w = wref.walk(state["scale"], state["node_index"], state["leaf_index"], starts, dirs)
    got, g = check_gradient("root only", root, root.leaf_data(), starts, dirs, w, 0.0, 0.0,
                            share=False)
    assert g["taken"][0] > 3000
    d_color, d_alpha = upstream(4096, 9, ~w["hit"] | (w["margin"] > ray_budget(w, 2.0, starts, dirs)))
    again = device_gradient(root, root.leaf_data(), starts, dirs, d_color, d_alpha, 0.0, BG)
    assert np.array_equal(bits(got), bits(again))
    # three leaves, every ray along the main diagonal
    scale, nodes, leaves, data, _, _ = hand_case()
    data = data.copy()
    data[2, 3] = 1.5
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    offset = (rng.random((4096, 1)) * 0.2).astype(np.float32)
    starts = np.float32([-2, -2, -2]) + offset * np.float32([1, -1, 0])
    dirs = np.tile(np.float32([1, 1, 1]), (4096, 1))
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    got, g = check_gradient("diagonal", tree, data, starts, dirs, w, 0.0, 0.0, share=False)
    assert g["taken"].max() > 1000
    d_color, d_alpha = upstream(4096, 9, ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts, dirs)))
    again = device_gradient(tree, data, starts, dirs, d_color, d_alpha, 0.0, BG)
    assert np.array_equal(bits(got), bits(again))


def test_edge_cases():
    import fourier_feature_nets as ffn
    scale, nodes, leaves, data, starts, dirs = hand_case()
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    d_color, d_alpha = upstream(5, 12)
    for stored in (-1.0, np.nan, 0.0):
        changed = data.copy()
        changed[2, 3] = 1.5
        changed[1, 3] = stored
        tree = ffn.OcTree(float(scale), nodes, leaves, changed)
        got = device_gradient(tree, changed, starts, dirs, d_color, d_alpha).cpu().numpy()
        g = gref.gradient(w, scale, starts, dirs, changed, d_color, d_alpha, 0.0, BG)
        assert (np.abs(got - g["grad"]) <= g["budget"]).all()
        if stored == 0.0:
            assert got[1, 3] != 0 and g["grad"][1, 3] != 0       # a leaf at 0 can come back
        else:
            assert got[1, 3] == 0
    # misses and NaN rays contribute nothing
    changed = data.copy()
    changed[2, 3] = 1.5
    tree = ffn.OcTree(float(scale), nodes, leaves, changed)
    bad_s = np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [2, 0, 0], [np.inf, 0, 0], [5, 5, 5]])
    bad_d = np.float32([[0, 0, 0], [1, 1, 1], [np.nan, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 0]])
    ones = np.ones((6, 3), np.float32), np.ones(6, np.float32)
    assert (bits(device_gradient(tree, changed, bad_s, bad_d, *ones)) == 0).all()
    mixed_s, mixed_d = np.concatenate([bad_s, starts]), np.concatenate([bad_d, dirs])
    up = np.concatenate([ones[0], d_color]), np.concatenate([ones[1], d_alpha])
    plain = device_gradient(tree, changed, starts, dirs, d_color, d_alpha)
    assert np.array_equal(bits(device_gradient(tree, changed, mixed_s, mixed_d, *up)), bits(plain))
    # one ray, and one more or less than a wave
    cloud, cloud_data, c_starts, c_dirs, cw = cloud_case()
    scale = cloud.state_dict["scale"]
    for count in (1, 63, 65):
        rows = slice(100, 100 + count)
        d_c, d_a = upstream(count, count)
        sub = wref.walk(scale, cloud.state_dict["node_index"], cloud.state_dict["leaf_index"],
                        c_starts[rows], c_dirs[rows])
        ok = ~sub["hit"] | (sub["margin"] > ray_budget(sub, scale, c_starts[rows], c_dirs[rows]))
        d_c[~ok] = 0
        d_a[~ok] = 0
        g = gref.gradient(sub, scale, c_starts[rows], c_dirs[rows], cloud_data, d_c, d_a, 0.0, BG)
        got = device_gradient(cloud, cloud_data, c_starts[rows], c_dirs[rows], d_c, d_a)
        got = got.cpu().numpy()
        assert (np.abs(got - g["grad"]) <= g["budget"]).all()
        assert (bits(got[g["taken"] == 0]) == 0).all()


def test_zero_upstream_gradient():
    from fourier_feature_nets_amd import ops
    tree, data, starts, directions, _ = cloud_case()
    dev_s, dev_d = cuda(starts), cuda(directions)
    out = tree.render_volume(dev_s, dev_d, 0.0, (0, 0, 0))
    rays = torch.arange(len(starts), dtype=torch.int64, device="cuda")
    count = len(starts)
    _, d_color, d_alpha = ops.mse_loss(out.color, out.alpha, out.color.clone(), out.alpha.clone(),
                                       rays, 1.0 / (3 * count), 0.1 / count)
    assert (bits(d_color) << 1 == 0).all() and (bits(d_alpha) << 1 == 0).all()
    state = tree.state_dict
    got = ops.octree_render_volume_backward(
        dev_s, dev_d, float(state["scale"]), tree.depth, cuda(state["node_index"], np.int64),
        cuda(state["leaf_index"], np.int64), cuda(data), d_color, d_alpha, 0.0, (0, 0, 0))
    assert (bits(got) << 1 == 0).all()


def test_one_step():
    """K7 then K17c on the GPU gradient, against torch.optim.Adam in float64 on the restatement's
    gradient (clipped as K7 clips), then the clamp.  Budget: the gradient's own budget scaled by
    the clip coefficient moves Adam's first step by at most lr * b / (|g| + eps) per element (the
    step is lr * g / (|g| + eps) at t = 1), plus 8 f32 roundings of the parameter."""
    from fourier_feature_nets_amd import ops
    tree, data, starts, directions, w = cloud_case()
    scale = tree.state_dict["scale"]
    ok = ~w["hit"] | (w["margin"] > ray_budget(w, scale, starts, directions))
    d_color, d_alpha = upstream(len(starts), 13, ok)
    d_color *= np.float32(1e-3)
    d_alpha *= np.float32(1e-3)
    g = gref.gradient(w, scale, starts, directions, data, d_color, d_alpha, 0.0, BG)
    grads = device_gradient(tree, data, starts, directions, d_color, d_alpha)
    lr, clip, max_norm, eps = 1e-2, 0.1, 0.1, 1e-8
    params = cuda(data)
    flat = params.view(-1)
    ops.clip_adam(flat, grads.view(-1), torch.zeros_like(flat), torch.zeros_like(flat), 1, lr,
                  clip_value=clip, max_norm=max_norm)
    ops.octree_project(params)
    got = params.cpu().numpy().astype(np.float64)
    want = torch.tensor(data.astype(np.float64), requires_grad=True)
    clipped = np.clip(g["grad"], -clip, clip)
    norm = np.sqrt((clipped ** 2).sum())
    coef = min(1.0, max_norm / (norm + 1e-6))
    want.grad = torch.tensor(clipped * coef)
    torch.optim.Adam([want], lr=lr, eps=eps).step()
    want = want.detach().numpy()
    want[:, :3] = np.clip(want[:, :3], 0.0, 1.0)
    want[:, 3] = np.maximum(want[:, 3], 0.0)
    moved = np.abs(clipped * coef)
    # at t = 1 the step is lr * g / (|g| + eps), whose slope in g is at most 1 / (|g| + eps); the
    # clip coefficient moves by at most the relative change of the norm
    coef_rel = np.sqrt((g["budget"] ** 2).sum()) / max(norm, 1e-30) + 1e-6
    budget = lr * (coef * g["budget"] + moved * coef_rel + 8 * 2.0 ** -24 * moved) / (moved + eps) \
        + 8 * 2.0 ** -24 * np.maximum(np.abs(data), lr)
    err = np.abs(got - want)
    print("one step: clip coefficient %.3g, worst error / budget %.3f" % (coef, (err / budget).max()))
    assert (err <= budget).all()
    assert (got[:, :3] >= 0).all() and (got[:, :3] <= 1).all() and (got[:, 3] >= 0).all()
    # the projection alone
    wild = cuda(np.float32([[-1, 2, np.nan, -3], [0.5, 1.0, 0.0, np.nan], [0.25, -0.0, 1.5, 7]]))
    ops.octree_project(wild)
    assert np.array_equal(wild.cpu().numpy(), np.float32([[0, 1, 0, 0], [0.5, 1, 0, 0],
                                                           [0.25, 0, 1, 7]]))


class _Sampler:
    """What ``fit_octree`` reads of a ``RaySampler``: one 'camera' holding every ray."""

    def __init__(self, starts, directions):
        self.starts, self.directions = starts, directions
        self.num_cameras, self.rays_per_camera = 1, starts.shape[0]


class _Dataset:
    def __init__(self, sampler, colors, alphas, alpha_weight=0.1):
        self.sampler, self.colors, self.alphas = sampler, colors, alphas
        self.alpha_weight = alpha_weight

    def _gt_alphas(self):
        return self.alphas


def test_fit_loop():
    import fourier_feature_nets as ffn
    tree, data, starts, directions, _ = cloud_case()
    center = np.float32(tree.center)
    dev_s, dev_d = cuda(starts + center), cuda(directions)
    target = tree.render_volume((dev_s - cuda(center)).contiguous(), dev_d, 0.0, (0, 0, 0))
    dataset = _Dataset(_Sampler(dev_s, dev_d), target.color.contiguous(), target.alpha.contiguous())
    noise = np.random.default_rng(14).normal(size=data.shape).astype(np.float32)
    start = data.copy()
    start[:, :3] = np.clip(data[:, :3] + 0.2 * noise[:, :3], 0, 1)
    start[:, 3] = np.maximum(data[:, 3] * (1 + 0.5 * noise[:, 3]), 0)
    state = tree.state_dict
    begin = ffn.OcTree(state["scale"], state["node_index"], state["leaf_index"], start)
    steps = 300
    fitted, log = ffn.fit_octree(begin, dataset, dataset, 4096, num_steps=steps,
                                 report_interval=150, center=tree.center, verbose=False)
    assert len(log) == steps and [e.step for e in log] == list(range(steps))
    assert np.array_equal(fitted.state_dict["leaf_index"], state["leaf_index"])
    assert np.array_equal(begin.leaf_data(), start) and fitted.center == tree.center
    losses = np.array([e.loss for e in log])
    assert np.isfinite(losses).all()
    first, middle, last = losses[:16].mean(), losses[steps // 2:steps // 2 + 16].mean(), \
        losses[-16:].mean()
    reports = [e for e in log if not np.isnan(e.val_psnr)]
    print("fit loop: loss %.6g at step 0, %.6g at the midpoint, %.6g at the end; val psnr %.2f -> "
          "%.2f" % (first, middle, last, reports[0].val_psnr, reports[-1].val_psnr))
    assert last < middle < first
    assert [e.step for e in reports] == list(range(10)) + [150]
    out = fitted.leaf_data()
    assert (out[:, :3] >= 0).all() and (out[:, :3] <= 1).all() and (out[:, 3] >= 0).all()


def test_train_octree_program(tmp_path):
    import fourier_feature_nets as ffn
    data_path, tree_path, out_path = [str(tmp_path / name) for name in
                                      ("data.npz", "tree.npz", "out.npz")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_synthetic_npz.py"),
                          data_path, "--size", "8", "--cameras", "4"], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    scale, nodes, leaves, data, _, _ = hand_case()
    data = data.copy()
    data[2, 3] = 1.5
    ffn.OcTree(float(scale), nodes, leaves, data).save(tree_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_octree.py"),
                          tree_path, data_path, out_path, "--center", "0", "0", "0", "--steps",
                          "20", "--batch-size", "64", "--min-transmittance", "1e-3"],
                         capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "3 leaves fitted" in res.stdout
    fitted = ffn.OcTree.load(out_path)
    assert np.array_equal(fitted.state_dict["node_index"], nodes)
    assert np.array_equal(fitted.state_dict["leaf_index"], leaves)
    out = fitted.leaf_data()
    assert out.shape == (3, 4) and out.dtype == np.float32 and not np.array_equal(out, data)
