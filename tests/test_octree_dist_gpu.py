"""K29 on the GPU: the per-ray distortion (``ops.octree_distortion``), its gradient folded into the
backward walks (``dist_scale`` / ``ray_distortion`` on ``ops.octree_render_volume_backward`` and
``ops.octree_render_volume_sh_backward``), ``OcTree.distortion``, the fields, ``dist_weight`` on the
fit loops and ``scripts/train_octree.py --dist-weight`` against the float64 restatement
(tests/octree_dist_reference.py) and its derived budgets, on the cases of the K17 tests.  No
reference file is read.

Rays whose margin does not exceed the per-ray budget of the K13 - K15 tests (``ray_budget``) have
no single right answer.  The distortion's gradient has no upstream to zero, so they are left out of
both sides by not being walked: the kernels get the other rays only, and the restatement sums those.
At most 2 % of a case -- asserted."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_dist_reference as dref
from tests import octree_grad_reference as gref
from tests import octree_walk_reference as wref
from tests.octree_dist_helpers import CASES, MIN_TS, T_MINS, Case, case
from tests.octree_lattice_helpers import lattice_rays, mixed_tree
from tests.octree_render_helpers import LEFT_OUT_CAP, camera_rays

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = (0.25, 0.5, 0.125)
STRIDE = {1: 16, 2: 28}


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def geometry(c):
    return (float(c.scale), c.depth, cuda(c.nodes, np.int64), cuda(c.leaves, np.int64))


def sh_rows(sigma, degree, seed=3):
    """Device rows of ``degree`` carrying the densities ``sigma`` and seeded coefficients."""
    from fourier_feature_nets_amd import ops
    channels = ops.octree_sh_channels(degree)
    data = np.random.default_rng(seed).normal(size=(len(sigma), channels)).astype(np.float32)
    data[:, -1] = sigma
    return ops.octree_sh_device_layout(data, degree)


def device_distortion(c, rows, offset, starts, dirs, t_min=0.0, min_t=0.0):
    from fourier_feature_nets_amd import ops
    return ops.octree_distortion(cuda(starts), cuda(dirs), *geometry(c), cuda(rows),
                                 rows.shape[1], offset, float(t_min), float(min_t))


def device_backward(c, data, starts, dirs, d_color, d_alpha, t_min=0.0, min_t=0.0, dist_scale=0.0,
                    want_d=True, degree=None):
    """-> d rows (numpy), and the (N,) ``ray_distortion`` tensor the backward filled."""
    from fourier_feature_nets_amd import ops
    ray_d = torch.full((len(starts),), -1.0, dtype=torch.float32, device="cuda") if want_d else None
    head = (cuda(starts), cuda(dirs), *geometry(c), cuda(data))
    tail = (cuda(d_color), cuda(d_alpha), float(t_min), BG, float(min_t))
    if degree is None:
        got = ops.octree_render_volume_backward(*head, *tail, dist_scale=dist_scale,
                                                ray_distortion=ray_d)
    else:
        got = ops.octree_render_volume_sh_backward(*head, degree, *tail, dist_scale=dist_scale,
                                                   ray_distortion=ray_d)
    return got.cpu().numpy(), ray_d


def zeros(count):
    return np.zeros((count, 3), np.float32), np.zeros(count, np.float32)


@functools.lru_cache(maxsize=None)
def reference(name, t_min, min_t):
    c = case(name)
    return dref.distortion(c.w, c.scale, c.starts, c.dirs, c.sigma, t_min, min_t, keep=c.ok)


def worst(err, budget):
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(np.where(budget > 0, err / budget, np.where(err > 0, np.inf, 0.0)).max())


def check_case(name, t_min, min_t):
    """The forward, the backward with zero upstream and ``dist_scale = 1``, and their bits."""
    c = case(name)
    ref = reference(name, t_min, min_t)
    ok = c.ok
    assert 1.0 - ok.mean() <= LEFT_OUT_CAP
    starts, dirs = c.starts[ok], c.dirs[ok]
    got = device_distortion(c, c.data, 3, starts, dirs, t_min, min_t)
    assert got.shape == (len(starts),) and got.dtype == torch.float32
    again = device_distortion(c, c.data, 3, starts, dirs, t_min, min_t)
    assert np.array_equal(bits(got), bits(again))
    d = got.cpu().numpy().astype(np.float64)
    err_d = np.abs(d - ref["dist"][ok])
    grad, ray_d = device_backward(c, c.data, starts, dirs, *zeros(len(starts)), t_min, min_t, 1.0)
    err_g = np.abs(grad[:, 3].astype(np.float64) - ref["grad"])
    print("%s t_min=%.2f min_T=%g: %d rays, %.4f left out, mean D %.4g; worst error / budget: "
          "D %.3f, d sigma %.3f; %d of %d leaves taken"
          % (name, t_min, min_t, len(c.starts), 1.0 - ok.mean(), ref["dist"][ok].mean(),
             worst(err_d, ref["budget_d"][ok]), worst(err_g, ref["budget_g"]),
             (ref["taken"] > 0).sum(), len(c.leaves)))
    assert np.isfinite(d).all() and (d >= -ref["budget_d"][ok]).all()
    assert (err_d <= ref["budget_d"][ok]).all()
    assert (bits(got)[ref["count"][ok] == 0] == 0).all()         # +0 for a ray that takes nothing
    assert grad.shape == (len(c.leaves), 4) and np.isfinite(grad).all()
    assert (bits(grad[:, :3]) == 0).all()                        # colours do not enter
    assert (err_g <= ref["budget_g"]).all()
    assert (bits(grad[ref["taken"] == 0]) == 0).all()
    assert np.array_equal(bits(ray_d), bits(got))                # phase 0 of K29b has K29a's bits
    return c, ref, got


def test_hand_case():
    for t_min in (0.0, 0.75):
        c = case("hand")
        ref = dref.distortion(c.w, c.scale, c.starts, c.dirs, c.sigma, t_min)
        got = device_distortion(c, c.data, 3, c.starts, c.dirs, t_min).cpu().numpy()
        assert (np.abs(got - ref["dist"]) <= ref["budget_d"]).all() and got[2] == 0
    check_case("hand", 0.0, 0.0)


@pytest.mark.parametrize("min_t", MIN_TS)
@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", CASES)
def test_forward_and_zero_upstream_backward_within_budget(name, t_min, min_t):
    check_case(name, t_min, min_t)


@pytest.mark.parametrize("min_t", MIN_TS)
@pytest.mark.parametrize("t_min", T_MINS)
@pytest.mark.parametrize("name", CASES)
def test_backward_with_random_upstream(name, t_min, min_t):
    """Each leaf within (K17's budget + s * the distortion's) of (K17's gradient + s * the
    distortion's), all four columns; the colour columns are K17's alone."""
    c = case(name)
    ref = reference(name, t_min, min_t)
    ok = c.ok
    s = 0.375
    rng = np.random.default_rng(17)
    d_color = rng.normal(size=(len(c.starts), 3)).astype(np.float32)
    d_alpha = rng.normal(size=len(c.starts)).astype(np.float32)
    d_color[~ok] = 0
    d_alpha[~ok] = 0
    k17 = gref.gradient(c.w, c.scale, c.starts, c.dirs, c.data, d_color, d_alpha, t_min, BG, min_t)
    got, _ = device_backward(c, c.data, c.starts[ok], c.dirs[ok], d_color[ok], d_alpha[ok], t_min,
                             min_t, s, want_d=False)
    want = k17["grad"].copy()
    want[:, 3] += s * ref["grad"]
    budget = k17["budget"].copy()
    budget[:, 3] += s * ref["budget_g"]
    err = np.abs(got.astype(np.float64) - want)
    print("%s t_min=%.2f min_T=%g, dist_scale %g: worst error / budget: colour %.3f sigma %.3f"
          % (name, t_min, min_t, s, worst(err[:, :3], budget[:, :3]), worst(err[:, 3], budget[:, 3])))
    assert np.isfinite(got).all() and (err <= budget).all()
    plain, _ = device_backward(c, c.data, c.starts[ok], c.dirs[ok], d_color[ok], d_alpha[ok],
                               t_min, min_t, 0.0, want_d=False)
    assert np.array_equal(bits(got[:, :3]), bits(plain[:, :3]))
    # the term is there: a leaf whose distortion gradient exceeds both budgets moved
    moved = s * np.abs(ref["grad"]) > 2 * budget[:, 3]
    assert (got[moved, 3] != plain[moved, 3]).all()


@pytest.mark.parametrize("degree", [1, 2])
@pytest.mark.parametrize("name", ["planes", "depth4"])
def test_sh_rows(name, degree):
    """SH rows carrying the same densities: the d sigma column within the distortion's budget with
    zero upstream, every coefficient column bit-zero, and D bit for bit the plain rows'."""
    c = case(name)
    ref = reference(name, 0.0, 1e-3)
    ok = c.ok
    starts, dirs = c.starts[ok], c.dirs[ok]
    rows = sh_rows(c.sigma, degree)
    assert rows.shape[1] == STRIDE[degree]
    plain = device_distortion(c, c.data, 3, starts, dirs, 0.0, 1e-3)
    wide = device_distortion(c, rows, 0, starts, dirs, 0.0, 1e-3)
    assert np.array_equal(bits(plain), bits(wide))
    grad, ray_d = device_backward(c, rows, starts, dirs, *zeros(len(starts)), 0.0, 1e-3, 1.0,
                                  degree=degree)
    assert np.array_equal(bits(ray_d), bits(plain))
    assert grad.shape == rows.shape and (bits(grad[:, 1:]) == 0).all()
    err = np.abs(grad[:, 0].astype(np.float64) - ref["grad"])
    print("%s degree %d: worst d sigma error / budget %.3f" % (name, degree,
                                                               worst(err, ref["budget_g"])))
    assert (err <= ref["budget_g"]).all()
    # with upstream: the d sigma column moves by the term, the coefficient columns do not
    rng = np.random.default_rng(5)
    up = rng.normal(size=(len(starts), 3)).astype(np.float32), rng.normal(size=len(starts)).astype(np.float32)
    with_term, _ = device_backward(c, rows, starts, dirs, *up, 0.0, 1e-3, 0.5, degree=degree)
    without, _ = device_backward(c, rows, starts, dirs, *up, 0.0, 1e-3, 0.0, want_d=False,
                                 degree=degree)
    assert np.array_equal(bits(with_term[:, 1:]), bits(without[:, 1:]))
    assert not np.array_equal(bits(with_term[:, 0]), bits(without[:, 0]))


@pytest.mark.parametrize("count", [1, 63, 64, 65, 129])
def test_ray_counts_around_a_wave(count):
    c = case("cloud")
    rows = np.nonzero(c.ok)[0][100:100 + count]
    starts, dirs = c.starts[rows], c.dirs[rows]
    sub = wref.walk(c.scale, c.nodes, c.leaves, starts, dirs)
    ref = dref.distortion(sub, c.scale, starts, dirs, c.sigma)
    got = device_distortion(c, c.data, 3, starts, dirs)
    assert (np.abs(got.cpu().numpy() - ref["dist"]) <= ref["budget_d"]).all()
    grad, ray_d = device_backward(c, c.data, starts, dirs, *zeros(count), dist_scale=1.0)
    assert np.array_equal(bits(ray_d), bits(got))
    assert (np.abs(grad[:, 3] - ref["grad"]) <= ref["budget_g"]).all()
    assert (bits(grad[ref["taken"] == 0]) == 0).all() and (bits(grad[:, :3]) == 0).all()


def test_root_only_tree_misses_and_inside_starts():
    rng = np.random.default_rng(8)
    starts, dirs = camera_rays(rng, 512, np.float32(2.0))       # a tenth start inside, some miss
    starts = np.concatenate([starts, np.float32([[5, 5, 5], [0.5, 0.25, -0.5]])])
    dirs = np.concatenate([dirs, np.float32([[1, 0, 0], [0, 0, 1]])])
    data = np.float32([[0.5, 0.25, 1.0, 0.4]])
    c = Case(2.0, np.zeros(0, np.int64), np.array([0], np.int64), data, starts, dirs)
    assert c.depth == 1 and (~c.w["hit"]).any() and 1.0 - c.ok.mean() <= LEFT_OUT_CAP
    ok = c.ok
    ref = dref.distortion(c.w, c.scale, starts, dirs, c.sigma, keep=ok)
    got = device_distortion(c, data, 3, starts[ok], dirs[ok]).cpu().numpy()
    assert (np.abs(got - ref["dist"][ok]) <= ref["budget_d"][ok]).all()
    assert (bits(got)[~c.w["hit"][ok]] == 0).all()              # a miss: +0
    inside = np.nonzero(ok)[0] == len(starts) - 1
    # from inside, along +z: one leaf from t = 0 to the face at z = 2, D = w^2 L / 3 with L = 2.5
    weight = 1.0 - np.exp(-0.4 * 2.5)
    assert abs(got[inside][0] - weight * weight * 2.5 / 3.0) <= ref["budget_d"][ok][inside][0]
    grad, _ = device_backward(c, data, starts[ok], dirs[ok], *zeros(int(ok.sum())), dist_scale=1.0)
    assert (bits(grad[:, :3]) == 0).all()
    assert abs(grad[0, 3] - ref["grad"][0]) <= ref["budget_g"][0]


def test_opaque_negative_nan_and_zero_densities():
    c = case("hand")
    diagonal = slice(3, 4)                       # leaves 0, 1, 2 in this order
    # the first leaf opaque: T reaches 0, the later leaves are untaken, everything is finite
    data = c.data.copy()
    data[0, 3] = 1e30
    got = device_distortion(c, data, 3, c.starts[diagonal], c.dirs[diagonal]).cpu().numpy()
    length = np.sqrt(3.0)
    assert np.isfinite(got).all() and abs(got[0] - length / 3.0) <= 1e-6
    grad, ray_d = device_backward(c, data, c.starts[diagonal], c.dirs[diagonal], *zeros(1),
                                  dist_scale=1.0)
    assert np.isfinite(grad).all() and (bits(grad[1:]) == 0).all() and (bits(grad[:, :3]) == 0).all()
    assert np.array_equal(bits(ray_d), bits(got))
    # a negative and a NaN density pass as sigma = 0 with a gradient of exactly 0
    for stored in (-1.0, np.nan):
        data = c.data.copy()
        data[1, 3] = stored
        ref = dref.distortion(c.w, c.scale, c.starts, c.dirs, data[:, 3])
        got = device_distortion(c, data, 3, c.starts, c.dirs).cpu().numpy()
        assert np.isfinite(got).all() and (np.abs(got - ref["dist"]) <= ref["budget_d"]).all()
        grad, _ = device_backward(c, data, c.starts, c.dirs, *zeros(5), dist_scale=1.0)
        assert np.isfinite(grad).all() and bits(grad[1:2, 3])[0] << 1 == 0
        assert (np.abs(grad[:, 3] - ref["grad"]) <= ref["budget_g"]).all()
        assert grad[0, 3] != 0 and grad[2, 3] != 0
    # all-zero densities: D and the gradient are bit-zero
    data = c.data.copy()
    data[:, 3] = 0
    assert (bits(device_distortion(c, data, 3, c.starts, c.dirs)) == 0).all()
    grad, ray_d = device_backward(c, data, c.starts, c.dirs, *zeros(5), dist_scale=1.0)
    assert (bits(grad) == 0).all() and (bits(ray_d) == 0).all()


def test_exact_lattice_rays():
    """Rays whose every crossing is exact in f32 and ties all the time: every ray is kept."""
    from tests.octree_volume_helpers import random_leaf_data
    scale, nodes, leaves = mixed_tree()
    starts, dirs = lattice_rays(scale, 5, 1500, 29)
    c = Case(scale, nodes, leaves, random_leaf_data(scale, leaves, seed=29), starts, dirs,
             every_ray=True)
    ref = dref.distortion(c.w, c.scale, starts, dirs, c.sigma)
    assert (ref["count"] > 2).sum() > 100
    got = device_distortion(c, c.data, 3, starts, dirs)
    err = np.abs(got.cpu().numpy() - ref["dist"])
    grad, ray_d = device_backward(c, c.data, starts, dirs, *zeros(len(starts)), dist_scale=1.0)
    err_g = np.abs(grad[:, 3] - ref["grad"])
    print("lattice: worst error / budget: D %.3f, d sigma %.3f"
          % (worst(err, ref["budget_d"]), worst(err_g, ref["budget_g"])))
    assert (err <= ref["budget_d"]).all() and (err_g <= ref["budget_g"]).all()
    assert np.array_equal(bits(ray_d), bits(got)) and (bits(grad[ref["taken"] == 0]) == 0).all()


def plain_tree(c, data=None):
    import fourier_feature_nets as ffn
    tree = ffn.OcTree(c.scale, c.nodes, c.leaves, c.data if data is None else data)
    tree._center = (0.0, 0.0, 0.0)
    return tree


def sh_tree(c, degree):
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    data = ops.octree_sh_file_layout(sh_rows(c.sigma, degree), degree)
    tree = ffn.OcTree(c.scale, c.nodes, c.leaves, data, sh_degree=degree)
    tree._center = (0.0, 0.0, 0.0)
    return tree


def test_directional_derivative_through_the_public_api():
    """<kernel gradient, v> against the restatement's central difference of sum_r D_r along a
    seeded direction v; tolerance: the summed budget and the restatement's own Richardson estimate."""
    import fourier_feature_nets as ffn
    c = case("depth4")
    ok = c.ok
    tree = plain_tree(c)
    starts, dirs = c.starts[ok], c.dirs[ok]
    by_tree = tree.distortion(starts, dirs)
    assert isinstance(by_tree, np.ndarray) and by_tree.shape == (len(starts),)
    assert np.array_equal(bits(by_tree), bits(device_distortion(c, c.data, 3, starts, dirs)))
    for degree in (1, 2):
        assert np.array_equal(bits(sh_tree(c, degree).distortion(cuda(starts), cuda(dirs))),
                              bits(by_tree))
    field = ffn.OctreeField(tree)
    ray_d = torch.empty((len(starts),), dtype=torch.float32, device="cuda")
    grad = field.backward(cuda(starts), cuda(dirs), *[cuda(z) for z in zeros(len(starts))],
                          dist_scale=1.0, ray_distortion=ray_d).cpu().numpy()
    assert np.array_equal(bits(ray_d), bits(by_tree))
    v = np.random.default_rng(31).normal(size=len(c.leaves))
    sigma = c.sigma.astype(np.float64)
    sub = wref.walk(c.scale, c.nodes, c.leaves, starts, dirs)
    ref = dref.distortion(sub, c.scale, starts, dirs, sigma)

    def fd(eps):
        return (dref.ray_distortion(sub, starts, dirs, sigma + eps * v)
                - dref.ray_distortion(sub, starts, dirs, sigma - eps * v)).sum() / (2.0 * eps)

    # the step keeps every density positive: sigma = max(stored, 0) stays smooth
    eps = 0.25 * float((sigma[sigma > 0] / np.abs(v[sigma > 0])).min())
    coarse, fine = fd(eps), fd(0.5 * eps)
    got = float((grad[:, 3].astype(np.float64) * v).sum())
    allowed = float((np.abs(v) * ref["budget_g"]).sum()) + abs(coarse - fine)
    print("directional: kernel %.9g, restatement analytic %.9g, FD %.9g (Richardson %.3g), "
          "allowed %.3g" % (got, float((ref["grad"] * v).sum()), fine, abs(coarse - fine), allowed))
    assert (sigma > 0).all() and abs(got - fine) <= allowed


# ------------------------------------------------------------------------------------ the fit
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


def fit_setup(degree=None):
    """The depth-4 case: targets rendered from the tree itself, the fit started from other data."""
    c = case("depth4")
    truth = plain_tree(c) if degree is None else sh_tree(c, degree)
    dev_s, dev_d = cuda(c.starts), cuda(c.dirs)
    target = truth.render_volume(dev_s, dev_d, 0.0, (0, 0, 0))
    dataset = _Dataset(_Sampler(dev_s, dev_d), target.color.contiguous(), target.alpha.contiguous())
    start = np.asarray(truth.leaf_data()).copy()
    start[:, -1 if degree is not None else 3] *= np.float32(1.5)
    import fourier_feature_nets as ffn
    begin = ffn.OcTree(c.scale, c.nodes, c.leaves, start, degree)
    begin._center = (0.0, 0.0, 0.0)
    return c, begin, dataset


def same_fit(a, b):
    (tree_a, log_a), (tree_b, log_b) = a, b
    assert np.array_equal(bits(tree_a.leaf_data()), bits(tree_b.leaf_data()))
    assert len(log_a) == len(log_b)
    for x, y in zip(log_a, log_b):
        assert x.step == y.step and np.float64(x.loss).tobytes() == np.float64(y.loss).tobytes()
        assert np.float64(x.val_psnr).tobytes() == np.float64(y.val_psnr).tobytes()


@pytest.mark.parametrize("degree", [None, 1])
def test_dist_weight_zero_is_the_fit_without_the_argument(degree, capsys):
    import fourier_feature_nets as ffn
    _, begin, dataset = fit_setup(degree)
    fit = ffn.fit_octree if degree is None else ffn.fit_octree_sh
    kwargs = dict(batch_size=256, num_steps=4, report_interval=2, min_transmittance=1e-3)
    without = fit(begin, dataset, dataset, **kwargs)
    printed = capsys.readouterr().out
    with_zero = fit(begin, dataset, dataset, dist_weight=0.0, **kwargs)
    printed_zero = capsys.readouterr().out
    same_fit(without, with_zero)
    assert "dist:" not in printed and "dist:" not in printed_zero
    strip = lambda text: [line.split("s/step")[1].split("eta:")[0] for line in text.splitlines()]  # noqa: E731
    assert strip(printed) == strip(printed_zero) and len(strip(printed)) == 4


def test_fit_with_the_term(monkeypatch, capsys):
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import octree_fit, ops
    c, begin, dataset = fit_setup()
    weight, seed, batch = 0.05, 77, 256
    kwargs = dict(batch_size=batch, num_steps=3, report_interval=2, seed=seed, dist_weight=weight)
    seen = []
    real = ops.clip_adam

    def spy(params, grads, *args, **kw):
        seen.append(grads.clone())
        return real(params, grads, *args, **kw)

    monkeypatch.setattr(octree_fit.ops, "clip_adam", spy)
    fitted, log = ffn.fit_octree(begin, dataset, dataset, **kwargs)
    monkeypatch.setattr(octree_fit.ops, "clip_adam", real)
    printed = capsys.readouterr().out
    assert len(log) == 3 and np.isfinite([e.loss for e in log]).all()
    assert np.isfinite(fitted.leaf_data()).all() and printed.count("dist:") == 3
    # the first step's gradient: the field's backward with dist_scale = dist_weight / count
    generator = torch.Generator(device="cuda")
    generator.manual_seed(seed)
    rays = torch.randperm(len(c.starts), generator=generator, device="cuda")[:batch]
    starts = dataset.sampler.starts[rays].contiguous()
    dirs = dataset.sampler.directions[rays].contiguous()
    field = ffn.OctreeField(begin)
    color, alpha, _ = field._render(field.data.detach(), starts, dirs, 0.0, (0.0, 0.0, 0.0), 0.0)
    _, d_color, d_alpha = ops.mse_loss(color, alpha, dataset.colors, dataset.alphas, rays,
                                       1.0 / (3 * batch), 0.1 / batch)
    want = field.backward(starts, dirs, d_color, d_alpha, dist_scale=weight / batch)
    assert np.array_equal(bits(seen[0]).reshape(-1), bits(want).reshape(-1))
    off = field.backward(starts, dirs, d_color, d_alpha)
    assert not np.array_equal(bits(off[:, 3]), bits(want[:, 3]))
    assert np.array_equal(bits(off[:, :3]), bits(want[:, :3]))
    # rounds = 0 of the adaptive fit is the plain fit with the same argument
    again = ffn.fit_octree(begin, dataset, dataset, verbose=False, **kwargs)
    adaptive = ffn.fit_octree_adaptive(begin, dataset, dataset, rounds=0, verbose=False, **kwargs)
    assert adaptive[2] == []
    same_fit((fitted, log), again)
    same_fit(again, adaptive[:2])
    # and the SH loop runs with it
    _, sh_begin, sh_dataset = fit_setup(2)
    sh_fitted, sh_log = ffn.fit_octree_sh(sh_begin, sh_dataset, None, batch_size=batch, num_steps=3,
                                          dist_weight=weight, verbose=False)
    assert len(sh_log) == 3 and np.isfinite([e.loss for e in sh_log]).all()
    assert sh_fitted.sh_degree == 2 and np.isfinite(sh_fitted.leaf_data()).all()


def test_train_octree_program_with_dist_weight(tmp_path):
    import fourier_feature_nets as ffn
    data_path, tree_path, out_path = [str(tmp_path / name) for name in
                                      ("data.npz", "tree.npz", "out.npz")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_synthetic_npz.py"),
                          data_path, "--size", "8", "--cameras", "4"], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    c = case("hand")
    ffn.OcTree(c.scale, c.nodes, c.leaves, c.data).save(tree_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_octree.py"),
                          tree_path, data_path, out_path, "--center", "0", "0", "0", "--steps",
                          "12", "--batch-size", "64", "--dist-weight", "0.01"],
                         capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "distortion prior: 0.01" in res.stdout and "dist:" in res.stdout
    assert "3 leaves fitted" in res.stdout
    out = ffn.OcTree.load(out_path).leaf_data()
    assert out.shape == (3, 4) and np.isfinite(out).all()
