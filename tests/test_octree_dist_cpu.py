"""K29 without a GPU: the float64 restatement of the distortion contract
(tests/octree_dist_reference.py) against closed forms and its own finite differences, that its budget
tells a wrong gradient from the right one on every case of the GPU tests, the argument checks of the
C ABI and of the fit loops, and the dispatch of ``dist_weight = 0`` to the entries without the term."""

import ctypes
import os
import types

import numpy as np
import pytest
import torch

from tests import octree_dist_reference as dref
from tests import octree_walk_reference as wref
from tests.octree_dist_helpers import CASES, MIN_TS, T_MINS, case
from tests.octree_lattice_helpers import grid_tree


def weights_of(lengths, sigmas):
    """w and T_{k+1} of consecutive taken leaves, in float64."""
    trans, out = 1.0, []
    for length, sigma in zip(lengths, sigmas):
        a = 1.0 - np.exp(-(sigma * length))
        out.append(trans * a)
        trans *= 1.0 - a
    return out


def test_closed_forms():
    c = case("hand")
    full = dref.distortion(c.w, c.scale, c.starts, c.dirs, c.sigma)
    # rays 0, 1 and 4 take one leaf each: D = w^2 L / 3 (world lengths 1, 0.5 and 0.5)
    for ray, leaf, length in ((0, 0, 1.0), (1, 1, 0.5), (4, 2, 0.5)):
        (weight,) = weights_of([length], [float(c.sigma[leaf])])
        assert full["count"][ray] == 1
        assert abs(full["dist"][ray] - weight * weight * length / 3.0) <= 1e-15
    # ray 2 takes nothing
    assert full["count"][2] == 0 and full["dist"][2] == 0.0 and full["budget_d"][2] == 0.0
    assert (full["dist"] >= 0).all()
    # two leaves with a gap: the cells 0 and 2 of a row of four along x, a ray along +x
    nodes, leaves = grid_tree(3, [(2, 0, 1, 1), (2, 2, 1, 1)])
    starts, dirs = np.float32([[-3.0, -0.25, -0.25]]), np.float32([[2.0, 0.0, 0.0]])
    w = wref.walk(2.0, nodes, leaves, starts, dirs)
    sigma = np.float64([0.8, 1.7])
    got = dref.distortion(w, 2.0, starts, dirs, sigma)
    # cell sides of 1: the leaves span x in [-2, -1] and [0, 1], lengths 1 from the start at x = -3
    w1, w2 = weights_of([1.0, 1.0], sigma)
    m1, m2 = 1.5, 3.5
    want = 2.0 * w1 * w2 * (m2 - m1) + (w1 * w1 * 1.0 + w2 * w2 * 1.0) / 3.0
    assert got["count"][0] == 2 and abs(got["dist"][0] - want) <= 1e-15
    # the pairwise form on a ray of three leaves
    ray = 3
    lengths = np.sqrt(3.0) * np.float64([1.0, 0.5, 0.5])
    mids = np.sqrt(3.0) * np.float64([1.5, 2.25, 2.75])
    ws = np.float64(weights_of(lengths, c.sigma[:3].astype(np.float64)))
    pairs = (ws[:, None] * ws[None, :] * np.abs(mids[:, None] - mids[None, :])).sum()
    assert abs(full["dist"][ray] - (pairs + (ws * ws * lengths).sum() / 3.0)) <= 1e-14


@pytest.mark.parametrize("name", ["hand", "depth4"])
def test_gradient_against_central_differences(name):
    """Richardson's own estimate is the tolerance: |analytic - FD(h/2)| <= |FD(h) - FD(h/2)| +
    1e-12 * scale."""
    c = case(name)
    # every density at least 0.05, so that a step of 0.01 stays where sigma = max(stored, 0) is
    # smooth and is large enough for the differences' own float64 rounding (about 1e-16 / h of a
    # ray's D) to stay below the 1e-12 term
    sigma = c.sigma.astype(np.float64) + 0.05
    analytic = dref.distortion(c.w, c.scale, c.starts, c.dirs, sigma)["grad"]

    def fd(leaf, h):
        up, down = sigma.copy(), sigma.copy()
        up[leaf] += h
        down[leaf] -= h
        # per ray first: the rays that do not take the leaf cancel exactly
        return (dref.ray_distortion(c.w, c.starts, c.dirs, up)
                - dref.ray_distortion(c.w, c.starts, c.dirs, down)).sum() / (2.0 * h)

    magnitude = max(1.0, float(np.abs(analytic).max()))
    worst = 0.0
    for leaf in range(len(sigma)):
        h = 1e-2
        coarse, fine = fd(leaf, h), fd(leaf, 0.5 * h)
        allowed = abs(coarse - fine) + 1e-12 * magnitude
        worst = max(worst, abs(analytic[leaf] - fine) / allowed)
        assert abs(analytic[leaf] - fine) <= allowed, (leaf, analytic[leaf], coarse, fine)
    print("%s: worst |analytic - FD(h/2)| / (|FD(h) - FD(h/2)| + 1e-12 scale) = %.3f" % (name, worst))


@pytest.mark.parametrize("name", CASES + ["depth4"])
def test_weighted_sum_of_g_is_twice_d(name):
    c = case(name)
    for t_min in T_MINS:
        full = dref.distortion(c.w, c.scale, c.starts, c.dirs, c.sigma, t_min)
        assert (full["dist"] >= 0).all()
        # float64 rounding of sums whose terms are at most the ray's reach (W <= 1): the
        # differences M_tot - M_{k+1} and m_k (W_tot - W_{k+1}) cancel at that magnitude
        assert (np.abs(full["wg"] - 2.0 * full["dist"]) <= 64 * 2.0 ** -52 * full["reach"] *
                np.maximum(full["count"], 1)).all()


@pytest.mark.parametrize("name", CASES + ["depth4"])
def test_the_budget_discriminates(name):
    """A gradient without the (2/3) w_k L_k term, and one without the sum over j > k, is further
    than the budget from the contract's on at least one leaf of every case the GPU tests use."""
    c = case(name)
    for t_min in T_MINS:
        for min_t in MIN_TS:
            full = dref.distortion(c.w, c.scale, c.starts, c.dirs, c.sigma, t_min, min_t,
                                   keep=c.ok)
            assert np.isfinite(full["budget_g"]).all() and np.isfinite(full["budget_d"]).all()
            for variant in ("no_self", "no_tail"):
                wrong = dref.distortion(c.w, c.scale, c.starts, c.dirs, c.sigma, t_min, min_t,
                                        variant=variant, keep=c.ok)
                apart = np.abs(wrong["grad"] - full["grad"]) > full["budget_g"]
                print("%s t_min=%.2f min_T=%g, %s: %d of %d leaves are further than the budget"
                      % (name, t_min, min_t, variant, apart.sum(), len(apart)))
                assert apart.any()


def test_negative_and_nan_densities_pass_as_zero():
    c = case("hand")
    for stored in (-1.0, np.nan):
        sigma = c.sigma.astype(np.float64).copy()
        sigma[1] = stored
        zero = sigma.copy()
        zero[1] = 0.0
        got = dref.distortion(c.w, c.scale, c.starts, c.dirs, sigma)
        want = dref.distortion(c.w, c.scale, c.starts, c.dirs, zero)
        assert np.array_equal(got["dist"], want["dist"]) and np.isfinite(got["grad"]).all()
        assert got["grad"][1] == 0.0 and got["budget_g"][1] == 0.0 and want["grad"][1] != 0.0
        assert np.array_equal(got["grad"][[0, 2]], want["grad"][[0, 2]])


# ------------------------------------------------------------------ the package, without a device
def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


NAMES = {"ffn_octree_distortion", "ffn_octree_render_volume_backward_dist",
         "ffn_octree_render_volume_sh_backward_dist", "ffn_octree_grad_dist_workspace_bytes"}


def test_symbols_are_declared_and_exported():
    _lib, lib = library()
    assert NAMES <= set(_lib.declared_symbols())
    for name in NAMES:
        assert getattr(lib, name)
    from fourier_feature_nets_amd import ops
    assert callable(ops.octree_distortion)


def test_bad_arguments_are_refused_by_name_without_a_device():
    _, lib = library()
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    lib.ffn_octree_grad_dist_workspace_bytes.restype = ctypes.c_int64
    lib.ffn_octree_grad_workspace_bytes.restype = ctypes.c_int64
    lib.ffn_octree_grad_sh_workspace_bytes.restype = ctypes.c_int64
    f, i64 = ctypes.c_float, ctypes.c_int64
    host = (ctypes.c_float * 64)()
    base = ctypes.addressof(host)
    base += (-base) % 16
    good, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def forward(n=4, t_min=0.0, stride=4, offset=3, min_t=0.0, rays=good, rows=good, out=good):
        status = lib.ffn_octree_distortion(rays, rays, i64(n), f(1.0), 3, None, i64(0), rays,
                                           i64(1), f(t_min), rows, stride, offset, f(min_t), out,
                                           None)
        return status, lib.ffn_last_error_string().decode()

    for kwargs, why in (({"stride": 0}, "sigma_offset"), ({"offset": 4}, "sigma_offset"),
                        ({"offset": -1}, "sigma_offset"), ({"t_min": float("nan")}, "t_min"),
                        ({"min_t": 1.0}, "min_transmittance"), ({"rows": None}, "null argument"),
                        ({"out": None}, "null argument"), ({"rays": None}, "null argument"),
                        ({"n": 0}, "shape")):
        status, text = forward(**kwargs)
        assert status != 0 and "ffn_octree_distortion" in text and why in text, (kwargs, text)

    def backward(dist_scale=1.0, n=4, channels=4, own=good, rays=good, data=None, bytes_=0,
                 entries=16, ray_distortion=None):
        status = lib.ffn_octree_render_volume_backward_dist(
            rays, rays, i64(n), f(1.0), 3, None, i64(0), rays, i64(1), f(0.0),
            own if data is None else data, channels, f(0), f(0), f(0), f(0.0), own, own, own,
            i64(bytes_), i64(entries), own, None, f(dist_scale), ray_distortion, None)
        return status, lib.ffn_last_error_string().decode()

    def backward_sh(dist_scale=1.0, own=good, rays=good, stride=16, degree=1):
        status = lib.ffn_octree_render_volume_sh_backward_dist(
            rays, rays, i64(4), f(1.0), 3, None, i64(0), rays, i64(1), f(0.0), own, f(0), f(0),
            f(0), f(0.0), own, own, own, i64(0), i64(16), own, None, degree, stride,
            f(dist_scale), None, None)
        return status, lib.ffn_last_error_string().decode()

    for call, who in ((backward, "ffn_octree_render_volume_backward_dist"),
                      (backward_sh, "ffn_octree_render_volume_sh_backward_dist")):
        for bad in (-1.0, float("nan"), float("inf"), -float("inf")):
            status, text = call(dist_scale=bad)
            assert status != 0 and who in text and "dist_scale" in text, (bad, text)
        status, text = call(own=None)
        assert status != 0 and who in text and "null argument" in text, text
        # the per-ray triples lie behind the parent's layout: its size alone is too small
        status, text = call()
        assert status != 0 and who in text and "workspace too small" in text, text
    status, text = backward(data=odd)
    assert status != 0 and "16-byte aligned" in text, text
    status, text = backward(channels=3)
    assert status != 0 and "channels" in text, text
    status, text = backward_sh(stride=14)
    assert status != 0 and "row_stride" in text, text
    status, text = backward_sh(degree=3)
    assert status != 0 and "degree" in text, text
    # sizing: the parent's bytes and three floats per ray, rounded up to 256
    for n, leaves, entries in ((64, 3, 1024), (20000, 7253, 1 << 20)):
        extra = (12 * n + 255) // 256 * 256
        plain = lib.ffn_octree_grad_workspace_bytes(i64(n), i64(leaves), i64(entries))
        assert lib.ffn_octree_grad_dist_workspace_bytes(i64(n), i64(leaves), i64(entries), 0) \
            == plain + extra
        for degree in (1, 2):
            sh = lib.ffn_octree_grad_sh_workspace_bytes(i64(n), i64(leaves), i64(entries), degree)
            assert lib.ffn_octree_grad_dist_workspace_bytes(i64(n), i64(leaves), i64(entries),
                                                            degree) == sh + extra
    for args in ((i64(0), i64(1), i64(1), 0), (i64(1), i64(1), i64(1), 3), (i64(1), i64(1), i64(1), -1)):
        assert lib.ffn_octree_grad_dist_workspace_bytes(*args) == -1
        assert "ffn_octree_grad_dist_workspace_bytes" in lib.ffn_last_error_string().decode()


def small_tree(sh_degree=None):
    import fourier_feature_nets as ffn
    c = case("hand")
    if sh_degree is None:
        return ffn.OcTree(c.scale, c.nodes, c.leaves, c.data)
    channels = 3 * (sh_degree + 1) ** 2 + 1
    data = np.zeros((len(c.leaves), channels), np.float32)
    data[:, -1] = c.sigma
    return ffn.OcTree(c.scale, c.nodes, c.leaves, data, sh_degree)


@pytest.mark.parametrize("bad", [-1e-3, float("nan"), float("inf"), "much", None, True])
def test_dist_weight_is_refused_by_name(bad):
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    for fit, tree in ((ffn.fit_octree, small_tree()), (ffn.fit_octree_sh, small_tree(1))):
        with pytest.raises(ValueError, match="dist_weight"):
            fit(tree, None, None, center=(0, 0, 0), dist_weight=bad)
        with pytest.raises(ValueError, match="dist_weight"):
            ffn.fit_octree_adaptive(tree, None, None, rounds=0, center=(0, 0, 0), dist_weight=bad)
    rays = torch.zeros((2, 3))
    index = torch.zeros((1,), dtype=torch.int64)
    with pytest.raises(ValueError, match="dist_scale"):
        ops.octree_render_volume_backward(rays, rays, 1.0, 1, index[:0], index, torch.zeros((1, 4)),
                                          rays, rays[:, 0], dist_scale=bad)
    with pytest.raises(ValueError, match="dist_scale"):
        ops.octree_render_volume_sh_backward(rays, rays, 1.0, 1, index[:0], index,
                                             torch.zeros((1, 16)), 1, rays, rays[:, 0],
                                             dist_scale=bad)


class _StubOps:
    """Records what a field's ``backward`` calls."""

    def __init__(self):
        self.calls = []

    def octree_render_volume_backward(self, *args, **kwargs):
        self.calls.append(("plain", len(args), dict(kwargs)))
        return "plain"

    def octree_render_volume_sh_backward(self, *args, **kwargs):
        self.calls.append(("sh", len(args), dict(kwargs)))
        return "sh"


def test_dist_weight_zero_dispatches_to_the_old_ops(monkeypatch):
    from fourier_feature_nets_amd import octree_fit
    stub = _StubOps()
    monkeypatch.setattr(octree_fit, "ops", stub)
    field = types.SimpleNamespace(_geometry=lambda: (1.0, 1, None, None), data=torch.zeros((1, 4)),
                                  workspace=None, sh_degree=1)
    rays = torch.zeros((2, 3))
    for method, kind, positional in ((octree_fit.OctreeField.backward, "plain", 14),
                                     (octree_fit.OctreeSHField.backward, "sh", 15)):
        stub.calls.clear()
        # off: the call of before the term existed -- positional arguments only, no keyword
        assert method(field, rays, rays, rays, rays[:, 0]) == kind
        assert method(field, rays, rays, rays, rays[:, 0], dist_scale=0.0, ray_distortion=None) == kind
        assert stub.calls == [(kind, positional, {}), (kind, positional, {})]
        stub.calls.clear()
        out = torch.zeros((2,))
        method(field, rays, rays, rays, rays[:, 0], dist_scale=0.25)
        method(field, rays, rays, rays, rays[:, 0], ray_distortion=out)
        assert [c[0] for c in stub.calls] == [kind, kind]
        assert stub.calls[0][2] == {"dist_scale": 0.25, "ray_distortion": None}
        assert stub.calls[1][2]["dist_scale"] == 0.0 and stub.calls[1][2]["ray_distortion"] is out


def test_ops_dispatch_by_entry_name(monkeypatch):
    """``ops``: with ``dist_scale == 0`` and no ``ray_distortion`` the entry point without the term
    is named; otherwise the ``_dist`` one, with the two arguments behind the parent's."""
    from fourier_feature_nets_amd import ops
    seen = []

    def fake_backward(name, *args, **kwargs):
        seen.append((name, kwargs.get("dist")))
        return None

    monkeypatch.setattr(ops, "_render_volume_backward", fake_backward)
    rays = torch.zeros((2, 3))
    index = torch.zeros((1,), dtype=torch.int64)
    plain = (rays, rays, 1.0, 1, index[:0], index, torch.zeros((1, 4)), rays, rays[:, 0])
    sh = (rays, rays, 1.0, 1, index[:0], index, torch.zeros((1, 16)), 1, rays, rays[:, 0])
    out = torch.zeros((2,))
    ops.octree_render_volume_backward(*plain)
    ops.octree_render_volume_backward(*plain, dist_scale=0.0)
    ops.octree_render_volume_backward(*plain, dist_scale=0.5)
    ops.octree_render_volume_backward(*plain, ray_distortion=out)
    ops.octree_render_volume_sh_backward(*sh)
    ops.octree_render_volume_sh_backward(*sh, dist_scale=2.0, ray_distortion=out)
    assert seen == [("ffn_octree_render_volume_backward", None),
                    ("ffn_octree_render_volume_backward", None),
                    ("ffn_octree_render_volume_backward", (0.5, None)),
                    ("ffn_octree_render_volume_backward", (0.0, out)),
                    ("ffn_octree_render_volume_sh_backward", None),
                    ("ffn_octree_render_volume_sh_backward", (2.0, out))]
