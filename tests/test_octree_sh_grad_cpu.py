"""Host side of K19 (fitting SH leaves): the float64 restatement of the gradient contract
(tests/octree_sh_grad_reference.py) against torch autograd and central differences through a second,
independent float64 writing of the render, its reduction to K17's restatement on a band-0 tree, the
layout inverse, the C ABI's argument checks, the refusals of ``OctreeSHField`` / ``fit_octree_sh``
before any device work, and the inputs of tests/test_octree_sh_grad_gpu.py (the share of rays its
cases leave out, in the float64 walk)."""

import ctypes
import os

import numpy as np
import pytest
import torch

from tests import octree_grad_reference as gref
from tests import octree_sh_grad_reference as sgref
from tests import octree_sh_reference as shref
from tests.octree_render_helpers import LEFT_OUT_CAP
from tests.octree_sh_helpers import DEGREES, SIZES, TREES, case, prefix, sh_leaf_data
from tests.octree_walk_helpers import two_level_tree

BG = (0.25, 0.5, 0.125)
Y0 = 0.28209479177387814
RAYS = 48


def upstream(count, seed):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(count, 3)).astype(np.float32), rng.normal(size=count).astype(np.float32)


def render(w, leaf_data, degree, directions, d_color, d_alpha, t_min, background):
    """The render written once more, in torch float64 and ray by ray, differentiable with respect
    to ``leaf_data`` ((L, 3B+1) float64 tensor, file order) -> sum(d_color * C) + sum(d_alpha *
    alpha).  Without an early end (that is a discontinuity)."""
    bases = (degree + 1) ** 2
    d64 = np.asarray(directions, np.float32).astype(np.float64)
    norm = np.linalg.norm(d64, axis=1)
    y = torch.tensor(shref.basis(directions, degree))
    bg = torch.tensor(np.asarray(background, np.float32).astype(np.float64))
    g_c = torch.tensor(np.asarray(d_color, np.float64))
    g_a = torch.tensor(np.asarray(d_alpha, np.float64))
    out = leaf_data.sum() * 0.0
    for r in range(len(w["hit"])):
        lo, hi = int(w["offsets"][r]), int(w["offsets"][r + 1])
        trans = torch.ones((), dtype=torch.float64)
        color = torch.zeros(3, dtype=torch.float64)
        for c in range(lo, hi):
            leaf = int(w["leaf"][c])
            if leaf < 0 or not w["t_out"][c] > t_min:
                continue
            length = (w["t_out"][c] - max(w["t_in"][c], t_min)) * norm[r]
            sigma = torch.clamp(leaf_data[leaf, -1], min=0.0)
            a = 1.0 - torch.exp(-(sigma * length))
            z = (leaf_data[leaf, :3 * bases].reshape(3, bases) * y[r][None, :]).sum(1)
            color = color + trans * a * torch.sigmoid(z)
            trans = trans * (1.0 - a)
        color = color + trans * bg
        out = out + (g_c[r] * color).sum() + g_a[r] * (1.0 - trans)
    return out


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("name", sorted(TREES))
def test_restatement_against_autograd_and_central_differences(name, degree):
    scale, nodes, leaves, starts, directions, w, _ = case(name)
    starts, directions, w = starts[:RAYS], directions[:RAYS], prefix(w, RAYS)
    data = sh_leaf_data(scale, leaves, degree).astype(np.float64)
    d_color, d_alpha = upstream(RAYS, 3 + degree)
    for t_min in (0.0, float(np.float32(0.7))):
        g = sgref.gradient(w, scale, starts, directions, data, degree, d_color, d_alpha, t_min, BG)
        assert g["grad"].shape == data.shape and g["budget"].shape == data.shape
        assert (g["taken"] > 0).any() and (g["budget"][g["taken"] > 0, -1] > 0).all()
        x = torch.tensor(data, requires_grad=True)
        render(w, x, degree, directions, d_color, d_alpha, t_min, BG).backward()
        auto = x.grad.numpy()
        worst = np.abs(auto - g["grad"]).max()
        print("%s degree %d t_min %.2f: restatement against autograd, worst %.3g (largest "
              "gradient %.3g)" % (name, degree, t_min, worst, np.abs(auto).max()))
        assert worst <= 1e-10
        assert (g["grad"][g["taken"] == 0] == 0).all()
        # central differences along seeded directions of the whole parameter vector
        rng = np.random.default_rng(degree)
        for _ in range(3):
            v = rng.normal(size=data.shape)
            h = 1e-6
            with torch.no_grad():
                up = render(w, torch.tensor(data + h * v), degree, directions, d_color, d_alpha,
                            t_min, BG).item()
                down = render(w, torch.tensor(data - h * v), degree, directions, d_color, d_alpha,
                              t_min, BG).item()
            slope, want = (up - down) / (2 * h), (g["grad"] * v).sum()
            # the truncation error of the central difference is h^2 f''' / 6, its rounding
            # 2^-53 |f| / h: both below 1e-6 of the scale of the directional derivative
            assert abs(slope - want) <= 1e-6 * max(1.0, abs(want)), (slope, want)


@pytest.mark.parametrize("degree", DEGREES)
def test_band_zero_tree_reduces_to_k17(degree):
    scale, nodes, leaves, starts, directions, w, _ = case("mixed4")
    bases = (degree + 1) ** 2
    data = sh_leaf_data(scale, leaves, degree).astype(np.float64)
    for c in range(3):
        data[:, c * bases + 1:(c + 1) * bases] = 0.0
    plain = np.zeros((len(data), 4))
    for c in range(3):
        plain[:, c] = 1.0 / (1.0 + np.exp(-(data[:, c * bases] * Y0)))
    plain[:, 3] = data[:, -1]
    d_color, d_alpha = upstream(len(starts), 5)
    for t_min, min_t in ((0.0, 0.0), (float(np.float32(0.7)), 1e-3)):
        g = sgref.gradient(w, scale, starts, directions, data, degree, d_color, d_alpha, t_min, BG,
                           min_t)
        k = gref.gradient(w, scale, starts, directions, plain, d_color, d_alpha, t_min, BG, min_t)
        assert np.array_equal(g["taken"], k["taken"])
        assert np.allclose(g["grad"][:, -1], k["grad"][:, 3], rtol=1e-12, atol=1e-14)
        for c in range(3):
            want = Y0 * plain[:, c] * (1.0 - plain[:, c]) * k["grad"][:, c]
            assert np.allclose(g["grad"][:, c * bases], want, rtol=1e-12, atol=1e-14)
        # with cmax = 1 the K19 budget of the density is at least K17's (whose cmax is below 1)
        assert (g["budget"][:, -1] >= k["budget"][:, 3]).all()


def test_wrong_restatements_differ():
    scale, nodes, leaves, starts, directions, w, _ = case("mixed4")
    data = sh_leaf_data(scale, leaves, 2)
    d_color, d_alpha = upstream(len(starts), 6)
    right = sgref.gradient(w, scale, starts, directions, data, 2, d_color, d_alpha, 0.0, BG)
    for variant in ("flipped", "slope", "short"):
        wrong = sgref.gradient(w, scale, starts, directions, data, 2, d_color, d_alpha, 0.0, BG,
                               variant=variant)
        far = np.abs(wrong["grad"] - right["grad"]) > 2 * right["budget"]
        assert far.any(), variant
        if variant == "short":
            assert far[wrong["dropped"]].any() and not np.delete(far, wrong["dropped"], 0).any()


def test_layout_inverse():
    from fourier_feature_nets_amd import ops
    scale, nodes, leaves = two_level_tree()
    for degree, stride in ((1, 16), (2, 28)):
        data = sh_leaf_data(scale, leaves, degree)
        rows = ops.octree_sh_device_layout(data, degree)
        back = ops.octree_sh_file_layout(rows, degree)
        assert back.dtype == np.float32 and back.flags.c_contiguous
        assert np.array_equal(back.view(np.uint32), data.view(np.uint32))
        assert np.array_equal(ops.octree_sh_device_layout(back, degree), rows)
        wide = np.zeros((len(rows), stride + 4), np.float32)
        wide[:, :stride] = rows
        assert np.array_equal(ops.octree_sh_file_layout(wide, degree), data)
        for bad in (rows[:, :-1], rows[:, :4], rows[0]):
            with pytest.raises(ValueError, match="leaf_rows"):
                ops.octree_sh_file_layout(bad, degree)
    with pytest.raises(ValueError, match="degree"):
        ops.octree_sh_file_layout(rows, 3)


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_k19_symbols_and_bad_arguments_without_a_device():
    _lib, lib = library()
    names = {"ffn_octree_render_volume_sh_backward", "ffn_octree_grad_sh_workspace_bytes",
             "ffn_octree_project_sh"}
    assert names <= set(_lib.declared_symbols())
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "K19a" in header and "K19b" in header and "K19c" in header
    lib.ffn_octree_render_volume_sh_backward.restype = ctypes.c_int
    lib.ffn_octree_project_sh.restype = ctypes.c_int
    lib.ffn_octree_grad_sh_workspace_bytes.restype = ctypes.c_int64
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    f, i64 = ctypes.c_float, ctypes.c_int64
    host = (ctypes.c_float * 64)()                      # 16-byte aligned below
    base = ctypes.addressof(host)
    aligned = ctypes.c_void_p(base + (-base) % 16)
    odd = ctypes.c_void_p(aligned.value + 4)

    def backward(n=4, depth=3, t_min=0.0, min_t=0.0, own=None, rays=None, degree=2, stride=28,
                 rows=None, out=None, space=None, bytes_=1 << 20, entries=64):
        status = lib.ffn_octree_render_volume_sh_backward(
            rays, rays, i64(n), f(1.0), depth, None, i64(0), rays, i64(1), f(t_min),
            rows if rows is not None else own, f(0), f(0), f(0), f(min_t), own, own,
            space if space is not None else own, i64(bytes_), i64(entries),
            out if out is not None else own, None, degree, stride, None)
        return status, lib.ffn_last_error_string().decode()

    for kwargs, why in (({}, "null argument"), ({"own": aligned}, "null argument"),
                        ({"n": 0, "own": aligned}, "shape"),
                        ({"depth": 30, "own": aligned}, "shape"),
                        ({"degree": 0}, "degree"), ({"degree": 3}, "degree"),
                        ({"stride": 24}, "row_stride"), ({"stride": 30}, "row_stride"),
                        ({"degree": 1, "stride": 12}, "row_stride"), ({"stride": 68}, "row_stride"),
                        ({"t_min": float("nan")}, "t_min"), ({"min_t": 1.0}, "min_transmittance"),
                        ({"min_t": float("nan")}, "min_transmittance"),
                        ({"own": aligned, "rays": aligned, "rows": odd}, "16-byte aligned"),
                        ({"own": aligned, "rays": aligned, "out": odd}, "16-byte aligned"),
                        ({"own": aligned, "rays": aligned, "space": odd}, "16-byte aligned"),
                        # 2^21 rays through a tree of depth 11: 2^21 * 3073 entry offsets
                        ({"own": aligned, "rays": aligned, "n": 1 << 21, "depth": 11}, "split the rays"),
                        ({"own": aligned, "rays": aligned, "entries": -1}, "shape"),
                        ({"own": aligned, "rays": aligned, "bytes_": 1024}, "workspace too small")):
        status, text = backward(**kwargs)
        assert status != 0 and "ffn_octree_render_volume_sh_backward" in text and why in text, \
            (kwargs, text)
    entries = i64(7)
    lib.ffn_octree_render_volume_sh_backward(
        None, None, i64(4), f(1.0), 3, None, i64(0), None, i64(1), f(0), None, f(0), f(0), f(0),
        f(0), None, None, None, i64(0), i64(0), None, ctypes.byref(entries), 2, 28, None)
    assert entries.value == -1
    for args, why in (((None, i64(4), 28, 2, None), "null argument"),
                      ((aligned, i64(0), 28, 2, None), "num_leaves"),
                      ((aligned, i64(1 << 31), 28, 2, None), "num_leaves"),
                      ((odd, i64(4), 28, 2, None), "16-byte aligned"),
                      ((aligned, i64(4), 28, 3, None), "degree"),
                      ((aligned, i64(4), 28, 0, None), "degree"),
                      ((aligned, i64(4), 24, 2, None), "row_stride"),
                      ((aligned, i64(4), 18, 1, None), "row_stride"),
                      ((aligned, i64(4), 12, 1, None), "row_stride")):
        status = lib.ffn_octree_project_sh(*args)
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and "ffn_octree_project_sh" in text and why in text, (args, text)
    size = lib.ffn_octree_grad_sh_workspace_bytes
    for args, why in (((i64(0), i64(1), i64(1), 2), "shape"), ((i64(1), i64(0), i64(1), 2), "shape"),
                      ((i64(1), i64(1), i64(-1), 2), "shape"),
                      ((i64(1), i64(1), i64(1 << 31), 2), "shape"),
                      ((i64(1), i64(1), i64(1), 0), "degree"), ((i64(1), i64(1), i64(1), 3), "degree")):
        assert size(*args) == -1
        text = lib.ffn_last_error_string().decode()
        assert "ffn_octree_grad_sh_workspace_bytes" in text and why in text, (args, text)
    # the size is host arithmetic: affine in max_entries up to alignment, below 96 bytes an entry
    # at degree 2 (and at degree 1), and above what an entry alone needs (16 + 4 + 4 + 2 * (4 + 4))
    for degree in DEGREES:
        for n, leaves in ((1, 1), (4096, 1000), (4096, 1 << 20)):
            small, large = size(i64(n), i64(leaves), i64(1 << 16), degree), \
                size(i64(n), i64(leaves), i64((1 << 16) + (1 << 20)), degree)
            slope = (large - small) / float(1 << 20)
            print("degree %d, n %d, L %d: %.2f bytes per additional entry" % (degree, n, leaves, slope))
            assert 40.0 <= slope < 96.0
            assert size(i64(n), i64(leaves), i64(0), degree) > 0
    assert size(i64(4096), i64(1000), i64(1 << 20), 2) > size(i64(4096), i64(1000), i64(1 << 20), 1)


def test_field_and_fit_refuse_before_any_device():
    import fourier_feature_nets as ffn
    assert ffn.OctreeSHField is not None and ffn.fit_octree_sh is not None
    import fourier_feature_nets_amd as amd
    assert amd.OctreeSHField is ffn.OctreeSHField and amd.fit_octree_sh is ffn.fit_octree_sh
    scale, nodes, leaves = two_level_tree()
    data = sh_leaf_data(scale, leaves, 2)
    plain = ffn.OcTree(float(scale), nodes, leaves, data[:, :4].copy())
    bare = ffn.OcTree(float(scale), nodes, leaves)
    for tree in (plain, bare, None):
        with pytest.raises(ValueError, match="no SH leaves"):
            ffn.OctreeSHField(tree, center=(0, 0, 0))
        with pytest.raises(ValueError, match="no SH leaves"):
            ffn.fit_octree_sh(tree, None, center=(0, 0, 0))
    tree = ffn.OcTree(float(scale), nodes, leaves, data, sh_degree=2)
    with pytest.raises(ValueError, match="center"):
        ffn.OctreeSHField(tree, center=(0, 0))
    with pytest.raises(ValueError, match="cent"):
        ffn.fit_octree_sh(tree, None)                   # a tree made by hand knows no centre
    for kwargs in ({"batch_size": 0}, {"num_steps": -1}, {"report_interval": 0}):
        with pytest.raises(ValueError, match="fit_octree_sh: batch_size"):
            ffn.fit_octree_sh(tree, None, center=(0, 0, 0), **kwargs)
    for rate in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="fit_octree_sh: learning_rate"):
            ffn.fit_octree_sh(tree, None, center=(0, 0, 0), learning_rate=rate)
    for value in (1.0, -0.1, float("nan")):
        with pytest.raises(ValueError, match="min_transmittance"):
            ffn.fit_octree_sh(tree, None, center=(0, 0, 0), min_transmittance=value)
    # the refusal of the plain entries now names the new ones
    with pytest.raises(ValueError, match="fit_octree_sh"):
        ffn.fit_octree(tree, None, center=(0, 0, 0))
    # fit_octree's signature is fit_octree_sh's
    import inspect
    assert str(inspect.signature(ffn.fit_octree)) == str(inspect.signature(ffn.fit_octree_sh))


@pytest.mark.parametrize("name", ["eight", "mixed4"])
def test_the_gpu_cases_leave_out_few_rays(name):
    """What tests/test_octree_sh_grad_gpu.py relies on, decided in the float64 walk alone."""
    scale, nodes, leaves, starts, directions, w, ok = case(name)
    for n in SIZES:
        assert 1.0 - ok[:n].mean() <= LEFT_OUT_CAP, (n, 1.0 - ok[:n].mean())
    # and every taken leaf has a positive budget in every channel that gets a gradient
    for degree in DEGREES:
        data = sh_leaf_data(scale, leaves, degree)
        d_color, d_alpha = upstream(len(starts), 9)
        d_color[~ok] = 0
        d_alpha[~ok] = 0
        g = sgref.gradient(w, scale, starts, directions, data, degree, d_color, d_alpha, 0.0, BG)
        moved = g["grad"] != 0
        assert (g["budget"][moved] > 0).all() and moved[g["taken"] > 0].any()
        rel = g["budget"][moved] / np.abs(g["grad"][moved])
        print("%s degree %d: %d of %d leaves taken, longest list %d; budget / |gradient| median "
              "%.3g" % (name, degree, (g["taken"] > 0).sum(), len(data), g["taken"].max(),
                        np.median(rel)))
