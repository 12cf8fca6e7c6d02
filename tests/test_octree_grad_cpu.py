"""K17 without a device: the float64 restatement of the gradient contract
(tests/octree_grad_reference.py) against torch's float64 autograd through a plain-torch restatement
of the volume composite and against central differences; the C ABI's declarations and argument
checks; the ``ValueError``s of ``OctreeField`` / ``fit_octree``."""

import ctypes
import os

import numpy as np
import pytest
import torch

from tests import octree_grad_reference as gref
from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref
from tests.octree_render_helpers import golden_rays, load_tree
from tests.octree_volume_helpers import hand_case, random_leaf_data
from tests.octree_walk_helpers import two_level_tree

BG = (0.25, 0.5, 0.125)


def torch_composite(w, directions, data, t_min, background, min_transmittance):
    """``octree_volume_reference.composite`` in plain torch float64, ray by ray; ``data`` (L,4) a
    float64 tensor that may require a gradient.  -> color (R,3), alpha (R,)."""
    norm = np.linalg.norm(np.asarray(directions, np.float32).astype(np.float64), axis=1)
    bg = torch.tensor(np.asarray(background, np.float32).astype(np.float64))
    colors, alphas = [], []
    for r in range(len(w["hit"])):
        trans = torch.ones((), dtype=torch.float64)
        color = torch.zeros(3, dtype=torch.float64)
        for c in range(w["offsets"][r], w["offsets"][r + 1]):
            leaf = int(w["leaf"][c])
            if leaf < 0 or not w["t_out"][c] > t_min:
                continue
            length = (w["t_out"][c] - max(w["t_in"][c], t_min)) * norm[r]
            stored = data[leaf, 3]
            sigma = stored if float(stored.detach()) >= 0 else torch.zeros((), dtype=torch.float64)
            a = 1.0 - torch.exp(-(sigma * length))
            color = color + trans * a * data[leaf, :3]
            trans = trans * (1.0 - a)
            if float(trans.detach()) <= min_transmittance:
                break
        colors.append(color + trans * bg)
        alphas.append(1.0 - trans)
    return torch.stack(colors), torch.stack(alphas)


def autograd_case(scale, nodes, leaves, data, starts, dirs, t_min, min_t, seed):
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    rng = np.random.default_rng(seed)
    d_color = rng.normal(size=(len(starts), 3))
    d_alpha = rng.normal(size=len(starts))
    g = gref.gradient(w, scale, starts, dirs, data, d_color, d_alpha, t_min, BG, min_t)
    leaf_values = torch.tensor(np.asarray(data, np.float64), requires_grad=True)
    color, alpha = torch_composite(w, dirs, leaf_values, t_min, BG, min_t)
    ((color * torch.tensor(d_color)).sum() + (alpha * torch.tensor(d_alpha)).sum()).backward()
    want = leaf_values.grad.numpy()
    top = np.abs(want).max()
    assert top > 0
    assert np.abs(g["grad"] - want).max() <= 1e-12 * top
    return w, g, d_color, d_alpha


def finite_hand_case():
    scale, nodes, leaves, data, starts, dirs = hand_case()
    data = data.copy()
    data[2, 3] = 1.5                     # the opaque leaf, finite for a gradient
    return scale, nodes, leaves, data, starts, dirs


@pytest.mark.parametrize("t_min, min_t", [(0.0, 0.0), (0.75, 0.0), (0.0, 0.3)])
def test_restatement_equals_autograd_on_the_hand_case(t_min, min_t):
    _, g, _, _ = autograd_case(*finite_hand_case(), t_min, min_t, 3)
    assert (g["taken"] > 0).all() and (g["budget"] > 0).all()


def test_restatement_equals_autograd_on_a_golden_tree():
    bare = load_tree("shell").state_dict
    starts, dirs = golden_rays("shell")
    starts, dirs = starts[:96], dirs[:96]
    data = random_leaf_data(bare["scale"], bare["leaf_index"])
    data[::7, 3] = -1.0                   # no gradient through a negative density
    _, g, _, _ = autograd_case(bare["scale"], bare["node_index"], bare["leaf_index"], data, starts,
                               dirs, 0.0, 1e-3, 4)
    assert (g["grad"][::7, 3] == 0).all() and (g["taken"] > 0).sum() > 10


def test_restatement_equals_central_differences():
    scale, nodes, leaves, data, starts, dirs = finite_hand_case()
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    rng = np.random.default_rng(5)
    d_color, d_alpha = rng.normal(size=(5, 3)), rng.normal(size=5)
    g = gref.gradient(w, scale, starts, dirs, data, d_color, d_alpha, 0.0, BG)

    def objective(values):
        v = vref.composite(w, scale, starts, dirs, values, 0.0, BG)
        return (v["color"] * d_color).sum() + (v["alpha"] * d_alpha).sum()

    base = data.astype(np.float64)
    step = 1e-6
    for leaf in range(3):
        for channel in range(4):
            up, down = base.copy(), base.copy()
            up[leaf, channel] += step
            down[leaf, channel] -= step
            slope = (objective(up) - objective(down)) / (2 * step)
            assert abs(slope - g["grad"][leaf, channel]) <= 1e-8 * max(1.0, abs(slope))


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


NAMES = {"ffn_octree_render_volume_backward", "ffn_octree_grad_workspace_bytes",
         "ffn_octree_project"}


def test_gradient_symbols_are_declared_and_exported():
    _lib, lib = library()
    assert NAMES <= set(_lib.declared_symbols())
    for name in NAMES:
        assert getattr(lib, name)
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "K17" in header and "d sigma_k" in header
    from fourier_feature_nets_amd import build, ops
    assert "octree_grad.hip" in build.SOURCES
    assert callable(ops.octree_render_volume_backward) and callable(ops.octree_project)


def test_bad_arguments_return_nonzero_without_a_device():
    _, lib = library()
    lib.ffn_octree_render_volume_backward.restype = ctypes.c_int
    lib.ffn_octree_project.restype = ctypes.c_int
    lib.ffn_octree_grad_workspace_bytes.restype = ctypes.c_int64
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    f, i64 = ctypes.c_float, ctypes.c_int64
    host = (ctypes.c_float * 64)()
    base = ctypes.addressof(host)
    base += (-base) % 16
    good, odd = ctypes.c_void_p(base), ctypes.c_void_p(base + 4)

    def backward(n=4, depth=3, t_min=0.0, channels=4, min_t=0.0, own=None, rays=None, data=None,
                 out=None, space=None, bytes_=0, entries=16):
        data = own if data is None else data
        out = own if out is None else out
        space = own if space is None else space
        status = lib.ffn_octree_render_volume_backward(
            rays, rays, i64(n), f(1.0), depth, None, i64(0), rays, i64(1), f(t_min), data,
            channels, f(0), f(0), f(0), f(min_t), own, own, space, i64(bytes_), i64(entries), out,
            None, None)
        return status, lib.ffn_last_error_string().decode()

    for kwargs, why in (({}, "null argument"), ({"own": good}, "null argument"),
                        ({"n": 0, "own": good, "rays": good}, "shape"),
                        ({"depth": 30, "own": good, "rays": good}, "shape"),
                        ({"t_min": float("nan")}, "t_min"), ({"channels": 3}, "channels"),
                        ({"min_t": 1.0}, "min_transmittance"),
                        ({"min_t": float("nan")}, "min_transmittance"),
                        ({"channels": 3, "t_min": float("nan"), "min_t": 2.0}, "channels"),
                        ({"own": good, "rays": good, "data": odd}, "16-byte aligned"),
                        ({"own": good, "rays": good, "out": odd}, "16-byte aligned"),
                        ({"own": good, "rays": good, "space": odd}, "16-byte aligned"),
                        ({"own": good, "rays": good, "n": 1 << 30, "depth": 11}, "split the rays"),
                        ({"own": good, "rays": good, "entries": -1}, "shape"),
                        ({"own": good, "rays": good}, "workspace too small")):
        status, text = backward(**kwargs)
        assert status != 0 and "ffn_octree_render_volume_backward" in text and why in text, \
            (kwargs, text)
    for args, why in (((None, i64(4), None), "null argument"), ((good, i64(0), None), "num_leaves"),
                      ((odd, i64(4), None), "16-byte aligned")):
        status = lib.ffn_octree_project(*args)
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and "ffn_octree_project" in text and why in text, text
    for args in ((i64(0), i64(1), i64(1)), (i64(1), i64(0), i64(1)), (i64(1), i64(1), i64(-1)),
                 (i64(1), i64(1), i64(1 << 31))):
        assert lib.ffn_octree_grad_workspace_bytes(*args) == -1
        assert "ffn_octree_grad_workspace_bytes" in lib.ffn_last_error_string().decode()
    small = lib.ffn_octree_grad_workspace_bytes(i64(64), i64(3), i64(1024))
    large = lib.ffn_octree_grad_workspace_bytes(i64(64), i64(3), i64(1 << 20))
    assert 0 < small < large and small % 256 == 0


def test_fitting_refuses_before_any_device():
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    assert ffn.OctreeField is not None and callable(ffn.fit_octree)
    for values in (None, np.zeros((3, 3), np.float32)):
        tree = ffn.OcTree(float(scale), nodes, leaves, values)
        with pytest.raises(ValueError, match="leaf_data"):
            ffn.OctreeField(tree)
        with pytest.raises(ValueError, match="leaf_data"):
            ffn.fit_octree(tree, None)
    baked = ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 4), np.float32))
    with pytest.raises(ValueError, match="cent"):
        ffn.fit_octree(baked, None)                      # a loaded tree has no centre
    with pytest.raises(ValueError, match="min_transmittance"):
        ffn.fit_octree(baked, None, center=(0, 0, 0), min_transmittance=1.0)
    with pytest.raises(ValueError, match="learning_rate"):
        ffn.fit_octree(baked, None, center=(0, 0, 0), learning_rate=0.0)
    with pytest.raises(ValueError, match="batch_size"):
        ffn.fit_octree(baked, None, center=(0, 0, 0), batch_size=0)
