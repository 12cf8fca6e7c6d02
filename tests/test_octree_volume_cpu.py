"""Host side of the K15 volume render: the float64 restatement (tests/octree_volume_reference.py)
against answers written out by hand and against an independent dense march, the C ABI's argument
checks, and what ``OcTree.render_volume`` / ``render_image(mode=...)`` / ``bake`` and the two
programs refuse or default to without a GPU."""

import ctypes
import os
import sys

import numpy as np
import pytest

from tests import octree_reference as oref
from tests import octree_volume_reference as vref
from tests import octree_walk_reference as wref
from tests.octree_render_helpers import golden_rays
from tests.octree_volume_helpers import hand_case, random_leaf_data, tie_density
from tests.octree_walk_helpers import two_level_tree

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
BG = (0.1, 0.2, 0.3)


def test_known_answers_on_a_hand_built_tree():
    """The expected values are spelled out from ``exp``; the chords are those of
    ``hand_case.__doc__``."""
    scale, nodes, leaves, data, starts, dirs = hand_case()
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    bg = np.float32(BG).astype(np.float64)
    rgb = data[:, :3].astype(np.float64)
    v = vref.composite(w, scale, starts, dirs, data, 0.0, BG)
    assert list(v["count"]) == [1, 1, 0, 3, 1]
    # ray 0: leaf 0, sigma 2 over a world length of (1 - 0.5) * |(2,0,0)| = 1
    a0 = 1 - np.exp(-2.0)
    assert np.allclose(v["color"][0], a0 * rgb[0] + (1 - a0) * bg, rtol=0, atol=1e-15)
    assert np.isclose(v["alpha"][0], a0, rtol=0, atol=1e-15) and v["depth"][0] == 0.5
    # ray 1: leaf 1, sigma 3 over 0.5
    a1 = 1 - np.exp(-1.5)
    assert np.allclose(v["color"][1], a1 * rgb[1] + (1 - a1) * bg, rtol=0, atol=1e-15)
    assert np.isclose(v["alpha"][1], a1, rtol=0, atol=1e-15) and v["depth"][1] == 3.0
    # ray 2: empty space only
    assert np.array_equal(v["color"][2], bg) and v["alpha"][2] == 0 and v["depth"][2] == 0
    assert v["gap"][2] == 0 and v["best"][2] == -1
    # ray 3: the diagonal, |d| = sqrt 3: leaf 0 over t 1 .. 2, leaf 1 over 2 .. 2.5, leaf 2 opaque
    root3 = np.sqrt(3.0)
    b0 = 1 - np.exp(-2.0 * root3)
    b1 = 1 - np.exp(-3.0 * 0.5 * root3)
    w0, w1, w2 = b0, (1 - b0) * b1, (1 - b0) * (1 - b1) * 1.0
    assert np.allclose(v["color"][3], w0 * rgb[0] + w1 * rgb[1] + w2 * rgb[2], rtol=0, atol=1e-15)
    assert v["alpha"][3] == 1.0 and v["trans"][3] == 0.0 and v["depth"][3] == 1.0
    assert np.isclose(v["gap"][3], w0 - w1, rtol=0, atol=1e-15)
    # ray 4: the opaque leaf alone
    assert np.array_equal(v["color"][4], rgb[2]) and v["alpha"][4] == 1 and v["depth"][4] == 2.0

    # t_min = 0.75 cuts leaf 0 on ray 0: world length (1 - 0.75) * 2 = 0.5, depth = t_min
    cut = vref.composite(w, scale, starts, dirs, data, 0.75, BG)
    c0 = 1 - np.exp(-2.0 * 0.5)
    assert np.allclose(cut["color"][0], c0 * rgb[0] + (1 - c0) * bg, rtol=0, atol=1e-15)
    assert cut["depth"][0] == 0.75 and cut["clamped"][0] and not v["clamped"][0]
    # t_min = 1 is the leaf's exit: t_out > t_min fails, nothing is taken
    gone = vref.composite(w, scale, starts, dirs, data, 1.0, BG)
    assert gone["count"][0] == 0 and np.array_equal(gone["color"][0], bg)
    # on the diagonal t_min = 2.25 drops leaf 0 and halves leaf 1
    d1 = 1 - np.exp(-3.0 * 0.25 * root3)
    late = vref.composite(w, scale, starts, dirs, data, 2.25, BG)
    assert late["count"][3] == 2
    assert np.allclose(late["color"][3], d1 * rgb[1] + (1 - d1) * rgb[2], rtol=0, atol=1e-15)
    assert late["depth"][3] == (2.25 if d1 >= 1 - d1 else 2.5)

    # a tie: leaf 1 with an opacity of exactly one half, then the opaque leaf 2 -- the first wins
    tie = data.astype(np.float64)
    tie[0, 3] = 0.0
    tie[1, 3] = tie_density(0.5 * root3)
    t = vref.composite(w, scale, starts, dirs, tie, 0.0, BG)
    assert t["count"][3] == 3 and t["gap"][3] == 0.0 and t["alpha"][3] == 1.0
    at = np.nonzero(w["ray"][t["taken"]] == 3)[0]
    assert sorted(t["weights"][at]) == [0.0, 0.5, 0.5]
    assert t["depth"][3] == 2.0                         # leaf 1's entry, not leaf 2's 2.5
    assert np.allclose(t["color"][3], 0.5 * rgb[1] + 0.5 * rgb[2], rtol=0, atol=1e-15)

    # no density anywhere (zero, negative, NaN): the background
    for value in (0.0, -3.0, np.nan):
        empty = data.copy()
        empty[:, 3] = value
        e = vref.composite(w, scale, starts, dirs, empty, 0.0, BG)
        assert np.array_equal(e["color"], np.repeat(bg[None], len(starts), 0))
        assert (e["alpha"] == 0).all() and (e["depth"] == 0).all() and (e["best"] == -1).all()

    # early termination: on the diagonal T after leaf 0 is exp(-2 sqrt 3) = 0.031
    early = vref.composite(w, scale, starts, dirs, data, 0.0, BG, min_transmittance=0.05)
    assert early["count"][3] == 1 and np.isclose(early["trans"][3], 1 - b0)
    assert np.allclose(early["color"][3], b0 * rgb[0] + (1 - b0) * bg, rtol=0, atol=1e-15)
    # the budget: no density, no drift term
    assert v["budget_c"][2] == 8 * 2.0 ** -24 and v["budget_a"][2] == 8 * 2.0 ** -24


def test_the_restatement_equals_a_dense_march():
    """An independent route to the same integral: 20 000 midpoint steps along the chord of the
    cube, the leaf of every midpoint from ``octree_reference.query``.  A step that straddles a
    boundary is attributed to one side: per boundary at most one step of optical depth
    ``sigma_max * step * |d|`` goes astray, on each of colour (times cmax) and alpha."""
    with np.load(os.path.join(HERE, "golden", "octree.npz")) as g:
        scale, nodes, leaves = g["shell/scale"], g["shell/node_index"], g["shell/leaf_index"]
    starts, directions = golden_rays("shell")
    w = wref.walk(scale, nodes, leaves, starts, directions)
    rng = np.random.default_rng(21)
    data = random_leaf_data(scale, leaves)
    data[:, 3] = (rng.random(len(leaves)) * 4.0 / np.float64(scale)).astype(np.float32)
    crossings = np.bincount(w["ray"][w["leaf"] >= 0], minlength=len(starts))
    rows = np.nonzero(w["hit"] & (crossings >= 2))[0][:64]
    assert len(rows) == 64
    t_min = 0.25
    v = vref.composite(w, scale, starts, directions, data, t_min, BG)
    steps = 20000
    bg = np.float32(BG).astype(np.float64)
    sigma64, rgb = data[:, 3].astype(np.float64), data[:, :3].astype(np.float64)
    cmax = float(rgb.max())
    worst = 0.0
    for r in rows:
        o, d = starts[r].astype(np.float64), directions[r].astype(np.float64)
        lo, hi = max(w["root_in"][r], t_min), w["root_out"][r]
        step = (hi - lo) / steps
        mid = lo + (np.arange(steps) + 0.5) * step
        slot = oref.query(scale, nodes, leaves, (o[None, :] + mid[:, None] * d[None, :]))
        sigma = np.where(slot >= 0, sigma64[np.maximum(slot, 0)], 0.0)
        tau = sigma * step * np.linalg.norm(d)
        trans = np.exp(-np.concatenate([[0.0], np.cumsum(tau)]))
        weight = trans[:-1] - trans[1:]                        # T_i (1 - exp(-tau_i))
        color = (weight[:, None] * rgb[np.maximum(slot, 0)]).sum(0) + trans[-1] * bg
        allowed = 2 * (crossings[r] + 1) * sigma64.max() * step * np.linalg.norm(d) * max(1.0, cmax)
        err = max(np.abs(color - v["color"][r]).max(), abs((1 - trans[-1]) - v["alpha"][r]))
        worst = max(worst, err / allowed)
        assert err <= allowed, (r, err, allowed)
    print("dense march: worst error / allowed %.3f over %d rays, alpha %.3f .. %.3f" %
          (worst, len(rows), v["alpha"][rows].min(), v["alpha"][rows].max()))
    assert v["alpha"][rows].min() < 0.5 < v["alpha"][rows].max()


def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_volume_symbols_are_declared_and_exported():
    _lib, lib = library()
    assert {"ffn_octree_render_volume", "ffn_octree_bake"} <= set(_lib.declared_symbols())
    assert lib.ffn_octree_render_volume and lib.ffn_octree_bake
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "K15" in header and "min_transmittance" in header and "softplus" in header


def test_bad_arguments_return_nonzero_without_a_device():
    """Nothing can be launched: a scalar is out of range, or a pointer is null, in every call.
    Which check refused is read from the library's error string.  The shape checks come after the
    null checks of the entry's own pointers, so those get a host buffer nobody reads."""
    _, lib = library()
    lib.ffn_octree_render_volume.restype = ctypes.c_int
    lib.ffn_octree_bake.restype = ctypes.c_int
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    f, i64 = ctypes.c_float, ctypes.c_int64
    host = (ctypes.c_float * 16)()

    def volume(n=4, depth=3, t_min=0.0, channels=4, min_t=0.0, own=None):
        status = lib.ffn_octree_render_volume(None, None, i64(n), f(1.0), depth, None, i64(0),
                                              None, i64(1), f(t_min), own, channels, f(0), f(0),
                                              f(0), f(min_t), own, own, own, None)
        return status, lib.ffn_last_error_string().decode()

    for kwargs, why in (({}, "null argument"), ({"own": host}, "null argument"),
                        ({"n": 0, "own": host}, "shape"), ({"depth": 30, "own": host}, "shape"),
                        ({"depth": 0, "own": host}, "shape"),
                        ({"t_min": float("nan")}, "t_min"), ({"channels": 3}, "channels"),
                        ({"channels": 0}, "channels"), ({"min_t": 1.0}, "min_transmittance"),
                        ({"min_t": -0.5}, "min_transmittance"),
                        ({"min_t": float("nan")}, "min_transmittance"),
                        # scalars first: which check refuses does not depend on the pointers
                        ({"channels": 3, "t_min": float("nan"), "min_t": 2.0}, "channels"),
                        ({"t_min": float("nan"), "min_t": 2.0, "own": host}, "t_min")):
        status, text = volume(**kwargs)
        assert status != 0 and "ffn_octree_render_volume" in text and why in text, (kwargs, text)
    for args, why in (((None, i64(4), None, None), "null argument"),
                      ((host, i64(0), host, None), "shape"),
                      ((host, i64(1 << 31), host, None), "shape")):
        status = lib.ffn_octree_bake(*args)
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and "ffn_octree_bake" in text and why in text, text


def test_volume_refuses_what_it_cannot_render_before_any_device():
    import fourier_feature_nets as ffn
    scale, nodes, leaves = two_level_tree()
    rays = np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32)
    bare = ffn.OcTree(float(scale), nodes, leaves)
    three = ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 3), np.float32))
    flat = ffn.OcTree(float(scale), nodes, leaves, np.zeros(12, np.float32))
    full = ffn.OcTree(float(scale), nodes, leaves, np.zeros((3, 4), np.float32))
    for tree in (bare, three, flat):
        with pytest.raises(ValueError, match="leaf_data"):
            tree.render_volume(*rays)
        with pytest.raises(ValueError, match="leaf_data"):
            tree.render_image(None, 0, center=(0, 0, 0), mode="volume")
    for value in (1.0, -0.1, 2.0, float("nan")):
        with pytest.raises(ValueError, match="min_transmittance"):
            full.render_volume(*rays, min_transmittance=value)
        with pytest.raises(ValueError, match="min_transmittance"):
            full.render_image(None, 0, center=(0, 0, 0), mode="volume", min_transmittance=value)
    with pytest.raises(ValueError, match="shading"):
        full.render_image(None, 0, center=(0, 0, 0), mode="volume", shading="faces")
    with pytest.raises(ValueError, match="mode"):
        full.render_image(None, 0, center=(0, 0, 0), mode="splat")
    with pytest.raises(ValueError, match="cent"):
        full.render_image(None, 0, mode="volume")
    # a loaded tree does not know its centre: nothing of the model is touched
    assert full.center is None
    with pytest.raises(ValueError, match="cent"):
        full.bake(None)
    with pytest.raises(ValueError, match="cent"):
        ffn.OcTree.load(full.state_dict).bake(None, view=(1, 0, 0), batch_size=8)


def test_program_parser_defaults():
    sys.path.insert(0, ROOT)
    from scripts import bake_octree, render_octree
    parser = bake_octree.build_parser()
    args = parser.parse_args(["tree.npz", "model.pt", "out.npz"])
    assert (args.tree_path, args.model_path, args.output_path) == ("tree.npz", "model.pt", "out.npz")
    assert args.center == [0.0, 0.0, 0.0] and args.view == [0.0, 0.0, 1.0]
    assert args.batch_size == 1 << 20 and args.device == "cuda"
    args = parser.parse_args(["t", "m", "o", "--center", "0.25", "-0.5", "-0.0001", "--view", "1",
                              "0", "0", "--batch-size", "300", "--device", "cuda:0"])
    assert args.center == [0.25, -0.5, -0.0001] and args.view == [1.0, 0.0, 0.0]
    assert args.batch_size == 300 and args.device == "cuda:0"
    with pytest.raises(SystemExit):
        parser.parse_args(["t", "m"])
    parser = render_octree.build_parser()
    args = parser.parse_args(["tree.npz", "data.npz", "out"])
    assert args.mode == "first-hit" and args.min_transmittance == 0.0
    assert args.shading == "flat" and args.split == "val" and args.num_cameras == 10
    args = parser.parse_args(["t", "d", "o", "--mode", "volume", "--min-transmittance", "1e-3"])
    assert args.mode == "volume" and args.min_transmittance == 1e-3
    with pytest.raises(SystemExit):
        parser.parse_args(["t", "d", "o", "--mode", "splat"])
