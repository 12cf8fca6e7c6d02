"""K26 without a GPU: the float64 restatement (tests/octree_focus_reference.py) against hand-worked
answers, its numpy-f32 operation list ``focus32`` inside the budgets of the restatement on every
scene the GPU test uses (so the budgets are attainable, and no ray of a scene is undecided, before a
GPU sees them), and the new surface: the header declares the entry point, ``_lib`` binds it,
``ops.octree_focus_sample`` refuses CPU tensors, ``RaySampler.focus_on_octree`` exists."""

import numpy as np
import pytest
import torch

from tests import octree_focus_reference as fref
from tests.octree_focus_helpers import (MIN_MASS, SCENES, hand_rays, reference, scene, targets,
                                        uniform_samples)


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("n_focus", [1, 3, 128])
def test_focus32_meets_the_budgets_of_the_restatement(name, n_focus):
    s = scene(name)
    w, c = reference(name)
    assert not fref.undecided(c, MIN_MASS).any()
    with_mass = c["mass"] >= MIN_MASS
    # a scene has rays with mass and (but for the root-only tree seen from all around) rays without
    assert with_mass.sum() >= 4
    u = targets(len(s["near"]), n_focus, 100 + n_focus)
    t, mass = fref.focus32(w, s["directions"], s["near"], s["far"], s["rows"][:, 3], u, MIN_MASS)
    worst = fref.check(c, s["near"], s["far"], u, MIN_MASS, t, mass, name)
    print("%s n_focus=%d: %d rays, %d with mass; worst |F(t) - u M| / budget %.3f, largest budget "
          "%.3g" % (name, n_focus, len(u), with_mass.sum(), worst, c["budget"][with_mass].max()))
    # the merge is a sort of the two halves
    uni = uniform_samples(s["near"], s["far"], 5)
    merged, _ = fref.focus32(w, s["directions"], s["near"], s["far"], s["rows"][:, 3], u, MIN_MASS,
                             uni)
    assert merged.shape == (len(u), 5 + n_focus)
    keep = ~np.isnan(merged).any(1)
    assert (np.diff(merged[keep], axis=1) >= 0).all()


def test_the_check_refuses_wrong_samples():
    """The checker has teeth: samples moved into a gap, or along the CDF by more than the budget,
    fail it."""
    s = scene("hand")
    w, c = reference("hand")
    u = targets(len(s["near"]), 4, 5, ends=False)
    t, mass = fref.focus32(w, s["directions"], s["near"], s["far"], s["rows"][:, 3], u, MIN_MASS)
    fref.check(c, s["near"], s["far"], u, MIN_MASS, t, mass)
    moved = t.copy()
    moved[0] = np.float32(0.25)                     # before leaf 0 (t 0.5 .. 1): empty space
    with pytest.raises(AssertionError):
        fref.check(c, s["near"], s["far"], u, MIN_MASS, moved, mass)
    moved = t.copy()
    moved[0] = np.sort(np.float32(0.5) + np.float32(0.5) * (u[0] * np.float32(0.99)))
    with pytest.raises(AssertionError):
        fref.check(c, s["near"], s["far"], u, MIN_MASS, moved, mass)
    with pytest.raises(AssertionError):
        fref.check(c, s["near"], s["far"], u, MIN_MASS, t, mass * np.float32(1.001))


def test_known_answers_of_the_hand_case():
    s = scene("hand")
    w, c = reference("hand")
    _, _, _, _, _, names = hand_rays()
    ray = {n: i for i, n in enumerate(names)}
    # masses: one leaf of optical depth sigma * world length
    one = ray["+x through leaf 0, zero components inside their slabs"]
    assert c["mass"][one] == pytest.approx(1 - np.exp(-2.0), abs=1e-15)       # 0.5 of t, |d| = 2
    assert c["mass"][ray["near cuts the leaf"]] == pytest.approx(1 - np.exp(-1.0), abs=1e-15)
    assert c["mass"][ray["far inside the leaf"]] == pytest.approx(1 - np.exp(-1.5), abs=1e-15)
    assert c["mass"][ray["near and far inside one leaf"]] == pytest.approx(1 - np.exp(-0.5), abs=1e-15)
    for name in ("far before the first leaf", "a zero component outside its slab",
                 "misses the cube, valid near and far", "a NaN direction", "near beyond far",
                 "through two empty octants"):
        assert c["mass"][ray[name]] == 0 and c["count"][ray[name]] == 0, name
    # the diagonal: leaves at t 1 .. 2, 2 .. 2.5, 2.5 .. 3 with |d| = sqrt 3, the last one opaque
    diag = ray["the diagonal through all three leaves"]
    a0, a1 = 1 - np.exp(-2 * np.sqrt(3)), 1 - np.exp(-3 * 0.5 * np.sqrt(3))
    lo = c["first"][diag]
    assert c["count"][diag] == 3 and c["mass"][diag] == pytest.approx(1.0, abs=1e-15)
    assert np.allclose(c["weight"][lo:lo + 3], [a0, (1 - a0) * a1, (1 - a0) * (1 - a1)], atol=1e-15)
    assert (c["t0"][lo:lo + 3] == [1, 2, 2.5]).all() and (c["t1"][lo:lo + 3] == [2, 2.5, 3]).all()
    # the start inside the cube: leaf 0 from near = 0 (its entry lies behind the start)
    inside = ray["a start inside the cube"]
    lo = c["first"][inside]
    assert (c["t0"][lo:lo + 3] == [0, .5, 1]).all() and (c["t1"][lo:lo + 3] == [.5, 1, 1.5]).all()
    # F: flat before, linear inside, M behind
    assert fref.evaluate(c, one, [0.0, 0.5, 0.75, 1.0, 1.5]) == pytest.approx(
        np.array([0, 0, .5, 1, 1]) * c["mass"][one], abs=1e-15)

    # one leaf and dyadic targets: t = t0 + u (t1 - t0), and u == 1 lands on t1
    u = np.tile(np.float32([0, .25, .5, .75, 1]), (len(names), 1))
    t, mass = fref.focus32(w, s["directions"], s["near"], s["far"], s["rows"][:, 3], u, MIN_MASS)
    fref.check(c, s["near"], s["far"], u, MIN_MASS, t, mass)
    assert np.allclose(t[one], [.5, .625, .75, .875, 1], atol=2e-7) and t[one, -1] == 1
    assert np.allclose(t[ray["near cuts the leaf"]], [.75, .8125, .875, .9375, 1], atol=2e-7)
    assert np.allclose(t[ray["far inside the leaf"]], .5 + u[0] * .375, atol=2e-7)
    assert np.allclose(t[ray["near and far inside one leaf"]], .625 + u[0] * .125, atol=2e-7)
    # the opaque leaf: a = 1 exactly, so f = u and the answers are exact
    opaque = ray["-x through the opaque leaf"]
    assert mass[opaque] == 1 and (t[opaque] == np.float32([2, 2.125, 2.25, 2.375, 2.5])).all()
    # fall-backs, bit for bit: near + u (far - near); near itself without near < far
    assert (t[ray["far before the first leaf"]] == np.float32(.375) * u[0]).all()
    assert (t[ray["misses the cube, valid near and far"]] == np.float32(.5) + u[0] * np.float32(3.5)).all()
    assert (t[ray["a NaN direction"]] == u[0]).all()
    assert (t[ray["near beyond far"]] == 2).all()
    # the diagonal ends on the opaque leaf: u == 1 lands on its t1 = 3, nothing beyond
    assert t[diag, -1] == 3 and (t[diag] >= 1).all()


def test_header_declares_and_lib_binds_the_entry_point():
    from fourier_feature_nets_amd import _lib
    assert "ffn_octree_focus_sample" in _lib.declared_symbols()
    with open(_lib.HEADER_PATH) as f:
        header = f.read()
    assert "K26" in header and "int ffn_octree_focus_sample(" in header
    lib = _lib.load()
    assert lib.ffn_octree_focus_sample is not None


def test_bad_arguments_are_refused_by_name_without_a_device():
    """Every refusal comes before any launch, so it needs no GPU: host buffers stand in for the
    pointers that nobody gets to read."""
    import ctypes
    from fourier_feature_nets_amd import _lib
    from fourier_feature_nets_amd._lib import c_f, c_i, c_i64
    lib = _lib.load()
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    fn = lib.ffn_octree_focus_sample
    fn.restype = ctypes.c_int
    buf = (ctypes.c_float * 4096)()
    out = (ctypes.c_float * 4096)()
    ptr = ctypes.cast(buf, ctypes.c_void_p)
    out_ptr = ctypes.cast(out, ctypes.c_void_p)
    null = ctypes.c_void_p(0)
    good = dict(starts=ptr, directions=ptr, near_far=ptr, num_rays_total=c_i64(8), ray_index=ptr,
                num_rays=c_i(8), cx=c_f(0), cy=c_f(0), cz=c_f(0), scale=c_f(1), depth=c_i(3),
                node_index=ptr, num_nodes=c_i64(2), leaf_index=ptr, num_leaves=c_i64(3),
                leaf_rows=ptr, stride=c_i(4), sigma_offset=c_i(3), u=ptr, n_focus=c_i(4),
                t_uniform=ptr, uniform_stride=c_i(4), n_uniform=c_i(4), min_mass=c_f(1e-3),
                t_out=out_ptr, mass_out=null, stream=null)
    max_depth = lib.ffn_octree_max_depth()
    bad = [("n_focus", dict(n_focus=c_i(0))),
           ("t_uniform", dict(t_uniform=null)),
           ("alias", dict(t_out=ptr)),
           ("alias", dict(t_out=ctypes.c_void_p(ptr.value + 4 * 10))),     # inside t_uniform's rows
           ("sigma_offset", dict(sigma_offset=c_i(4))),
           ("sigma_offset", dict(sigma_offset=c_i(-1))),
           ("depth", dict(depth=c_i(0))),
           ("depth", dict(depth=c_i(max_depth + 1))),
           ("2^31", dict(num_rays=c_i(1 << 24), n_focus=c_i(128), n_uniform=c_i(0), t_uniform=null)),
           ("min_mass", dict(min_mass=c_f(float("nan")))),
           ("min_mass", dict(min_mass=c_f(-1e-3))),
           ("uniform_stride", dict(uniform_stride=c_i(3))),
           ("null", dict(u=null)),
           ("null", dict(t_out=null))]
    for word, change in bad:
        args = dict(good, **change)
        status = fn(*args.values())
        message = lib.ffn_last_error_string().decode()
        assert status != 0, (word, change)
        assert message.startswith("ffn_octree_focus_sample: ") and word in message, (word, message)
    assert not any(out), "a refused call wrote to t_out"


def test_op_refuses_cpu_tensors():
    from fourier_feature_nets_amd import ops
    s = scene("hand")
    n = len(s["near"])
    index = torch.arange(n, dtype=torch.int64)
    args = (torch.from_numpy(s["starts"]), torch.from_numpy(s["directions"]),
            torch.from_numpy(np.stack([s["near"], s["far"]])), index, s["center"], s["scale"],
            s["depth"], torch.from_numpy(s["node_index"]), torch.from_numpy(s["leaf_index"]),
            torch.from_numpy(s["rows"]), 4, 3, torch.zeros((n, 2)))
    with pytest.raises(RuntimeError, match="must live on the GPU"):
        ops.octree_focus_sample(*args)


def test_sampler_and_tree_have_the_new_surface():
    import inspect
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd.sampler import RaySampler
    sig = inspect.signature(RaySampler.focus_on_octree)
    assert list(sig.parameters) == ["self", "tree", "center", "min_mass"]
    assert sig.parameters["center"].default == (0, 0, 0)
    assert sig.parameters["min_mass"].default == 1e-3
    sig = inspect.signature(ffn.OcTree.focus_samples)
    assert list(sig.parameters) == ["self", "starts", "directions", "near_far", "ray_index", "u",
                                    "t_uniform", "center", "min_mass", "return_mass"]
    # a tree without a density column refuses by name, before any device is needed
    bare = ffn.OcTree(1.0, [0, 8], [1, 65, 72])
    with pytest.raises(ValueError, match="OcTree.focus_samples: the tree has no density column"):
        bare.focus_samples(None, None, None, None, None, center=(0, 0, 0))
    colors = ffn.OcTree(1.0, [0, 8], [1, 65, 72], np.zeros((3, 3), np.float32))
    with pytest.raises(ValueError, match="no density column"):
        colors.focus_samples(None, None, None, None, None, center=(0, 0, 0))


def test_cli_focus_tree_options():
    import os
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from scripts import _cli
    parser = _cli.build_parser("t", _cli.TRAIN_COMMON, _cli.SKIP_GRID, _cli.FOCUS_TREE)
    args = parser.parse_args(["data.npz", "out"])
    assert args.focus_tree is None and args.focus_tree_center is None
    assert args.focus_carve_depth == 0 and args.focus_min_mass == 1e-3
    assert _cli.check_focus_tree(args) is False and _cli.focus_tree(args) is None
    args = parser.parse_args(["data.npz", "out", "--focus-carve-depth", "8", "--focus-min-mass", "0.01"])
    assert _cli.check_focus_tree(args) is True and args.focus_min_mass == 0.01
    args = parser.parse_args(["data.npz", "out", "--focus-tree", "t.npz", "--focus-tree-center",
                              "0", "0.5", "1"])
    assert _cli.check_focus_tree(args) is True and args.focus_tree_center == [0.0, 0.5, 1.0]
    for argv, word in ((["--focus-tree", "t.npz", "--focus-carve-depth", "6"], "two sources of one tree"),
                       (["--focus-carve-depth", "6", "--opacity-model", "m.pt"], "--opacity-model"),
                       (["--focus-tree", "t.npz", "--focus-tree-center", "0", "0", "0",
                         "--opacity-model", "m.pt"], "--opacity-model"),
                       (["--focus-tree", "t.npz"], "--focus-tree-center")):
        with pytest.raises(SystemExit, match=word):
            _cli.check_focus_tree(parser.parse_args(["data.npz", "out"] + argv))
    # the tables the reference's flags live in are what they were
    assert not any(row[0].startswith("--focus-tree") for row in _cli.TRAIN_COMMON + _cli.ORBIT)
