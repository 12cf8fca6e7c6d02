"""Host side of the K13 ray walk: the float64 restatement (tests/octree_walk_reference.py) against
ray paths the reference itself returned (tests/golden/octree_walk.npz from
tests/golden/make_octree_walk.py), against answers worked out by hand, and what ``OcTree.walk`` /
``spans`` do without a GPU.

The reference advances by ``t += 1e-5`` nudges; on a ray that cuts a region in a chord of a few
nudges it may step over the region, so such GRAZING rays (restatement margin below 4e-5 in t) are
left out -- at most 10 % of a fixture, a cap, asserted.  On all other rays the leaf sequences are
EQUAL.  The reference's t is the plane crossing plus its nudges: ``reference - crossing`` lies
between minus the f32 rounding of the reference's own arithmetic and twice the largest excess the
generator saw on that fixture."""

import ctypes
import os

import numpy as np
import pytest

from tests import octree_walk_reference as wref
from tests.octree_walk_helpers import two_level_tree

HERE = os.path.dirname(os.path.abspath(__file__))
TREES = ["shell", "planes", "nodata"]


@pytest.fixture(scope="module")
def golden():
    out = {}
    for name in ("octree.npz", "octree_walk.npz"):
        with np.load(os.path.join(HERE, "golden", name)) as g:
            out[name] = {k: g[k] for k in g.files}
    return out


def case(golden, name):
    tree = {k: golden["octree.npz"][name + "/" + k] for k in ("scale", "node_index", "leaf_index")}
    rays = {k.split("/", 1)[1]: v for k, v in golden["octree_walk.npz"].items()
            if k.startswith(name + "/")}
    return tree, rays


def test_fixture_covers_the_cases(golden):
    g = golden["octree_walk.npz"]
    assert [str(n) for n in g["names"]] == TREES and list(g["lengths"]) == [64, 6]
    assert float(g["grazing"]) == 4e-5
    for name in TREES:
        tree, rays = case(golden, name)
        assert len(rays["starts"]) >= 1000 and (rays["directions"] != 0).all()
        inside = (np.abs(rays["starts"]) < tree["scale"]).all(1)
        norm = np.linalg.norm(rays["directions"], axis=1)
        assert inside.sum() >= 100 and (~inside).sum() >= 500
        assert (np.abs(norm - 1) > 0.05).sum() >= 100 and (np.abs(norm - 1) < 1e-3).sum() >= 100
        leaves = rays["leaves_64"]
        assert ((leaves >= 0).any(1)).sum() >= 100                 # rays that cross leaves
        w = wref.walk(tree["scale"], tree["node_index"], tree["leaf_index"], rays["starts"],
                      rays["directions"])
        assert (~w["hit"]).sum() >= 20                             # rays that miss the cube
        assert (np.diff(w["offsets"]) > 5).sum() >= 100            # paths that 6 truncates


@pytest.mark.parametrize("length", [64, 6])
@pytest.mark.parametrize("name", TREES)
def test_restatement_equals_the_reference_paths(golden, name, length):
    tree, rays = case(golden, name)
    w = wref.walk(tree["scale"], tree["node_index"], tree["leaf_index"], rays["starts"],
                  rays["directions"])
    grazing = w["margin"] < float(golden["octree_walk.npz"]["grazing"])
    print("%s: %d of %d rays grazing" % (name, grazing.sum(), len(grazing)))
    assert grazing.mean() <= 0.10
    t_stops, leaves, written = wref.path(w, length)
    ref_t, ref_leaves = rays["t_stops_%d" % length], rays["leaves_%d" % length]
    ok = ~grazing
    assert np.array_equal(leaves[ok], ref_leaves[ok])
    assert (written[ok] <= length - 1).all()
    # t: stops, then the fill (the cube's exit t; the reference stores it unnudged)
    column = np.arange(length)[None, :]
    live = (ok & w["hit"])[:, None] & (column < written[:, None])
    fill = (ok & w["hit"])[:, None] & (column >= written[:, None])
    diff = ref_t.astype(np.float64) - t_stops
    # the reference's own f32 arithmetic: a few roundings of its operands (|plane| + |o|) / |d|
    lo = np.abs(rays["starts"]).max(1) + float(tree["scale"])
    rounding = 8 * (np.spacing(np.float32(lo)) / np.abs(rays["directions"]).min(1)
                    + np.spacing(np.abs(ref_t).max(1).astype(np.float32)))[:, None]
    bound = 2 * float(rays["max_excess"])
    print("%s L=%d: excess in [%.3g, %.3g], allowed %.3g" % (name, length, diff[live].min(),
                                                              diff[live].max(), bound))
    assert (diff >= -rounding)[live].all()
    assert (diff <= bound)[live].all()
    assert (np.abs(diff) <= rounding)[fill].all()


def test_known_answers_on_a_hand_built_tree():
    scale, nodes, leaves = two_level_tree()
    ids, slot, centers, half = wref.regions(scale, nodes, leaves)
    assert len(ids) == 7 + 8 and sorted(slot[slot >= 0]) == [0, 1, 2]
    assert np.array_equal(np.sort((2 * half) ** 3), [0.125] * 8 + [1.0] * 7)
    # the main diagonal: leaf 1, then through shared corners into 65 and 72
    starts = np.float32([[-2, -2, -2], [-2, -0.5, -0.5], [0.25, 0.3, -3], [0.2, 0.3, 0.1]])
    dirs = np.float32([[1, 1, 1], [2, 0, 0], [0, 0, 1], [0, 0, -0.5]])
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    t, leaf, written = wref.path(w, 8)
    assert list(written) == [3, 2, 3, 3]
    assert list(leaf[0][:3]) == [0, 1, 2] and np.allclose(t[0][:3], [1, 2, 2.5])
    assert np.allclose(t[0][3:], 3.0) and (leaf[0][3:] == -1).all()
    # along x at y = z = -.5 (zero components inside their slabs): leaf 1, then the empty octant 5
    assert list(leaf[1][:2]) == [0, -1] and np.allclose(t[1][:2], [0.5, 1.0])
    assert np.allclose(t[1][2:], 1.5)
    # up the z axis at (.25, .3): the empty octant 7 (z < 0), leaf 65 (z in [0, .5]), the empty 66
    w3 = wref.walk(scale, nodes, leaves, starts[2:3], dirs[2:3])
    t3, leaf3, written3 = wref.path(w3, 8)
    assert list(leaf3[0][:3]) == [-1, 1, -1] and np.allclose(t3[0][:3], [2, 3, 3.5])
    assert written3[0] == 3 and np.allclose(t3[0][3:], 4.0)
    # a start inside, direction -z of length .5: the whole chord, negative t included
    w4 = wref.walk(scale, nodes, leaves, starts[3:4], dirs[3:4])
    t4, leaf4, _ = wref.path(w4, 8)
    assert list(leaf4[0][:3]) == [-1, 1, -1] and np.allclose(t4[0][:3], [-1.8, -0.8, 0.2])
    assert np.allclose(t4[0][3:], 2.2)
    # spans over the leaves after t_min = 0: ray 0 from 1 to 3 (the cube's far corner)
    t_in, t_out, hit = wref.spans(w, scale, 3, dirs, 0.0, 0.0)
    assert hit[0] and np.allclose([t_in[0], t_out[0]], [1.0, 3.0])
    assert hit[1] and np.allclose([t_in[1], t_out[1]], [0.5, 1.0])
    t_in1, t_out1, _ = wref.spans(w, scale, 3, dirs, 0.0, 1.0)
    side = 2.0 / 4
    assert np.allclose(t_in[:2] - t_in1[:2], side / np.linalg.norm(dirs[:2], axis=1))
    assert np.allclose(t_out1[:2] - t_out[:2], side / np.linalg.norm(dirs[:2], axis=1))


def test_truncation_and_fill():
    scale, nodes, leaves = two_level_tree()
    w = wref.walk(scale, nodes, leaves, np.float32([[-2, -2, -2]]), np.float32([[1, 1, 1]]))
    t, leaf, written = wref.path(w, 3)            # at most L - 1 = 2 stops
    assert written[0] == 2 and list(leaf[0]) == [0, 1, -1] and np.allclose(t[0], [1, 2, 3])
    t, leaf, written = wref.path(w, 2)
    assert written[0] == 1 and list(leaf[0]) == [0, -1] and np.allclose(t[0], [1, 3])


def test_zero_components_and_misses():
    scale, nodes, leaves = two_level_tree()
    starts = np.float32([[-2, 1.5, 0.2],      # zero y outside its slab: a miss
                         [-2, 1.0, 0.2],      # on the cube's own face: inside
                         [0.1, 0.1, 0.1],     # no direction at all: a miss
                         [3, 3, 3],           # pointing away, line through the cube: a hit at t < 0
                         [3, 0, 0]])          # passes by
    dirs = np.float32([[1, 0, 0], [1, 0, 0], [0, 0, 0], [1, 1, 1], [0, 1, 0]])
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    assert list(w["hit"]) == [False, True, False, True, False]
    t, leaf, written = wref.path(w, 4)
    assert (leaf[[0, 2, 4]] == -1).all() and list(written[[0, 2, 4]]) == [0, 0, 0]
    assert written[1] == 3 and np.allclose(t[1][:3], [1, 2, 2.5]) and (leaf[1] == -1).all()
    assert np.allclose(t[3][:3], [-4, -3, -2.5])
    nan = wref.walk(scale, nodes, leaves, np.float32([[np.nan, 0, 0], [0, 0, 0]]),
                    np.float32([[1, 0, 0], [np.nan, 1, 0]]))
    assert not nan["hit"].any()


def test_root_only_tree():
    w = wref.walk(np.float32(2.0), np.zeros(0, np.int64), np.array([0], np.int64),
                  np.float32([[-4, 0.5, 0.5], [0, 0, 0]]), np.float32([[1, 0, 0], [0, 0, 4]]))
    t, leaf, written = wref.path(w, 4)
    assert list(written) == [1, 1] and list(leaf[:, 0]) == [0, 0]
    assert np.allclose(t[0], [2, 6, 6, 6]) and np.allclose(t[1], [-0.5, 0.5, 0.5, 0.5])
    t_in, t_out, hit = wref.spans(w, 2.0, 1, np.float32([[1, 0, 0], [0, 0, 4]]), 0.0, 0.0)
    assert hit.all() and np.allclose(t_in, [2, 0]) and np.allclose(t_out, [6, 0.5])


def test_walk_and_spans_raise_without_a_gpu_and_intersect_stays_out():
    import torch
    import fourier_feature_nets as ffn
    from fourier_feature_nets.octree import Path
    assert Path._fields == ("t_stops", "leaves")
    scale, nodes, leaves = two_level_tree()
    tree = ffn.OcTree(float(scale), nodes, leaves)
    assert tree.center is None and sorted(tree.state_dict) == ["leaf_index", "node_index", "scale"]
    with pytest.raises(NotImplementedError, match="intersect"):
        tree.intersect(np.zeros((1, 3)), np.ones((1, 3)), 4)
    with pytest.raises(AssertionError):
        tree.walk(np.zeros((2, 3), np.float32), np.ones(3, np.float32), 4)
    with pytest.raises(AssertionError):
        tree.spans(np.zeros((2, 2), np.float32), np.ones((2, 2), np.float32))
    if torch.cuda.is_available():
        return          # with a GPU, tests/test_octree_walk_gpu.py covers walk and spans
    with pytest.raises((RuntimeError, AssertionError)):
        tree.walk(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32), 4)
    with pytest.raises((RuntimeError, AssertionError)):
        tree.spans(np.zeros((1, 3), np.float32), np.ones((1, 3), np.float32))
    with pytest.raises((RuntimeError, AssertionError)):
        tree.query(np.zeros((1, 3), np.float32))


def test_walk_symbols_are_declared_and_exported():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    assert {"ffn_octree_walk", "ffn_octree_spans"} <= set(_lib.declared_symbols())
    lib = ctypes.CDLL(_lib.LIB_PATH)
    lib.ffn_octree_walk.restype = ctypes.c_int
    lib.ffn_octree_spans.restype = ctypes.c_int
    # argument checks refuse before any launch: no GPU is touched
    assert lib.ffn_octree_walk(None, None, ctypes.c_int64(4), ctypes.c_float(1.0), 3, None,
                               ctypes.c_int64(0), None, ctypes.c_int64(1), 8, None, None, None) != 0
    assert lib.ffn_octree_spans(None, None, ctypes.c_int64(4), ctypes.c_float(1.0), 30, None,
                                ctypes.c_int64(0), None, ctypes.c_int64(1), ctypes.c_float(0),
                                ctypes.c_float(1), None, None, None, None) != 0
