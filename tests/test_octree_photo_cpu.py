"""Host side of K28, carving by photo-consistency: the integer policy ``photo_actions`` at its
boundary and against a float64 variance, the numpy restatement (tests/photo_reference.py) on the
scenes the GPU tests use (no undecided pair; the two-blob scene loses exactly its phantoms), what the
methods, the op and the C ABI refuse without a GPU, the programs' arguments, and the routing of
``build_from_silhouettes(photo_threshold=...)``."""

import ctypes
import inspect
import os
import sys

import numpy as np
import pytest
import torch

from tests import photo_helpers as ph
from tests import photo_reference as pref
from tests.carve_helpers import AXIS_EYES, Scene, rig
from tests.octree_lattice_helpers import grid_tree
from tests.visible_helpers import camera_arrays

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
F = np.float32
SYMBOL = "ffn_octree_visible_moments"
MAX_CAMERAS = 66051


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def rows_of(pixels):
    """moments (1,8) uint32 of one leaf seen by cameras holding ``pixels`` (n,3)."""
    p = np.asarray(pixels, np.int64).reshape(-1, 3)
    return np.array([[*p.sum(0), len(p), *(p ** 2).sum(0), 0]], np.uint32)


# ------------------------------------------------------------------------------- the policy
def test_photo_actions_is_exact_at_equality_and_one_above():
    """Two cameras that differ by d in every channel: n Q - S = 3 d^2, and limit n^2 = 4 limit.
    With threshold = 0.2, (255 threshold)^2 = 2601 exactly, limit = 7803: d = 102 gives
    3 * 10404 = 31212 = 4 * 7803, equality, which keeps; d = 103 is above."""
    from fourier_feature_nets import photo_actions
    from fourier_feature_nets_amd import ops
    assert pref.limit_of(0.2) == 7803
    at, above = rows_of([[10, 20, 30], [112, 122, 132]]), rows_of([[10, 20, 30], [113, 123, 133]])
    assert photo_actions(at, 0.2).tolist() == [ops.OCTREE_KEEP]
    assert photo_actions(above, 0.2).tolist() == [ops.OCTREE_DROP]
    # one unit of n Q - S above the limit, in one channel
    one = rows_of([[0, 0, 0], [0, 0, 2]])                    # n Q - S = 2 * 4 - 4 = 4
    assert photo_actions(one, 0.0).tolist() == [ops.OCTREE_DROP]          # limit 0
    assert pref.limit_of(1 / 255) == 3                                    # 4 > 3 * 4 fails
    assert photo_actions(one, 1 / 255).tolist() == [ops.OCTREE_KEEP]
    same = rows_of([[7, 8, 9]] * 5)
    assert photo_actions(same, 0.0).tolist() == [ops.OCTREE_KEEP]         # 0 > 0 fails
    out = photo_actions(np.concatenate([at, above, same]), 0.2)
    assert out.dtype == np.uint8 and out.shape == (3,)
    assert photo_actions(np.zeros((0, 8), np.uint32), 0.1).shape == (0,)


def test_photo_actions_honours_min_views():
    from fourier_feature_nets import photo_actions
    loud = rows_of([[0, 0, 0], [255, 255, 255], [0, 255, 0]])
    assert photo_actions(loud, 0.1).tolist() == [0]
    assert photo_actions(loud, 0.1, min_views=3).tolist() == [0]
    assert photo_actions(loud, 0.1, min_views=4).tolist() == [1]
    unseen = np.zeros((1, 8), np.uint32)
    single = rows_of([[200, 0, 90]])
    assert photo_actions(np.concatenate([unseen, single]), 0.0).tolist() == [1, 1]


def test_photo_actions_against_a_float64_variance_and_the_restatement():
    from fourier_feature_nets import photo_actions
    rng = np.random.default_rng(71)
    rows = []
    for _ in range(400):
        n = int(rng.integers(1, 40))
        spread = int(rng.integers(1, 128))
        base = rng.integers(0, 256 - spread, 3)
        rows.append(rows_of(base + rng.integers(0, spread + 1, (n, 3))))
    # and the corner of the bound: every camera of a full buffer on 255, and half of them on 0
    full = np.array([[255 * MAX_CAMERAS] * 3 + [MAX_CAMERAS] + [65025 * MAX_CAMERAS] * 3 + [0]],
                    np.uint32)
    half = np.array([[255 * 33025] * 3 + [MAX_CAMERAS] + [65025 * 33025] * 3 + [0]], np.uint32)
    moments = np.concatenate(rows + [full, half])
    variance = pref.variance(moments)
    for threshold in (0.0, 0.02, 0.1, 0.3, 1.0):
        got = photo_actions(moments, threshold)
        assert np.array_equal(got, pref.actions(moments, threshold))
        judged = moments[:, 3] >= 2
        # the integer limit is ceil(3 (255 t)^2): within 1 / (3 * 255^2) of t^2 in variance
        far = judged & (np.abs(variance - threshold ** 2) > 1e-4)
        assert far.sum() > 300
        assert np.array_equal(got[far] == 0, variance[far] > threshold ** 2)
        assert (got[~judged] == 1).all()
    assert photo_actions(moments, 0.1)[-2:].tolist() == [1, 0]


def test_photo_actions_refusals():
    from fourier_feature_nets import photo_actions
    good = rows_of([[1, 2, 3], [4, 5, 6]])
    for value in (-0.01, 1.01, float("nan")):
        with pytest.raises(ValueError, match="threshold"):
            photo_actions(good, value)
    for value in (1, 0, -2, 2.5, True):
        with pytest.raises(ValueError, match="min_views"):
            photo_actions(good, 0.1, min_views=value)
    for bad in (good[:, :4], good[0], good.astype(np.int64), good.astype(np.float32)):
        with pytest.raises(ValueError, match="moments must be"):
            photo_actions(bad, 0.1)
    carried = good.copy()
    carried[0, 7] = 1
    with pytest.raises(ValueError, match="eighth field"):
        photo_actions(carried, 0.1)
    swollen = good.copy()
    swollen[0, 1] = 255 * 2 + 1
    with pytest.raises(ValueError, match="not the moments of bytes"):
        photo_actions(swollen, 0.1)
    crowded = good.copy()
    crowded[0, 3] = MAX_CAMERAS + 1
    with pytest.raises(ValueError, match="count"):
        photo_actions(crowded, 0.1)


# ------------------------------------------------------------------------------- the scenes
ALPHA_U8 = ph.ALPHA_U8


@pytest.mark.parametrize("name,leaves,cameras", [("grid", 200, 6), ("mixed", None, 5)])
def test_the_moment_scenes_have_no_undecided_pair(name, leaves, cameras):
    scale, nodes, ids, density, cams, images = ph.moment_scene(name)
    assert len(cams) == cameras and (leaves is None or len(ids) == leaves)
    proj, eyes = camera_arrays(cams, (0, 0, 0))
    for tau in (0.0, 0.3):
        got = pref.moments(scale, nodes, ids, density, images, proj, eyes, ALPHA_U8, tau)
        assert not got["undecided"].any()
        m = got["moments"]
        assert 0 < got["visible"].sum() < got["candidate"].sum() < got["pairs"]
        assert (m[:, 3] > 1).sum() > 50 and not m[:, 7].any()
        # squares are not sums: Cauchy-Schwarz, strict wherever two cameras differ
        assert (m[:, 3:4] * m[:, 4:7] >= m[:, :3] ** 2).all()
        assert (m[:, 3:4] * m[:, 4:7] > m[:, :3] ** 2).any()


def blob_images():
    scene = ph.blob_scene()
    nodes, ids, rows = scene["true"]
    return ph.images_of(ph.reference_render(scene["scale"], nodes, ids, rows[:, :3]),
                        scene["cameras"])


def test_the_two_blob_scene_loses_exactly_its_phantoms_in_the_restatement():
    """What the GPU tests rely on, held to the restatement with the float64 first hit as the
    renderer: every sweep is free of undecided pairs, three sweeps drop, the fourth converges, the
    phantoms and only they go, and sweep 2 judges leaves that sweep 1 could not."""
    scene = ph.blob_scene()
    images = blob_images()
    assert set(map(tuple, images[images[..., 3] > 0][:, :3])) == {ph.RED, ph.BLUE}
    _, ids, rows = scene["start"]
    proj, eyes = camera_arrays(scene["cameras"], (0, 0, 0))
    out = pref.carve(scene["scale"], ids, dict(zip(ids.tolist(), rows[:, 3].tolist())), images,
                     proj, eyes, ALPHA_U8, 0.3, 0.1)
    sweeps = out["sweeps"]
    assert out["converged"] and [len(s["dropped"]) > 0 for s in sweeps] == [True, True, True, False]
    assert all(s["undecided"] == 0 for s in sweeps)
    assert np.array_equal(out["leaf_index"], scene["true"][1])
    gone = np.sort(np.concatenate([s["dropped"] for s in sweeps]))
    assert np.array_equal(gone, scene["phantom_ids"]) and len(gone) == 30
    first = dict(zip(sweeps[0]["leaf_index"].tolist(), sweeps[0]["moments"][:, 3].tolist()))
    newly = [i for i, n in zip(sweeps[1]["leaf_index"].tolist(), sweeps[1]["moments"][:, 3].tolist())
             if n >= 2 and first[i] < 2]
    assert len(newly) >= 4 and set(newly) & set(sweeps[1]["dropped"].tolist())


# ------------------------------------------------------------------------------- the C ABI
def library():
    from fourier_feature_nets_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        from fourier_feature_nets_amd.build import build_library
        build_library(verbose=False)
    return _lib, ctypes.CDLL(_lib.LIB_PATH)


def test_the_symbol_is_declared_exported_bound_and_documented():
    _lib, lib = library()
    assert SYMBOL in _lib.declared_symbols()
    assert getattr(lib, SYMBOL) and getattr(_lib.load(), SYMBOL)
    with open(_lib.HEADER_PATH) as f:
        text = f.read()
    text = " ".join(text[text.index("K28a"):text.index(SYMBOL + "(")].replace("*", " ").split())
    assert "66051" in text and "bit for bit" in text and "No counterpart in the reference" in text
    from fourier_feature_nets_amd import ops
    assert ops.OCTREE_MOMENTS_MAX_CAMERAS == MAX_CAMERAS
    assert 65025 * MAX_CAMERAS < 2 ** 32 <= 65025 * (MAX_CAMERAS + 1)


def test_bad_arguments_return_nonzero_without_a_device():
    _, lib = library()
    lib.ffn_last_error_string.restype = ctypes.c_char_p
    fn = getattr(lib, SYMBOL)
    fn.restype = ctypes.c_int
    f, i64, i = ctypes.c_float, ctypes.c_int64, ctypes.c_int
    buffer = (ctypes.c_float * 64)()
    base = ctypes.addressof(buffer)
    base += (-base) % 16
    host, odd, byte = ctypes.c_void_p(base), ctypes.c_void_p(base + 4), ctypes.c_void_p(base + 1)

    def call(centers=host, leaves=8, depth=2, nodes=host, num_nodes=1, ids=host, data=host,
             stride=4, offset=3, images=host, blocks=host, cameras=2, height=4, width=4, alpha=128,
             tau=0.3, moments=host):
        return (centers, i64(leaves), f(1), i(depth), nodes, i64(num_nodes), ids, data, i(stride),
                i(offset), images, blocks, i(cameras), i(height), i(width), i(alpha), f(tau),
                moments, None)

    for kwargs, why in (({"centers": None}, "null argument"), ({"ids": None}, "null argument"),
                        ({"nodes": None}, "null argument"), ({"data": None}, "null argument"),
                        ({"images": None}, "null argument"), ({"blocks": None}, "null argument"),
                        ({"moments": None}, "null argument"),
                        ({"images": byte}, "images must be 4-byte aligned"),
                        ({"moments": odd}, "moments 16-byte aligned"),
                        ({"leaves": 0}, "num_leaves"), ({"leaves": 2 ** 31 + 1}, "num_leaves"),
                        ({"num_nodes": -1}, "num_nodes"),
                        ({"depth": 0}, "depth"), ({"depth": 12}, "depth"),
                        ({"cameras": 0}, "cameras >= 1"), ({"cameras": -3}, "cameras >= 1"),
                        ({"height": 0}, "height"), ({"width": 0}, "width"),
                        ({"height": (1 << 24) + 1}, "height"), ({"width": (1 << 24) + 1}, "width"),
                        ({"alpha": 0}, "alpha_u8"), ({"alpha": 256}, "alpha_u8"),
                        ({"tau": float("nan")}, "min_transmittance"),
                        ({"tau": -0.1}, "min_transmittance"), ({"tau": 1.0}, "min_transmittance"),
                        ({"stride": 0}, "stride"), ({"offset": -1}, "sigma_offset"),
                        ({"offset": 4}, "sigma_offset")):
        status = fn(*call(**kwargs))
        text = lib.ffn_last_error_string().decode()
        assert status != 0 and SYMBOL in text and why in text, (kwargs, text)


def good(cameras=3):
    return dict(leaf_centers=torch.zeros((8, 3)), leaf_index=torch.arange(1, 9),
                rows=torch.zeros((8, 4)), stride=4, sigma_offset=3,
                images_u8=torch.zeros((cameras, 1, 1, 4), dtype=torch.uint8),
                proj=torch.ones((cameras, 3, 4)), eyes=torch.ones((cameras, 3)), depth=2,
                alpha_u8=128, min_transmittance=0.3, moments=True)


def test_the_op_refuses_what_needs_no_device():
    from fourier_feature_nets_amd import ops
    assert ops.octree_visible_check(**good()) == (8, 3, 1, 1)
    assert ops.octree_visible_check(**good(MAX_CAMERAS)) == (8, MAX_CAMERAS, 1, 1)
    with pytest.raises(ValueError, match="octree_visible_moments: images_u8 holds 66052 cameras"):
        ops.octree_visible_check(**good(MAX_CAMERAS + 1))
    assert ops.octree_visible_check(**{**good(), "out": torch.zeros((8, 8), dtype=torch.uint32)})
    for change, why in (({"out": torch.zeros((8, 4), dtype=torch.uint32)}, "out must be"),
                        ({"out": torch.zeros((8, 8), dtype=torch.int32)}, "out must be a"),
                        ({"out": torch.zeros((7, 8), dtype=torch.uint32)}, "out must be"),
                        ({"alpha_u8": 0}, "octree_visible_moments: alpha_u8"),
                        ({"min_transmittance": 1.0}, "min_transmittance"),
                        ({"rows": torch.zeros((8, 5))}, "octree_visible_moments: rows must be")):
        with pytest.raises(ValueError, match=why):
            ops.octree_visible_check(**{**good(), **change})
    # K24's own limit and shape are what they were
    votes = {**good(ops.octree_carve_max_cameras() + 1), "moments": False}
    with pytest.raises(ValueError, match="octree_visible_votes: images_u8 holds"):
        ops.octree_visible_check(**votes)
    with pytest.raises(ValueError, match="out must be"):
        ops.octree_visible_check(**{**good(), "moments": False,
                                    "out": torch.zeros((8, 8), dtype=torch.uint32)})
    # the check comes first: host tensors never reach a launch
    args = {k: v for k, v in good().items() if k != "moments"}
    with pytest.raises(ValueError, match="alpha_u8"):
        ops.octree_visible_moments(scale=1.0, node_index=torch.zeros(1, dtype=torch.int64),
                                   **{**args, "alpha_u8": 0})


# ------------------------------------------------------------------------------- the methods
class Untouched(Scene):
    """A dataset whose sampler (and with it the device) must not be asked for."""

    @property
    def sampler(self):
        raise AssertionError("went to the device before checking")


def small_tree(channels=4, sh_degree=None):
    import fourier_feature_nets as ffn
    nodes, ids = grid_tree(2, [(1, 0, 0, 0), (1, 1, 0, 0)])
    return ffn.OcTree(1.0, nodes, ids, np.zeros((2, channels), F), sh_degree=sh_degree)


def test_the_methods_refuse_bad_arguments_before_any_device():
    import fourier_feature_nets as ffn
    cameras = rig(AXIS_EYES[:2], 4.0, 8, 8)
    images = np.zeros((2, 8, 8, 4), np.uint8)
    scene = Scene(images, cameras)
    tree = small_tree()
    crowd = Scene(np.zeros((MAX_CAMERAS + 1, 1, 1, 4), np.uint8), cameras[:1] * (MAX_CAMERAS + 1))
    for method in (tree.visible_moments, tree.carve_photo):
        with pytest.raises(ValueError, match="pass center"):           # a loaded tree has none
            method(scene)
        with pytest.raises(ValueError, match="alpha_threshold"):
            method(scene, (0, 0, 0), alpha_threshold=1.5)
        for value in (1.0, -0.1, float("nan")):
            with pytest.raises(ValueError, match="min_transmittance"):
                method(scene, (0, 0, 0), min_transmittance=value)
        with pytest.raises(ValueError, match="alpha channel"):
            method(Scene(images[..., :3], cameras), (0, 0, 0))
        with pytest.raises(ValueError, match="color_space must be RGB"):
            method(Scene(images, cameras, "YCrCb"), (0, 0, 0))
        with pytest.raises(ValueError, match="1 cameras for 2 images"):
            method(Scene(images, cameras[:1]), (0, 0, 0))
        with pytest.raises(ValueError, match="66052 cameras; at most 66051"):
            method(crowd, (0, 0, 0))
    with pytest.raises(ValueError, match="leaf_data"):
        ffn.OcTree(1.0, *grid_tree(2, [(1, 0, 0, 0)])).visible_moments(scene, (0, 0, 0))
    for value in (-0.1, 1.5, float("nan")):
        with pytest.raises(ValueError, match="OcTree.carve_photo: threshold"):
            tree.carve_photo(scene, (0, 0, 0), threshold=value)
    with pytest.raises(ValueError, match="OcTree.carve_photo: min_views"):
        tree.carve_photo(scene, (0, 0, 0), min_views=1)
    for value in (-1, 2.5, True):
        with pytest.raises(ValueError, match="max_sweeps"):
            tree.carve_photo(scene, (0, 0, 0), max_sweeps=value)
    sh = small_tree(13, 1)
    with pytest.raises(ValueError, match="coefficients, not a colour"):
        sh.carve_photo(scene, (0, 0, 0), recolor=True)
    doc = " ".join(ffn.OcTree.carve_photo.__doc__.lower().split())
    for phrase in ("one ray per", "nearest pixel", "own densities", "uniform texture", "specular",
                   "guarantee of the box carve", "untuned"):
        assert phrase in doc, phrase
    sig = inspect.signature(ffn.OcTree.carve_photo).parameters
    assert [sig[k].default for k in ("center", "threshold", "min_views", "max_sweeps",
                                     "alpha_threshold", "min_transmittance", "recolor")] == \
        [None, 0.1, 2, 16, 0.5, 0.3, False]
    sig = inspect.signature(ffn.OcTree.visible_moments).parameters
    assert sig["min_transmittance"].default == 0.3 and sig["alpha_threshold"].default == 0.5
    assert inspect.signature(ffn.photo_actions).parameters["min_views"].default == 2


def test_the_sweep_loop_on_stubbed_moments():
    """The loop alone, with the moments and ``refine`` stubbed on the host: decisions per sweep from
    one tree, the report, the stop on a sweep without drops, ``max_sweeps``, and the refusal to drop
    every leaf."""
    import fourier_feature_nets as ffn
    loud, calm = rows_of([[0, 0, 0], [255, 255, 255]])[0], rows_of([[9, 9, 9], [9, 9, 9]])[0]
    one, none = rows_of([[5, 5, 5]])[0], np.zeros(8, np.uint32)

    class Stub(ffn.OcTree):
        def __init__(self, script, leaves):
            self.script, self.leaves = script, leaves

        num_leaves = property(lambda self: self.leaves)

        def _dev(self):
            return "cpu"

        def _visible_moments_on_device(self, images, cameras, alpha_u8, center, tau):
            return torch.from_numpy(np.stack(self.script[0]).astype(np.int64)).to(torch.uint32)

        def refine(self, action):
            parent = np.nonzero(np.asarray(action) != 0)[0]
            return Stub(self.script[1:], len(parent)), parent

    images = np.zeros((2, 1, 1, 4), np.uint8)
    script = [[loud, calm, one, none, loud], [calm, loud, none], [calm, one]]
    args = ("who", images, [None, None], 128, (0, 0, 0), 0.1, 2)
    tree, report, last, origin = Stub(script, 5)._photo_sweeps(*args, 16, 0.3)
    assert [tuple(s) for s in report] == [(5, 4, 3, 2), (3, 2, 2, 1), (2, 2, 1, 0)]
    assert report.converged and tree.leaves == 2 and origin.tolist() == [1, 3]
    assert np.array_equal(last, np.stack(script[2]))
    tree, report, last, origin = Stub(script, 5)._photo_sweeps(*args, 2, 0.3)
    assert len(report) == 2 and not report.converged and last is None and origin.tolist() == [1, 3]
    tree, report, last, origin = Stub(script, 5)._photo_sweeps(*args, 2, 0.3, True)
    assert np.array_equal(last, np.stack(script[2]))          # one more call, of the final tree
    tree, report, last, origin = Stub(script, 5)._photo_sweeps(*args, 0, 0.3)
    assert report == [] and not report.converged and origin.tolist() == [0, 1, 2, 3, 4]
    with pytest.raises(ValueError, match="threshold"):
        Stub([[loud, loud]], 2)._photo_sweeps(*args, 16, 0.3)


def test_build_from_silhouettes_routes_by_photo_threshold(monkeypatch):
    """``photo_threshold=None`` never asks for sweeps.  With a threshold the unmerged hull is
    swept with the carve's own alpha threshold and ``visible_transmittance``; the cells that are
    left go, in code order, to the ``color="visible"`` votes of a second unmerged tree and then to
    ``_from_cells`` with the caller's tolerances.  (Host tensors, stubs for the kernels.)"""
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import octree as octree_module
    cameras = rig(AXIS_EYES[:2], 4.0, 8, 8)
    scene = Scene(np.full((2, 8, 8, 4), 255, np.uint8), cameras)
    scene.sampler = type("S", (), {"device": "cpu"})()
    codes = torch.tensor([3, 9, 12], dtype=torch.int32)
    data = torch.tensor([[.1, .2, .3, 5.], [.4, .5, .6, 5.], [.7, .8, .9, 5.]])
    calls, swept, asked = [], [], []

    class Hull:
        def __init__(self, leaves):
            self.leaves = leaves

        def _photo_sweeps(self, who, images, cams, alpha_u8, center, threshold, min_views,
                          max_sweeps, tau, want_moments=False):
            swept.append((self.leaves, alpha_u8, center, threshold, min_views, max_sweeps, tau))
            report = ffn.PhotoReport([ffn.PhotoSweep(3, 3, 3, 1), ffn.PhotoSweep(2, 2, 2, 0)])
            report.converged = True
            return None, report, None, np.array([0, 2], np.int64)

        def _visible_votes_on_device(self, images, cams, alpha_u8, center, tau):
            asked.append((self.leaves, tau))
            return torch.from_numpy(np.array([[255, 0, 510, 2], [51, 102, 153, 1]], np.uint32))

    def from_cells(codes_in, data_in, depth, scale, center, tolerances, device):
        calls.append((codes_in.clone(), data_in.clone(), tolerances))
        return Hull(len(codes_in)) if tolerances is None else "tree"

    monkeypatch.setattr(octree_module.ops, "octree_carve_select",
                        lambda *a, **k: (codes.clone(), data.clone()))
    monkeypatch.setattr(ffn.OcTree, "_from_cells", staticmethod(from_cells))
    build = ffn.OcTree.build_from_silhouettes
    for kwargs, why in (({"photo_threshold": 1.5}, "photo_threshold"),
                        ({"photo_threshold": float("nan")}, "photo_threshold"),
                        ({"photo_threshold": 0.1, "photo_min_views": 1}, "photo_min_views"),
                        ({"photo_threshold": 0.1, "photo_max_sweeps": -1}, "photo_max_sweeps"),
                        ({"photo_threshold": 0.1, "visible_transmittance": 1.0},
                         "visible_transmittance")):
        with pytest.raises(ValueError, match=why):
            build(Untouched(scene.images, cameras), 3, **kwargs)
    assert build(scene, 3, merge_tolerance=0.25) == "tree" and len(calls) == 1 and not swept
    calls.clear()
    report = ffn.PhotoReport()
    assert build(scene, 3, center=(0.5, 0, 0), alpha_threshold=0.25, merge_tolerance=0.25,
                 visible_transmittance=0.1, photo_threshold=0.2, photo_min_views=3,
                 photo_max_sweeps=5, photo_report=report) == "tree"
    assert swept == [(3, 64, (0.5, 0.0, 0.0), 0.2, 3, 5, 0.1)] and not asked
    assert [tuple(s) for s in report] == [(3, 3, 3, 1), (2, 2, 2, 0)] and report.converged
    assert len(calls) == 2 and calls[0][2] is None and calls[1][2] == (0.25, 0.25)
    assert torch.equal(calls[0][0], codes) and torch.equal(calls[0][1], data)
    assert torch.equal(calls[1][0], codes[[0, 2]]) and torch.equal(calls[1][1], data[[0, 2]])
    # with color="visible" the votes come from the thinned cells
    calls.clear()
    swept.clear()
    assert build(scene, 3, color="visible", photo_threshold=0.2, merge_tolerance=0.25) == "tree"
    assert [c[0].tolist() for c in calls] == [[3, 9, 12], [3, 12], [3, 12]]
    assert swept[0][0] == 3 and swept[0][6] == 0.3 and asked == [(2, 0.3)]
    want = data.numpy()[[0, 2]].copy()
    want[0, :3] = F([255, 0, 510]) / F(510)
    want[1, :3] = F([51, 102, 153]) / F(255)
    assert np.array_equal(bits(calls[2][1].numpy()), bits(want))
    sig = inspect.signature(build).parameters
    assert [sig[k].default for k in ("photo_threshold", "photo_min_views", "photo_max_sweeps")] == \
        [None, 2, 16]


# ------------------------------------------------------------------------------- the programs
def test_program_parsers():
    sys.path.insert(0, ROOT)
    import fourier_feature_nets as ffn
    from scripts import carve_octree, photo_carve_octree
    parser = carve_octree.build_parser()
    text = parser.format_help()
    for flag in ("--photo-threshold", "--photo-min-views", "--photo-max-sweeps"):
        assert flag in text
    args = parser.parse_args(["d", "t"])
    assert args.photo_threshold is None and args.photo_min_views == 2
    assert args.photo_max_sweeps == 16
    args = parser.parse_args(["d", "t", "--photo-threshold", "0.2", "--photo-min-views", "3",
                              "--photo-max-sweeps", "4"])
    assert (args.photo_threshold, args.photo_min_views, args.photo_max_sweeps) == (0.2, 3, 4)
    parser = photo_carve_octree.build_parser()
    args = parser.parse_args(["tree.npz", "data.npz", "out.npz"])
    assert (args.tree_path, args.data_path, args.output_path) == ("tree.npz", "data.npz", "out.npz")
    assert args.center == [0.0, 0.0, 0.0] and args.split == "train" and args.recolor is False
    sig = inspect.signature(ffn.OcTree.carve_photo).parameters
    for name in ("threshold", "min_views", "max_sweeps", "alpha_threshold", "min_transmittance"):
        assert getattr(args, name) == sig[name].default, name
    args = parser.parse_args(["a", "b", "c", "--center", "0.5", "-1", "2", "--split", "val",
                              "--threshold", "0.05", "--min-views", "3", "--max-sweeps", "2",
                              "--alpha-threshold", "0.25", "--min-transmittance", "0.1",
                              "--recolor"])
    assert args.center == [0.5, -1.0, 2.0] and args.split == "val" and args.recolor is True
    assert (args.threshold, args.min_views, args.max_sweeps) == (0.05, 3, 2)
    assert args.alpha_threshold == 0.25 and args.min_transmittance == 0.1
    for bad in (["a", "b"], ["a", "b", "c", "--split", "all"], ["a", "b", "c", "--min-views", "x"],
                ["a", "b", "c", "--center", "1", "2"]):
        with pytest.raises(SystemExit):
            parser.parse_args(bad)
    report = ffn.PhotoReport([ffn.PhotoSweep(5, 4, 3, 2), ffn.PhotoSweep(3, 3, 3, 0)])
    report.converged = True
    import contextlib
    import io
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        carve_octree.print_report(report)
    assert "photo sweep 1: 5 leaves, 4 seen, 3 judged, 2 dropped" in out.getvalue()
    assert "converged after 2 sweeps" in out.getvalue()
