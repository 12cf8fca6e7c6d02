"""K18 on the GPU: the SH volume render (K18a, ``OcTree.render_volume`` of a tree with
``sh_degree``) against hand-written answers, against its float64 restatement
(tests/octree_sh_reference.py) and against K15 where the two must agree; the projection kernel
(K18b) bit for bit against numpy float32; ``OcTree.bake_sh`` on a model whose coefficients are
known; and the two programs.  No reference file is read.

Colour and alpha are compared within the per-ray budgets of the restatement on every ray whose
margin exceeds ``ray_budget`` (tests/octree_render_helpers.py); at most 2 % of a case is left out,
asserted here and, for the float64 walk alone, in tests/test_octree_sh_cpu.py."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_sh_reference as shref
from tests import octree_walk_reference as wref
from tests.octree_render_helpers import LEFT_OUT_CAP, SCENE, ray_budget
from tests.octree_sh_helpers import DEGREES, SIZES, TREES, case, prefix, sh_leaf_data
from tests.octree_volume_helpers import hand_case
from tests.octree_walk_helpers import opaque_ball

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BG = (0.25, 0.5, 0.125)
EPS = 2.0 ** -24
Y0 = 0.28209479177387814


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-np.asarray(z, np.float64)))


def sh_tree(scale, nodes, leaves, data, degree):
    import fourier_feature_nets as ffn
    return ffn.OcTree(float(scale), nodes, leaves, data, sh_degree=degree)


def plain_tree(scale, nodes, leaves, data):
    import fourier_feature_nets as ffn
    return ffn.OcTree(float(scale), nodes, leaves, data)


@pytest.mark.parametrize("degree", DEGREES)
def test_known_answers_in_one_leaf(degree):
    """The root is the only leaf (scale 2, density 0.5): a ray through the centre along an axis has
    a chord of 4 in the world, whatever the length of its direction."""
    bases = (degree + 1) ** 2
    rng = np.random.default_rng(3)
    k = ((rng.random((3, bases)) * 2 - 1) * 2).astype(np.float32)
    data = np.concatenate([k.reshape(-1), np.float32([0.5])])[None, :]
    tree = sh_tree(2.0, np.zeros(0, np.int64), np.array([0], np.int64), data, degree)
    dirs = np.float32([[1, 0, 0], [-1, 0, 0], [0, 2, 0], [0, -2, 0], [0, 0, 0.5], [0, 0, -0.5],
                       [1, 1, 0], [1, -2, 2]])
    starts = (-5 * dirs / np.linalg.norm(dirs, axis=1, keepdims=True)).astype(np.float32)
    out = tree.render_volume(starts, dirs, background=BG)
    assert type(out).__name__ == "RenderResult"
    assert all(isinstance(x, np.ndarray) and x.dtype == np.float32 for x in out)
    w = wref.walk(2.0, np.zeros(0, np.int64), np.array([0], np.int64), starts, dirs)
    v = shref.composite(w, 2.0, starts, dirs, data, degree, 0.0, BG)
    u = dirs.astype(np.float64) / np.linalg.norm(dirs.astype(np.float64), axis=1, keepdims=True)
    x, y, z = u[:, 0], u[:, 1], u[:, 2]
    table = [np.full(8, Y0), -0.4886025119029199 * y, 0.4886025119029199 * z,
             -0.4886025119029199 * x, 1.0925484305920792 * x * y, -1.0925484305920792 * y * z,
             0.31539156525252005 * (2 * z * z - x * x - y * y), -1.0925484305920792 * x * z,
             0.5462742152960396 * (x * x - y * y)]
    basis = np.stack(table[:bases], 1)
    colour = sigmoid(basis @ k.astype(np.float64).T)                     # (8,3)
    chord = np.where(np.arange(8) < 6, 4.0, 0.0)
    # the oblique rays: the chord of the cube [-2, 2]^3 through its centre
    chord[6] = 4.0 * np.sqrt(2.0)
    chord[7] = 4.0 / (2.0 / 3.0)
    a = 1.0 - np.exp(-0.5 * chord)
    want = a[:, None] * colour + (1 - a)[:, None] * np.float32(BG).astype(np.float64)[None, :]
    err = np.abs(out.color.astype(np.float64) - want).max(1)
    print("one leaf, degree %d: worst colour error / budget %.3f" % (degree, (err / v["budget_c"]).max()))
    assert (err <= v["budget_c"]).all()
    assert (np.abs(out.alpha.astype(np.float64) - a) <= v["budget_a"]).all()
    # opposite directions: the band-1 terms change sign, so the colours differ
    for i in (0, 2, 4):
        assert np.abs(out.color[i] - out.color[i + 1]).max() > 1e-3
        assert bits(out.alpha[i]) == bits(out.alpha[i + 1])


def check_sh(what, scale, data, degree, starts, directions, t_min, got, w, ok):
    """Asserts ``got`` against the restatement, depth as the K15 test checks it; -> v."""
    v = shref.composite(w, scale, starts, directions, data, degree, t_min, BG)
    count = len(w["hit"])
    assert got.color.shape == (count, 3) and got.alpha.shape == got.depth.shape == (count,)
    assert got.color.dtype == got.alpha.dtype == got.depth.dtype == np.float32
    left_out = 1.0 - ok.mean()
    took = v["count"] > 0
    err_c = np.abs(got.color.astype(np.float64) - v["color"]).max(1)
    err_a = np.abs(got.alpha.astype(np.float64) - v["alpha"])
    print("%s degree %d n=%d t_min=%.2f: %d take a leaf, %.4f left out; worst error / budget: "
          "colour %.3f alpha %.3f" % (what, degree, count, t_min, took.sum(), left_out,
                                      (err_c / v["budget_c"])[ok].max(),
                                      (err_a / v["budget_a"])[ok].max()))
    assert left_out <= LEFT_OUT_CAP
    assert (err_c <= v["budget_c"])[ok].all()
    assert (err_a <= v["budget_a"])[ok].all()
    none = ok & ~took
    assert (bits(got.color[none]) == bits(np.float32(BG))[None, :]).all()
    assert (got.alpha[none] == 0).all() and (got.depth[none] == 0).all()
    depth = got.depth.astype(np.float64)
    sure = ok & (v["best"] >= 0) & (v["gap"] > 2 * v["budget_a"])
    clamped = sure & v["clamped"]
    free = sure & ~v["clamped"]
    assert (bits(got.depth[clamped]) == bits(np.float32(t_min))).all()
    allowed = np.zeros(count)
    allowed[v["best"] >= 0] = v["entry"][v["best"][v["best"] >= 0]]
    assert (np.abs(depth - v["depth"]) <= allowed)[free].all()
    taken_ray = w["ray"][v["taken"]]
    nearest = np.full(count, np.inf)
    np.minimum.at(nearest, taken_ray, np.abs(depth[taken_ray] - v["t0"]) - v["entry"])
    heaviest = np.zeros(count)
    np.maximum.at(heaviest, taken_ray, v["weights"])
    unsure = ok & took & ~sure
    fine = (nearest <= 0) | ((got.depth == 0) & (heaviest <= 2 * v["budget_a"]))
    assert fine[unsure].all()
    return v


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("name", sorted(TREES))
def test_sh_render_equals_the_restatement(name, degree):
    scale, nodes, leaves, starts, directions, w, ok = case(name)
    data = sh_leaf_data(scale, leaves, degree)
    tree = sh_tree(scale, nodes, leaves, data, degree)
    full = tree.render_volume(starts, directions, 0.0, BG)
    for n in SIZES:
        got = tree.render_volume(starts[:n], directions[:n], 0.0, BG)
        check_sh(name, scale, data, degree, starts[:n], directions[:n], 0.0, got, prefix(w, n),
                 ok[:n])
        for a, b in zip(got, full):          # a ray's answer does not depend on its neighbours
            assert np.array_equal(bits(a), bits(b[:n]))
    # t_min inside the leaves: the depth of a cut leaf is t_min itself
    t_min = float(np.float32(1.0 * float(scale)))
    got = tree.render_volume(starts, directions, t_min, BG)
    check_sh(name, scale, data, degree, starts, directions, t_min, got, w, ok)
    # device tensors in, device tensors out, the same bits
    dev = tree.render_volume(torch.from_numpy(starts).cuda(), torch.from_numpy(directions).cuda(),
                             t_min, BG)
    assert all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in dev)
    for a, b in zip(dev, got):
        assert np.array_equal(bits(a.cpu().numpy()), bits(b))


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("name", sorted(TREES))
def test_reduction_to_k15(name, degree):
    """Bands >= 1 zero and band 0 = logit / Y_0: the colour no longer depends on the view, and the
    plain tree [sigmoid(logit), sigma] is the same volume.  alpha and depth: the same bits.  Colour:
    (logit / Y_0) * Y_0 is within 2^-23 |logit| of the logit, a quarter of that in the colour with
    |logit| <= 1, and the two sigmoids round on their own: 4 * 2^-24 per unit of sum w = alpha
    (a black background, so that nothing else is in the sum)."""
    from fourier_feature_nets_amd import ops
    scale, nodes, leaves, starts, directions, _, _ = case(name)
    bases = (degree + 1) ** 2
    rng = np.random.default_rng(5)
    logits = np.zeros((len(leaves), 4), np.float32)
    logits[:, :3] = rng.random((len(leaves), 3)) * 2 - 1
    sigma = sh_leaf_data(scale, leaves, degree)[:, -1]
    data = np.zeros((len(leaves), 3 * bases + 1), np.float32)
    data[:, 0:3 * bases:bases] = logits[:, :3] / np.float32(Y0)
    data[:, -1] = sigma
    flat = ops.octree_bake(torch.from_numpy(logits).cuda()).cpu().numpy()
    flat[:, 3] = sigma
    for t_min, min_t in ((0.0, 0.0), (float(scale), 0.0), (0.0, 0.5)):
        sh = sh_tree(scale, nodes, leaves, data, degree).render_volume(
            starts, directions, t_min, min_transmittance=min_t)
        k15 = plain_tree(scale, nodes, leaves, flat).render_volume(
            starts, directions, t_min, min_transmittance=min_t)
        assert np.array_equal(bits(sh.alpha), bits(k15.alpha))
        assert np.array_equal(bits(sh.depth), bits(k15.depth))
        diff = np.abs(sh.color.astype(np.float64) - k15.color.astype(np.float64)).max(1)
        allowed = 4 * EPS * k15.alpha.astype(np.float64)
        print("%s degree %d t_min %.2f min_T %.1f: worst colour difference / (4 eps alpha) %.3f, "
              "%d rays with alpha > 0" % (name, degree, t_min, min_t,
                                          (diff[allowed > 0] / allowed[allowed > 0]).max(),
                                          (allowed > 0).sum()))
        assert (diff <= allowed).all()
        assert (k15.alpha > 0).sum() > 200


@pytest.mark.parametrize("degree", DEGREES)
def test_walk_options(degree):
    """``hand_case``: t_min inside leaf 0 on ray 0, and min_transmittance = 0.5 behind the opaque
    leaf 2 on the diagonal -- as in K15: the walk ends, alpha is the plain tree's bit for bit."""
    scale, nodes, leaves, flat, starts, dirs = hand_case()
    data = sh_leaf_data(scale, leaves, degree)
    data[:, -1] = flat[:, 3]
    tree = sh_tree(scale, nodes, leaves, data, degree)
    plain = plain_tree(scale, nodes, leaves, flat)
    w = wref.walk(scale, nodes, leaves, starts, dirs)
    for t_min, min_t in ((0.0, 0.0), (0.75, 0.0), (1.0, 0.0), (0.0, 0.5), (2.25, 0.05)):
        got = tree.render_volume(starts, dirs, t_min, BG, min_t)
        ref = plain.render_volume(starts, dirs, t_min, BG, min_t)
        assert np.array_equal(bits(got.alpha), bits(ref.alpha))
        assert np.array_equal(bits(got.depth), bits(ref.depth))
        v = shref.composite(w, scale, starts, dirs, data, degree, t_min, BG, min_t)
        # rays 0 .. 2 within the budget; 3 and 4 end in the opaque leaf, whose density of 1e30
        # makes the budget expression meaningless: four leaf steps of rounding
        err = np.abs(got.color.astype(np.float64) - v["color"]).max(1)
        assert (err[:3] <= v["budget_c"][:3]).all()
        assert (err[3:] <= 8 * 4 * EPS + v["own"][3:]).all()
    cut = tree.render_volume(starts, dirs, 0.75, BG)
    assert bits(cut.depth[0]) == bits(np.float32(0.75))
    gone = tree.render_volume(starts, dirs, 1.0, BG)
    assert np.array_equal(bits(gone.color[0]), bits(np.float32(BG))) and gone.alpha[0] == 0
    # min_transmittance = 0.5.  Ray 4 meets the opaque leaf alone: the walk had ended there with any
    # threshold.  On the diagonal leaf 0 leaves T = exp(-2 sqrt 3) = 0.031 <= 0.5, so the walk ends
    # after it and never reaches the opaque leaf: alpha is 1 - T, not 1, as the plain tree's
    early = tree.render_volume(starts, dirs, 0.0, BG, 0.5)
    late = tree.render_volume(starts, dirs, 0.0, BG, 0.0)
    assert early.alpha[4] == 1.0 and late.alpha[4] == 1.0 and late.alpha[3] == 1.0
    assert np.array_equal(bits(early.color[4]), bits(late.color[4]))
    assert abs(float(early.alpha[3]) - (1 - np.exp(-2 * np.sqrt(3.0)))) <= 8 * 2 * EPS
    assert bits(early.alpha[3]) == bits(plain.render_volume(starts, dirs, 0.0, BG, 0.5).alpha[3])
    assert bits(early.depth[3]) == bits(np.float32(1.0))
    with pytest.raises(Exception, match="t_min"):
        tree.render_volume(starts, dirs, float("nan"))


@pytest.mark.parametrize("degree", DEGREES)
def test_directions(degree):
    scale, nodes, leaves, starts, directions, w, ok = case("mixed4")
    data = sh_leaf_data(scale, leaves, degree)
    tree = sh_tree(scale, nodes, leaves, data, degree)
    base = tree.render_volume(starts, directions, 0.0, BG)
    v = shref.composite(w, scale, starts, directions, data, degree, 0.0, BG)
    for factor in (1e-3, 1e3):
        scaled = (directions * np.float32(factor)).astype(np.float32)
        ws = wref.walk(scale, nodes, leaves, starts, scaled)
        got = tree.render_volume(starts, scaled, 0.0, BG)
        diff = np.abs(got.color.astype(np.float64) - base.color.astype(np.float64)).max(1)
        both_ok = ok & (~ws["hit"] | (ws["margin"] > ray_budget(ws, scale, starts, scaled)))
        assert 1.0 - both_ok.mean() <= LEFT_OUT_CAP
        allowed = 2 * v["budget_c"]                   # twice the budget of the unscaled rays
        print("directions x %g, degree %d: worst colour difference / allowed %.3f"
              % (factor, degree, (diff / allowed)[both_ok].max()))
        assert (diff <= allowed)[both_ok].all()
        assert np.abs(got.alpha.astype(np.float64) - base.alpha)[both_ok].max() <= \
            2 * v["budget_a"].max()
    # rays no walk can follow: the background, 0 and 0 exactly, and no NaN anywhere
    s = float(scale)
    bad_s = np.float32([[0, 0, 0], [np.nan, 0, 0], [0, 0, 0], [2 * s, 0, 0], [np.inf, 0, 0],
                        [0, 0.1, 3 * s]])
    bad_d = np.float32([[0, 0, 0], [1, 1, 1], [np.nan, 1, 0], [0, 1, 1], [1, 0, 0], [1, 0, 0]])
    bad = tree.render_volume(bad_s, bad_d, 0.0, BG)
    assert (bits(bad.color) == bits(np.float32(BG))[None, :]).all()
    assert (bits(bad.alpha) == 0).all() and (bits(bad.depth) == 0).all()
    # among good rays they change nothing
    mixed_s = np.concatenate([starts[:70], bad_s, starts[70:130]])
    mixed_d = np.concatenate([directions[:70], bad_d, directions[70:130]])
    both = tree.render_volume(mixed_s, mixed_d, 0.0, BG)
    assert not any(np.isnan(x).any() for x in both)
    assert np.array_equal(bits(both.color[:70]), bits(base.color[:70]))
    assert np.array_equal(bits(both.color[76:]), bits(base.color[70:130]))
    assert (bits(both.color[70:76]) == bits(np.float32(BG))[None, :]).all()
    # numpy and tensors are not mixed, as in walk
    with pytest.raises(TypeError, match="both"):
        tree.render_volume(starts, torch.from_numpy(directions).cuda())
    with pytest.raises(TypeError, match="both"):
        tree.render_volume(torch.from_numpy(starts).cuda(), directions)


def test_nothing_is_inferred_from_the_channel_count():
    """13 channels without ``sh_degree``: the first four are [r, g, b, sigma], as today."""
    from fourier_feature_nets_amd import ops
    scale, nodes, leaves, starts, directions, _, _ = case("mixed4")
    data = np.abs(sh_leaf_data(scale, leaves, 1)) * np.float32(0.25)
    tree = plain_tree(scale, nodes, leaves, data)
    assert tree.sh_degree is None and data.shape[1] == 13
    got = tree.render_volume(starts, directions, 0.0, BG)
    dev = [torch.from_numpy(x).cuda() for x in (starts, directions, nodes, leaves, data)]
    want = ops.octree_render_volume(dev[0], dev[1], float(scale), tree.depth, dev[2], dev[3],
                                    dev[4], 0.0, BG, 0.0)
    for a, b in zip(got, want):
        assert np.array_equal(bits(a), bits(b.cpu().numpy()))
    four = plain_tree(scale, nodes, leaves, data[:, :4].copy()).render_volume(starts, directions,
                                                                              0.0, BG)
    for a, b in zip(got, four):
        assert np.array_equal(bits(a), bits(b))
    sh = sh_tree(scale, nodes, leaves, data, 1).render_volume(starts, directions, 0.0, BG)
    assert not np.array_equal(bits(sh.color), bits(got.color))


@pytest.mark.parametrize("degree", DEGREES)
@pytest.mark.parametrize("n", [1, 64, 65, 4097])
def test_k18b_bit_for_bit(n, degree):
    from fourier_feature_nets_amd import ops
    bases = (degree + 1) ** 2
    views = 5
    rng = np.random.default_rng(100 * degree + n)
    logits = ((rng.random((views, n, 4)) * 2 - 1) * 6).astype(np.float32)
    logits[0, 0, 3] = 25.0                                   # beyond softplus' threshold
    weights = ((rng.random((views, bases)) * 2 - 1)).astype(np.float32)
    inv = np.float32(1.0 / views)

    def run():
        out = torch.zeros((n, 3 * bases + 1), dtype=torch.float32, device="cuda")
        for j in range(views):
            same = ops.octree_sh_accumulate(torch.from_numpy(logits[j]).cuda(), out, weights[j],
                                            float(inv), degree)
            assert same is out
        return out.cpu().numpy()

    got = run()
    want = np.zeros((n, 3 * bases + 1), np.float32)
    for j in range(views):
        for c in range(3):
            term = weights[j][None, :] * logits[j][:, c:c + 1]            # f32 product
            want[:, c * bases:(c + 1) * bases] = want[:, c * bases:(c + 1) * bases] + term
        soft = ops.octree_bake(torch.from_numpy(logits[j]).cuda()).cpu().numpy()[:, 3]
        want[:, -1] = want[:, -1] + soft * inv
    assert want.dtype == np.float32
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(run()), bits(got))
    # a batch is a slice of the rows
    if n > 64:
        out = torch.zeros((n, 3 * bases + 1), dtype=torch.float32, device="cuda")
        for j in range(views):
            for lo, hi in ((0, 37), (37, n)):
                ops.octree_sh_accumulate(torch.from_numpy(logits[j, lo:hi].copy()).cuda(),
                                         out[lo:hi], weights[j], float(inv), degree)
        assert np.array_equal(bits(out.cpu().numpy()), bits(got))
    with pytest.raises(ValueError, match="weights"):
        ops.octree_sh_accumulate(torch.zeros((n, 4), device="cuda"),
                                 torch.zeros((n, 3 * bases + 1), device="cuda"), weights[0][:-1],
                                 1.0, degree)
    with pytest.raises(ValueError, match="leaf_data"):
        ops.octree_sh_accumulate(torch.zeros((n, 4), device="cuda"),
                                 torch.zeros((n, 3 * bases), device="cuda"), weights[0], 1.0,
                                 degree)


class KnownCoefficients(torch.nn.Module):
    """logit_c(x, view) = sum_b A_cb(x) Y_b(view) for a smooth A, and a positive sigma logit that
    depends on the view too."""
    use_view = True

    def __init__(self):
        super().__init__()
        self.dummy = torch.nn.Parameter(torch.zeros(1))
        self.calls = []

    @staticmethod
    def coefficients(x):
        """(N,3) float64 -> (N,3,9)"""
        c = np.arange(3, dtype=np.float64)[None, :, None]
        b = np.arange(9, dtype=np.float64)[None, None, :]
        px, py, pz = [x[:, i][:, None, None] for i in range(3)]
        return np.sin(1.3 * px + 0.7 * c + 0.4 * b) + 0.5 * np.cos(0.9 * py - 1.1 * pz + 0.3 * b * c)

    @staticmethod
    def sigma_logit(x, view):
        return 1.0 + 0.5 * x[:, 0] * view[:, 2] + 0.25 * view[:, 0]

    def forward(self, positions, views):
        from fourier_feature_nets_amd.octree import sh_basis
        self.calls.append(int(positions.shape[0]))
        x = positions.detach().cpu().numpy().astype(np.float64)
        v = views.detach().cpu().numpy().astype(np.float64)
        assert (v == v[0]).all()                       # one direction for the whole batch
        y = sh_basis(v, 2)
        rgb = (self.coefficients(x) * y[:, None, :]).sum(2)
        out = np.concatenate([rgb, self.sigma_logit(x, v)[:, None]], 1)
        return torch.from_numpy(out.astype(np.float32)).to(positions.device)


def test_bake_sh_recovers_known_coefficients():
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd.octree import sh_basis, sh_view_directions
    model = KnownCoefficients().cuda()
    cloud = np.random.default_rng(8).random((4000, 3), dtype=np.float32) * 2 - 1
    bare = ffn.OcTree.build_from_samples(torch.from_numpy(cloud).cuda(), 3, 1)
    assert bare.depth == 3 and bare.num_leaves > 30
    before = bare.state_dict
    tree = bare.bake_sh(model, degree=2, num_views=64)
    assert tree is not bare and tree.sh_degree == 2 and bare.sh_degree is None
    assert bare.leaf_data() is None and tree.center == bare.center
    assert np.array_equal(tree.state_dict["leaf_index"], before["leaf_index"])
    assert np.array_equal(tree.state_dict["node_index"], before["node_index"])
    assert model.calls == [bare.num_leaves] * 64 and model.training
    data = tree.leaf_data()
    assert data.shape == (bare.num_leaves, 28) and data.dtype == np.float32
    # the points the model is given: one f32 add, as bake_sh makes it
    centres = (bare.leaf_centers() + np.float32(bare.center)[None, :]).astype(np.float64)
    want = KnownCoefficients.coefficients(centres).reshape(-1, 27)
    views = sh_view_directions(64)
    y = sh_basis(views, 2)
    # Tolerance.  The model's logits are f32 roundings of sum_b A_b Y_b: each within eps * L with
    # L = max |logit|; and it is handed the f32 rounding of a view, within eps of it per component,
    # which moves a logit by at most 1.6 eps sum_b |A_b| (the gradient bound of
    # tests/octree_sh_reference.py): together dl per logit.  The fit is k = P l with P = pinv(Y) cast to f32: a perturbation dl of the
    # 64 logits moves k by at most |dl|_2 / smin(Y) <= sqrt(64) dl / smin(Y); the cast of P adds
    # eps |P| |l| <= eps * sum_j |P_bj| L per coefficient; the accumulation is 64 products and 64
    # sums in f32, each within eps of a partial sum of at most sum_j |P_bj| L: 128 eps sum_j |P_bj| L.
    # With cond(Y) = smax / smin = 1.0136 for these 64 views the first term is the smallest.
    smin = np.linalg.svd(y, compute_uv=False).min()
    level = float(np.abs((want.reshape(-1, 3, 9)[:, :, None, :] * y[None, None, :, :]).sum(3)).max())
    p_rows = np.abs(np.linalg.pinv(y)).sum(1).max()
    spread = 1.6 * float(np.abs(want.reshape(-1, 3, 9)).sum(2).max())
    tolerance = EPS * ((level + spread) * 8.0 / smin + 129.0 * p_rows * level)
    err = np.abs(data[:, :27].astype(np.float64) - want).max()
    print("bake_sh recovery: %d leaves, cond(Y) %.4f, worst |k - A| %.3g, tolerance %.3g"
          % (len(data), np.linalg.cond(y), err, tolerance))
    assert err <= tolerance
    # sigma: the mean over the views of softplus: the sigma logit and its view in f32 (2 eps, the
    # slope of softplus is below 1), softplus within 4 ulp = 8 eps relative, a product with 1/64
    # (exact) and 64 sums of at most the largest term each, and the result's own rounding
    soft = np.stack([np.log1p(np.exp(KnownCoefficients.sigma_logit(centres, np.repeat(v[None], len(centres), 0))))
                     for v in views], 0)
    mean = soft.mean(0)
    assert (np.abs(data[:, 27].astype(np.float64) - mean) <= (64 + 8 + 2 + 1) * EPS * soft.max()).all()
    # batches: the same bits
    model.calls.clear()
    small = bare.bake_sh(model, degree=2, num_views=64, batch_size=5)
    assert np.array_equal(bits(small.leaf_data()), bits(data))
    assert len(model.calls) == 64 * -(-bare.num_leaves // 5) and max(model.calls) == 5
    again = bare.bake_sh(model, degree=2, num_views=64)
    assert np.array_equal(bits(again.leaf_data()), bits(data))
    one = bare.bake_sh(model, degree=1, num_views=8)
    assert one.sh_degree == 1 and one.leaf_data().shape == (bare.num_leaves, 13)
    # the render of the baked tree sees the view: two opposite rays through one leaf differ
    o = np.float32([[0.1, 0.2, -3], [0.1, 0.2, 3]])
    d = np.float32([[0, 0, 1], [0, 0, -1]])
    out = tree.render_volume(o, d)
    assert out.alpha[0] > 0.1 and np.abs(out.color[0] - out.color[1]).max() > 1e-3


def test_bake_sh_of_a_model_without_view():
    import fourier_feature_nets as ffn
    torch.manual_seed(7)
    model = ffn.PositionalFourierMLP(3, 4, 5.5, num_channels=64).to("cuda")
    scale, nodes, leaves, starts, directions, _, _ = case("mixed4")
    bare = plain_tree(scale, nodes, leaves, None)
    center = (0.125, -0.25, 0.0625)
    with pytest.raises(ValueError, match="cent"):
        bare.bake_sh(model)
    flat = bare.bake(model, center=center)
    for degree in DEGREES:
        bases = (degree + 1) ** 2
        tree = bare.bake_sh(model, degree=degree, center=center, batch_size=50)
        assert tree.sh_degree == degree and tree.center == center and flat.sh_degree is None
        data = tree.leaf_data()
        assert data.shape == (len(leaves), 3 * bases + 1) and data.dtype == np.float32
        higher = np.ones(3 * bases + 1, bool)
        higher[0:3 * bases:bases] = False
        higher[-1] = False
        assert (data[:, higher] == 0).all() and np.abs(data[:, 0:3 * bases:bases]).max() > 0
        assert np.array_equal(bits(data[:, -1]), bits(flat.leaf_data()[:, 3]))
        sh = tree.render_volume(starts, directions)
        k15 = flat.render_volume(starts, directions)
        assert np.array_equal(bits(sh.alpha), bits(k15.alpha))
        assert np.array_equal(bits(sh.depth), bits(k15.depth))
        # the reduction tolerance of test_reduction_to_k15
        logit = np.abs(data[:, 0:3 * bases:bases].astype(np.float64) * Y0).max()
        diff = np.abs(sh.color.astype(np.float64) - k15.color.astype(np.float64)).max(1)
        allowed = 4 * EPS * k15.alpha.astype(np.float64)
        print("no view, degree %d: largest |logit| %.2f, worst colour difference / allowed %.3f"
              % (degree, logit, (diff[allowed > 0] / allowed[allowed > 0]).max()))
        assert (diff <= allowed).all()


def test_bake_sh_and_render_programs(tmp_path):
    """bake_octree.py --sh-degree 2, then render_octree.py --mode volume without a flag of its
    own: the file says what it is."""
    from PIL import Image
    import fourier_feature_nets as ffn
    model_path, tree_path = str(tmp_path / "voxels.pt"), str(tmp_path / "tree.npz")
    baked_path, out_dir = str(tmp_path / "baked.npz"), str(tmp_path / "frames")
    opaque_ball().save(model_path)
    ffn.OcTree.build_from_model(opaque_ball().to("cuda"), 4).save(tree_path)

    def run(script, *args):
        res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + list(args),
                             capture_output=True, text=True, cwd=ROOT)
        assert res.returncode == 0, res.stderr[-2000:]
        return res.stdout.splitlines()

    lines = run("bake_octree.py", tree_path, model_path, baked_path, "--sh-degree", "2",
                "--num-views", "20", "--batch-size", "50")
    with np.load(baked_path) as baked, np.load(tree_path) as tree:
        assert np.array_equal(baked["leaf_index"], tree["leaf_index"])
        assert int(baked["sh_degree"]) == 2 and baked["sh_degree"].dtype == np.int32
        data = baked["leaf_data"]
        assert data.shape == (len(tree["leaf_index"]), 28) and data.dtype == np.float32
    told = [line for line in lines if line.endswith("leaves baked")]
    assert len(told) == 1 and int(told[0].split()[0]) == len(data)
    density = [line for line in lines if line.startswith("density min")]
    assert len(density) == 1
    assert np.isclose(float(density[0].split()[6]), data[:, -1].max(), rtol=1e-5)
    lines = run("render_octree.py", baked_path, SCENE, out_dir, "--split", "train",
                "--num-cameras", "2", "--mode", "volume")
    with np.load(SCENE) as scene:
        height, width = scene["images"].shape[1:3]
    for camera in range(2):
        with Image.open(os.path.join(out_dir, "frame_%05d.png" % camera)) as image:
            assert image.size == (width, height) and image.mode == "RGB"
            assert np.asarray(image).max() > 0
    assert len([line for line in lines if line.startswith("camera ")]) == 2
