"""K26 on the GPU (``ops.octree_focus_sample`` / ``OcTree.focus_samples`` /
``RaySampler.focus_on_octree``) against the float64 restatement of its contract
(tests/octree_focus_reference.py on the crossings of tests/octree_walk_reference.py): the budget
checks (i), (ii) and the mass, the fall-back and the merge bit for bit, repeatability, plain against
SH rows, the centre, the exact lattice case, ``u == 1`` and NaN targets, the refused arguments, and
the sampler end to end on the 16 x 16 golden scene.  The scenes and their restatements are shared
with tests/test_octree_focus_cpu.py, which shows on the CPU that the budgets can be met and that no
ray is undecided."""

import contextlib
import io
import os

import numpy as np
import pytest
import torch

from tests import octree_focus_reference as fref
from tests.octree_focus_helpers import (MIN_MASS, SCENES, hand_rays, reference, scene, targets,
                                        uniform_samples)
from tests.octree_lattice_helpers import grid_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE16 = os.path.join(ROOT, "tests", "golden", "scene16.npz")


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def bits(x):
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def quiet(fn, *args, **kwargs):
    with contextlib.redirect_stdout(io.StringIO()):
        return fn(*args, **kwargs)


def run(s, index, u, uniform=None, n_uniform=None, center=None, rows=None, stride=4, offset=3,
        starts=None, min_mass=MIN_MASS):
    """One K26 call on scene ``s`` for the batch ``index`` -> t (R,S), mass (R,) as numpy."""
    from fourier_feature_nets_amd import ops
    d = dev()
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)       # noqa: E731
    t, mass = ops.octree_focus_sample(
        put(s["starts"] if starts is None else starts), put(s["directions"]),
        put(np.stack([s["near"], s["far"]])), put(np.asarray(index, np.int64)),
        s["center"] if center is None else center, s["scale"], s["depth"], put(s["node_index"]),
        put(s["leaf_index"]), put(s["rows"] if rows is None else rows), stride, offset, put(u),
        None if uniform is None else put(uniform), n_uniform, min_mass, want_mass=True)
    return t.cpu().numpy(), mass.cpu().numpy()


def subset(c, index):
    """The restatement ``c`` of a scene for the batch ``index`` (ids may repeat)."""
    index = np.asarray(index)
    sizes = c["first"][index + 1] - c["first"][index]
    first = np.concatenate([[0], np.cumsum(sizes)])
    take = np.concatenate([np.arange(c["first"][i], c["first"][i + 1]) for i in index]) \
        if sizes.sum() else np.zeros(0, np.int64)
    out = {k: c[k][index] for k in ("mass", "count", "budget_a", "rounding", "slope", "budget")}
    out.update({k: c[k][take] for k in ("t0", "t1", "weight", "before", "e0", "e1")})
    out["first"] = first
    return out


# R at the wave edge; n_focus 1, 2, 3, 64, 128; n_uniform 0, 1, 64; one S = 300 beyond K2d's 256
SHAPES = [(1, 1, 0), (63, 2, 1), (64, 3, 64), (65, 64, 0), (129, 128, 64), (129, 128, 0),
          (64, 236, 64), (65, 1, 1), (1, 128, 64), (63, 3, 0), (129, 64, 1), (129, 2, 64)]


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("rays,n_focus,n_uniform", SHAPES)
def test_budgets_fallback_order_and_merge(name, rays, n_focus, n_uniform):
    s = scene(name)
    _, c = reference(name)
    total = len(s["near"])
    index = (np.arange(rays) * 7 + n_focus) % total              # any ids, some of them twice
    u = targets(rays, n_focus, 1000 + rays + n_focus)
    near, far = s["near"][index], s["far"][index]
    t, mass = run(s, index, u)
    assert t.shape == (rays, n_focus) and t.dtype == np.float32 and mass.shape == (rays,)
    worst = fref.check(subset(c, index), near, far, u, MIN_MASS, t, mass, name)
    print("%s R=%d n_focus=%d: worst |F(t) - u M| / budget %.3f" % (name, rays, n_focus, worst))
    # the same call gives the same bits
    again, mass_again = run(s, index, u)
    assert (bits(t) == bits(again)).all() and (bits(mass) == bits(mass_again)).all()
    if n_uniform:
        # K2a's rows in a wider buffer: only the first n_uniform columns of a row are read
        wide = np.full((rays, n_uniform + 3), np.float32(-7.0))
        wide[:, :n_uniform] = uniform_samples(near, far, n_uniform)
        merged, mass_merged = run(s, index, u, wide, n_uniform)
        assert merged.shape == (rays, n_uniform + n_focus)
        want = np.sort(np.concatenate([wide[:, :n_uniform], t], axis=1), axis=1)
        assert (bits(merged) == bits(want)).all()
        assert (bits(mass_merged) == bits(mass)).all()


def test_hand_case_on_the_device():
    s = scene("hand")
    w, c = reference("hand")
    _, _, _, _, _, names = hand_rays()
    ray = {n: i for i, n in enumerate(names)}
    index = np.arange(len(names))
    u = np.tile(np.float32([0, .25, .5, .75, 1]), (len(names), 1))
    t, mass = run(s, index, u)
    fref.check(c, s["near"], s["far"], u, MIN_MASS, t, mass)
    one = ray["+x through leaf 0, zero components inside their slabs"]
    assert np.allclose(t[one], [.5, .625, .75, .875, 1], atol=2e-7) and t[one, -1] == 1
    assert np.allclose(t[ray["near cuts the leaf"]], [.75, .8125, .875, .9375, 1], atol=2e-7)
    opaque = ray["-x through the opaque leaf"]
    assert mass[opaque] == 1 and (t[opaque] == np.float32([2, 2.125, 2.25, 2.375, 2.5])).all()
    assert (t[ray["far before the first leaf"]] == np.float32(.375) * u[0]).all()
    assert (t[ray["misses the cube, valid near and far"]] == np.float32(.5) + u[0] * np.float32(3.5)).all()
    assert (t[ray["a NaN direction"]] == u[0]).all()
    assert (t[ray["near beyond far"]] == 2).all()
    diag = ray["the diagonal through all three leaves"]
    assert t[diag, -1] == 3                          # u == 1: the t1 of the last taken leaf
    for name in ("a zero component outside its slab", "through two empty octants", "a NaN direction"):
        assert mass[ray[name]] == 0


@pytest.mark.parametrize("name", ["shell", "mixed"])
def test_a_ray_alone_equals_the_ray_in_a_batch(name):
    s = scene(name)
    total = len(s["near"])
    u = targets(total, 64, 77)
    uni = uniform_samples(s["near"], s["far"], 64)
    batch, mass = run(s, np.arange(total), u, uni)
    _, c = reference(name)
    picks = [int(np.argmax(c["count"])), 0, total - 1, int(np.argmin(c["mass"]))]
    for r in picks:
        alone, mass_alone = run(s, [r], u[r:r + 1], uni[r:r + 1])
        assert (bits(alone[0]) == bits(batch[r])).all() and bits(mass_alone)[0] == bits(mass)[r]


@pytest.mark.parametrize("degree", [1, 2])
def test_plain_and_sh_rows_with_the_same_densities_give_the_same_bits(degree):
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    s = scene("shell")
    total = len(s["near"])
    index = np.arange(total)
    u = targets(total, 32, 3)
    plain, mass = run(s, index, u)
    channels = ops.octree_sh_channels(degree)
    data = np.random.default_rng(degree).normal(size=(len(s["rows"]), channels)).astype(np.float32)
    data[:, -1] = s["rows"][:, 3]
    device_rows = ops.octree_sh_device_layout(data, degree)
    sh, mass_sh = run(s, index, u, rows=device_rows, stride=device_rows.shape[1], offset=0)
    assert (bits(sh) == bits(plain)).all() and (bits(mass_sh) == bits(mass)).all()
    # and through the trees themselves
    d = dev()
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)       # noqa: E731
    args = (put(s["starts"]), put(s["directions"]), put(np.stack([s["near"], s["far"]])),
            put(index.astype(np.int64)), put(u))
    tree = ffn.OcTree(s["scale"], s["node_index"], s["leaf_index"], s["rows"])
    tree_sh = ffn.OcTree(s["scale"], s["node_index"], s["leaf_index"], data, sh_degree=degree)
    a, m = tree.focus_samples(*args, center=s["center"], return_mass=True)
    b = tree_sh.focus_samples(*args, center=s["center"])
    assert (bits(a.cpu().numpy()) == bits(plain)).all() and (bits(m.cpu().numpy()) == bits(mass)).all()
    assert (bits(b.cpu().numpy()) == bits(plain)).all()


def test_center_equals_shifted_starts():
    s = scene("planes")
    assert np.abs(s["center"]).max() > 0
    total = len(s["near"])
    index = np.arange(total)
    u = targets(total, 16, 9)
    with_center, mass = run(s, index, u)
    shifted = (s["starts"] - s["center"][None, :]).astype(np.float32)        # torch's `starts - shift`
    zero, mass_zero = run(s, index, u, center=np.zeros(3, np.float32), starts=shifted)
    assert (bits(with_center) == bits(zero)).all() and (bits(mass) == bits(mass_zero)).all()
    assert (mass >= MIN_MASS).sum() > 20


def test_lattice_rays_through_an_opaque_leaf_are_exact():
    """Depth 3, scale 2 (finest side 1): leaf A is the cell (1, 1, 1) of the 4^3 grid, [-1, 0]^3,
    opaque (sigma L >= 200, so expf gives exactly 0 and a = 1); leaf B behind it along +x, the
    cell (2, 1, 1), [0, 1] x [-1, 0]^2.  Lattice rays: every crossing is exact in f32, M = 1, and with
    dyadic targets t = t0 + u (t1 - t0) bit for bit; B receives no sample."""
    nodes, leaves = grid_tree(3, [(2, 1, 1, 1), (2, 2, 1, 1)])
    order = {int(v): k for k, v in enumerate(leaves)}
    from tests.octree_lattice_helpers import cell_id
    rows = np.zeros((2, 4), np.float32)
    rows[order[cell_id(2, 1, 1, 1)], 3] = 400.0          # the shortest chord below is 1 world unit
    rows[order[cell_id(2, 2, 1, 1)], 3] = 1.0
    f32 = np.float32
    # (start, direction, t0, t1) through A, then B
    cases = [([-3, -.5, -.5], [1, 0, 0], 2, 3), ([-3, -.5, -.5], [2, 0, 0], 1, 1.5),
             ([-2, -.5, -1.5], [1, 0, .5], 1, 2), ([-4, -.5, -.5], [.5, 0, 0], 6, 8)]
    s = dict(scale=2.0, depth=3, node_index=nodes, leaf_index=leaves, rows=rows,
             center=np.zeros(3, f32), starts=f32([c[0] for c in cases]),
             directions=f32([c[1] for c in cases]), near=np.zeros(4, f32), far=np.full(4, 16, f32))
    u = np.tile(f32([0, .125, .25, .5, .75, .875, 1]), (4, 1))
    t, mass = run(s, np.arange(4), u)
    for r, (_, _, t0, t1) in enumerate(cases):
        want = f32(t0) + u[r] * f32(t1 - t0)
        assert (bits(t[r]) == bits(want)).all(), (r, t[r], want)
        assert t[r].max() == t1                          # nothing in the leaf behind
    assert (mass == 1).all()
    # the restatement agrees (and its f32 list gives the same bits)
    from tests import octree_walk_reference as wref
    w = wref.walk(2.0, nodes, leaves, s["starts"], s["directions"])
    c = fref.cdf(w, 2.0, s["starts"], s["directions"], s["near"], s["far"], rows[:, 3])
    fref.check(c, s["near"], s["far"], u, MIN_MASS, t, mass)
    t32, mass32 = fref.focus32(w, s["directions"], s["near"], s["far"], rows[:, 3], u, MIN_MASS)
    assert (bits(t32) == bits(t)).all() and (bits(mass32) == bits(mass)).all()


def test_u_of_one_and_nan_targets():
    s = scene("hand")
    _, _, _, _, _, names = hand_rays()
    ray = {n: i for i, n in enumerate(names)}
    inside = ray["a start inside the cube"]              # leaves end at t 0.5, 1, 1.5 (opaque last)
    one = ray["+x through leaf 0, zero components inside their slabs"]
    miss = ray["misses the cube, valid near and far"]
    nan = np.float32(np.nan)
    u = np.float32([[.25, .5, 1, 1], [.25, nan, .75, 1], [0, nan, .5, 1]])
    t, _ = run(s, [inside, one, miss], u)
    # u == 1 lands on the t1 of the last taken leaf
    assert t[0, 2] == 1.5 and t[0, 3] == 1.5
    # a NaN target on a ray with mass: it and what follows land on the end of the mass, in the row
    assert np.isfinite(t[1]).all() and (np.diff(t[1]) >= 0).all()
    assert (t[1, 1:] == 1).all() and .5 <= t[1, 0] <= 1
    # on the fall-back the NaN stays in the row, the others are what they are without it
    want = np.float32(.5) + u[2] * np.float32(3.5)
    assert np.isnan(t[2, 1]) and (bits(t[2, [0, 2, 3]]) == bits(want[[0, 2, 3]])).all()
    # with uniform samples too: S entries, every finite one inside [near, far], nothing beyond the row
    uni = uniform_samples(s["near"][[inside, one, miss]], s["far"][[inside, one, miss]], 3)
    guard = np.full((3, 3 + 5), np.float32(-7.0))
    guard[:, :3] = uni
    merged, _ = run(s, [inside, one, miss], u, guard, 3)
    assert merged.shape == (3, 7)
    assert (bits(merged[:2]) == bits(np.sort(np.concatenate([uni[:2], t[:2]], 1), 1))).all()
    assert np.isnan(merged[2]).sum() == 1
    assert (np.sort(merged[2][~np.isnan(merged[2])]) ==
            np.sort(np.concatenate([uni[2], t[2][~np.isnan(t[2])]]))).all()


def test_targets_out_of_order_stay_inside_the_row():
    s = scene("shell")
    total = len(s["near"])
    u = np.random.default_rng(4).random((total, 9), dtype=np.float32)         # not sorted
    uni = uniform_samples(s["near"], s["far"], 4)
    d = dev()
    from fourier_feature_nets_amd import ops
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)       # noqa: E731
    t = ops.octree_focus_sample(
        put(s["starts"]), put(s["directions"]), put(np.stack([s["near"], s["far"]])),
        put(np.arange(total, dtype=np.int64)), s["center"], s["scale"], s["depth"],
        put(s["node_index"]), put(s["leaf_index"]), put(s["rows"]), 4, 3, put(u), put(uni))
    t = t.cpu().numpy()
    assert t.shape == (total, 13) and np.isfinite(t).all()
    assert (t >= s["near"][:, None]).all() and (t <= s["far"][:, None]).all()
    _, c = reference("shell")
    with_mass = c["mass"] >= MIN_MASS
    for r in np.nonzero(with_mass)[0]:
        # every value is a uniform sample or lies in a taken leaf
        mine = ~np.isin(bits(t[r]), bits(uni[r]))
        assert fref.inside_taken(c, r, t[r][mine]).all()


def test_refused_arguments_write_nothing():
    from fourier_feature_nets_amd import ops
    from fourier_feature_nets_amd._lib import FfnError, c_f, c_i, c_i64
    s = scene("hand")
    d = dev()
    put = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)       # noqa: E731
    n = len(s["near"])
    starts, dirs, nf = put(s["starts"]), put(s["directions"]), put(np.stack([s["near"], s["far"]]))
    index = put(np.arange(n, dtype=np.int64))
    nodes, leaves, rows = put(s["node_index"]), put(s["leaf_index"]), put(s["rows"])
    u = put(targets(n, 4, 1))
    uni = put(uniform_samples(s["near"], s["far"], 4))
    out = torch.full((n, 8), -7.0, dtype=torch.float32, device=d)
    mass = torch.full((n,), -7.0, dtype=torch.float32, device=d)
    null = ops._dev(None)

    def call(**change):
        a = dict(starts=ops._dev(starts), directions=ops._dev(dirs), near_far=ops._dev(nf),
                 total=c_i64(n), index=ops._dev(index, torch.int64), rays=c_i(n), cx=c_f(0),
                 cy=c_f(0), cz=c_f(0), scale=c_f(s["scale"]), depth=c_i(s["depth"]),
                 nodes=ops._dev(nodes, torch.int64), num_nodes=c_i64(nodes.numel()),
                 leaves=ops._dev(leaves, torch.int64), num_leaves=c_i64(leaves.numel()),
                 rows=ops._dev(rows), stride=c_i(4), offset=c_i(3), u=ops._dev(u), n_focus=c_i(4),
                 uni=ops._dev(uni), uni_stride=c_i(4), n_uniform=c_i(4), min_mass=c_f(1e-3),
                 out=ops._dev(out), mass=ops._dev(mass))
        a.update(change)
        return ops._call("ffn_octree_focus_sample", *a.values())

    bad = [("n_focus", dict(n_focus=c_i(0))),
           ("t_uniform", dict(uni=null)),
           ("alias", dict(out=ops._dev(uni))),
           ("sigma_offset", dict(offset=c_i(4))),
           ("depth", dict(depth=c_i(0))),
           ("depth", dict(depth=c_i(ops.octree_max_depth() + 1))),
           ("2^31", dict(rays=c_i(1 << 28))),
           ("min_mass", dict(min_mass=c_f(float("nan")))),
           ("min_mass", dict(min_mass=c_f(-1.0)))]
    for word, change in bad:
        with pytest.raises(FfnError, match="ffn_octree_focus_sample") as err:
            call(**change)
        assert word in str(err.value), (word, str(err.value))
    torch.cuda.synchronize()
    assert (out == -7.0).all() and (mass == -7.0).all()
    assert (uni.cpu().numpy() == uniform_samples(s["near"], s["far"], 4)).all()
    call()                                               # the good call goes through
    torch.cuda.synchronize()
    assert (out != -7.0).all() and (mass != -7.0).all()
    # the Python layers refuse what they can see
    tree_args = (starts, dirs, nf, index, s["center"], s["scale"], s["depth"], nodes, leaves, rows)
    with pytest.raises(ValueError, match="sigma_offset"):
        ops.octree_focus_sample(*tree_args, 4, 4, u)
    with pytest.raises(ValueError, match="n_focus"):
        ops.octree_focus_sample(*tree_args, 4, 3, u[:, :0])
    with pytest.raises(ValueError, match="min_mass"):
        ops.octree_focus_sample(*tree_args, 4, 3, u, min_mass=float("nan"))


# ------------------------------------------------------------------------------ end to end
def carved_tree(dataset):
    import fourier_feature_nets as ffn
    lo = dataset.sampler.bounds_min[0]
    hi = dataset.sampler.bounds_max[0]
    center = tuple(float(v) for v in (lo + hi) / 2)
    scale = float((hi - lo).max()) / 2
    tree = ffn.OcTree.build_from_silhouettes(dataset, 4, center, scale, min_views=1)
    return tree, center


def test_sampler_end_to_end_on_the_golden_scene(golden):
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd.caster import TrainEngine
    from tests.test_pipeline_gpu import _small_model
    torch.manual_seed(5)
    np.random.seed(5)
    model = _small_model(golden("training"))
    train = quiet(ffn.ImageDataset.load, SCENE16, "train", 16, True, True, device=dev())
    val = quiet(ffn.ImageDataset.load, SCENE16, "val", 16, True, False, device=dev())
    plain = train.sampler
    index = plain._valid_for_camera(0)[:100].contiguous()

    # a sampler without a tree gives the bits it gave before, in the same process: K2a alone
    torch.manual_seed(11)
    before = plain.sample_t(index, None)
    torch.manual_seed(11)
    noise = plain._noise(index.shape[0], 16)
    from fourier_feature_nets_amd import ops
    k2a = ops.sample_t(plain.near_far, index, 16, plain._unit(16), noise, None)
    assert torch.equal(before, k2a)

    tree, center = carved_tree(train)
    assert tree.num_leaves > 1 and tree.leaf_data().shape[1] == 4
    focused = plain.focus_on_octree(tree, center)
    assert focused is not plain and focused.focus_sampling and focused.opacity_model is None
    assert focused.cdfs is None and focused.focus_tree is tree
    assert focused.focus_tree_center == center and focused.focus_min_mass == 1e-3
    assert focused.starts is plain.starts and focused.near_far is plain.near_far
    assert plain.focus_tree is None and not plain.focus_sampling
    t = focused.sample_t(index, None)
    assert t.shape == (100, 16) and torch.isfinite(t).all() and (t[:, 1:] >= t[:, :-1]).all()
    assert (t >= plain.near_far[0][index][:, None]).all()        # (K2a's jitter may pass far)
    mass = focused.focus_mass(index)
    assert mass.shape == (100,) and (mass >= 1e-3).any()
    # the plain sampler, after all that, still gives its bits
    torch.manual_seed(11)
    assert torch.equal(plain.sample_t(index, None), before)
    # composes with clip_to_octree in either order
    a = quiet(plain.clip_to_octree, tree, center).focus_on_octree(tree, center)
    b = quiet(plain.focus_on_octree(tree, center).clip_to_octree, tree, center)
    assert a.focus_tree is tree and b.focus_tree is tree and torch.equal(a.near_far, b.near_far)
    keep = a.valid_index(index)
    if keep.numel():
        torch.manual_seed(3)
        ta = a.sample_t(keep, None)
        torch.manual_seed(3)
        assert torch.equal(ta, b.sample_t(keep, None))
    # two sources of one distribution are refused
    with_model = quiet(ffn.RaySampler, plain.bounds, plain.cameras, 16, False, model, device=dev(),
                       focus_mode="live")
    with pytest.raises(ValueError, match="opacity_model"):
        with_model.focus_on_octree(tree, center)

    # render_rays, a 4-step fit, sample_cameras and the prefetch
    train.sampler = focused
    val.sampler = val.sampler.focus_on_octree(tree, center)
    caster = ffn.Raycaster(model)
    out = caster.render_rays(val.sampler, val.sampler._valid_for_camera(0))
    assert torch.isfinite(out.color).all() and torch.isfinite(out.alpha).all()
    sub = quiet(train.sample_cameras, val.num_cameras, val.num_samples, False)
    assert sub.sampler.focus_tree is tree and sub.sampler.focus_tree_center == center
    assert sub.sampler.focus_min_mass == focused.focus_min_mass and sub.sampler.focus_sampling
    log = quiet(caster.fit, train, val, 64, 5e-4, 4, 0, 4, 0.1, 25000, 0.0, [])
    assert all(np.isfinite(e.val_psnr) and np.isfinite(e.train_psnr) for e in log)
    assert caster.engine._can_prefetch(focused)
    assert isinstance(caster.engine, TrainEngine)
