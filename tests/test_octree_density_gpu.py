"""K16 on the device: the three kernels against the numpy restatement
(tests/octree_density_reference.py) bit for bit, ``OcTree.build_from_model`` against the
restatement fed with the model's own logits, and the density tree against the shell tree of
``build_from_samples`` + ``bake`` as a picture of the model."""

import contextlib
import functools
import io

import numpy as np
import pytest
import torch

from tests import octree_density_reference as dref
from tests.helpers import look_at_camera
from tests.octree_density_helpers import blob_field, hand_cases
from tests.octree_walk_helpers import opaque_ball

pytestmark = pytest.mark.gpu
F = np.float32
CENTER = (0.3, -0.2, 0.1)


def bits(x):
    return np.ascontiguousarray(x, dtype=F).view(np.uint32)


def dev(x, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(x))
    return (t if dtype is None else t.to(dtype)).to("cuda").contiguous()


# ------------------------------------------------------------------------------------ K16a
@pytest.mark.parametrize("depth,first,count", [(1, 0, 1), (2, 0, 8), (2, 3, 4), (4, 37, 300),
                                               (11, 2 ** 30 - 300, 300)])
def test_cell_centers(depth, first, count):
    """A chunk aligned to neither 8 nor 256; a scale whose chain rounds; the last codes of the
    deepest grid (the index arithmetic is 64-bit)."""
    from fourier_feature_nets_amd import ops
    scale = float(F(0.7))
    got = ops.octree_cell_centers(first, count, CENTER, scale, depth, "cuda")
    ids = torch.arange(first, first + count, device="cuda") + dref.first_id(depth - 1)
    chain, depths = ops.octree_leaf_geometry(ids.contiguous(), scale)
    want = chain + torch.tensor(CENTER, dtype=torch.float32, device="cuda")
    assert (depths == depth - 1).all()
    assert np.array_equal(bits(got.cpu().numpy()), bits(want.cpu().numpy()))
    assert np.array_equal(bits(got.cpu().numpy()),
                          bits(dref.cell_centers(first, count, CENTER, scale, depth)))


# ------------------------------------------------------------------------------------ K16b
def seeded_logits(count, kind):
    rng = np.random.default_rng(100 + count)
    logits = rng.normal(size=(count, 4)).astype(F) * F(3)
    if kind == "all":
        logits[:, 3] = np.abs(logits[:, 3]) + F(1)
    elif kind == "none":
        logits[:, 3] = F(-30)
    return logits


@pytest.mark.parametrize("kind", ["mixed", "all", "none", "edge"])
@pytest.mark.parametrize("count", [1, 255, 256, 257, 2049])
def test_density_select(count, kind):
    from fourier_feature_nets_amd import ops
    depth, first = 6, 12345                       # 8^5 = 32768 codes
    side, tau = dref.side_of(1.0, depth), dref.tau_of(0.01)
    logits = seeded_logits(count, "mixed" if kind == "edge" else kind)
    if kind == "edge":
        # sigma > 20 passes through softplus unchanged: a row with sigma * side == tau exactly
        # needs tau / side > 20, so this case has its own (power-of-two) side and threshold
        side, tau = F(2.0 ** -10), F(21 * 2.0 ** -10)
        logits[0] = [0.5, -0.5, 1.0, 21.0]                               # == tau: not kept
        logits[count // 2] = [0.5, -0.5, 1.0, np.nextafter(F(21), F(22))]    # the next f32: kept
        logits[count - 1] = [0.5, np.nan, 1.0, np.nan]                   # NaN: not kept
        if count > 3:
            logits[1] = [np.nan, 0.0, 0.0, 30.0]             # a NaN colour does not decide
    baked = ops.octree_bake(dev(logits)).cpu().numpy()
    want_codes, want_data = dref.select(baked, first, tau, side)
    codes, data = ops.octree_density_select(dev(logits), first, float(tau), float(side), depth)
    assert codes.dtype == torch.int32 and data.dtype == torch.float32
    assert codes.shape[0] == len(want_codes) == data.shape[0]
    assert np.array_equal(codes.cpu().numpy(), want_codes)
    assert np.array_equal(bits(data.cpu().numpy()), bits(want_data))
    kept = want_codes - first
    assert np.array_equal(bits(data.cpu().numpy()), bits(baked[kept]))
    if kind == "all":
        assert len(kept) == count
    if kind == "none":
        assert len(kept) == 0
    if kind == "edge":
        assert 0 not in kept and count - 1 not in kept
        assert count < 3 or count // 2 in kept
        assert count <= 3 or 1 in kept
    if kind == "mixed" and count > 100:
        assert 0 < len(kept) < count
    # numpy's own activations agree to rounding (not bitwise: another exp).  The device is within
    # 4 ulp of the exact value (test_octree_volume_gpu.test_bake); numpy's f32 exp, add and
    # divide / log1p, half an ulp to an ulp each, stay within another 4
    with np.errstate(invalid="ignore"):
        close = np.abs(dref.activate(logits) - baked) <= 8 * np.spacing(np.abs(baked))
    assert (close | np.isnan(baked)).all()


# ------------------------------------------------------------------------------------ K16c
def device_passes(codes, levels, data, depth, tol):
    from fourier_feature_nets_amd import ops
    state = (dev(codes, torch.int32), dev(levels, torch.int32), dev(data))
    passes = []
    for level in range(depth - 1, 0, -1):
        state = ops.octree_merge_level(*state, level, depth, tol[0], tol[1])
        passes.append(tuple(x.cpu().numpy() for x in state))
    return passes


def same_passes(got, want):
    assert len(got) == len(want)
    for (gc, gl, gd), (wc, wl, wd) in zip(got, want):
        assert np.array_equal(gc, wc) and np.array_equal(gl, wl)
        assert np.array_equal(bits(gd), bits(wd))


@pytest.mark.parametrize("name", sorted(hand_cases()))
def test_merge_hand_cases(name):
    case = hand_cases()[name]
    depth = case["depth"]
    codes = np.asarray(case["codes"], np.int32)
    levels = np.full(len(codes), depth - 1, np.int32)
    want = []
    dref.merge(codes, levels, case["data"], depth, *case["tol"], passes=want)
    got = device_passes(codes, levels, case["data"], depth, case["tol"])
    same_passes(got, want)
    nodes, leaves, data = dref.tree(*got[-1], depth)
    assert leaves.tolist() == case["leaves"] and nodes.tolist() == case["nodes"]
    if "mean" in case:
        assert np.array_equal(bits(data[0]), bits(case["mean"]))


@pytest.mark.parametrize("tol", [(0.01, 0.01), (0.0, 0.0), (1.0, 1e9)])
def test_merge_blob_field(tol):
    depth = 5
    field = blob_field(depth)
    codes, data = dref.select(field, 0, dref.tau_of(0.01), dref.side_of(1.0, depth))
    assert len(codes) > 2049                       # more than one scan tile
    levels = np.full(len(codes), depth - 1, np.int32)
    want = []
    dref.merge(codes, levels, data, depth, *tol, passes=want)
    got = device_passes(codes, levels, data, depth, tol)
    same_passes(got, want)
    assert len(want[-1][0]) < len(codes)
    assert len(set(want[-1][1].tolist())) >= 3 or tol[1] > 1
    ids = dref.leaf_ids(*got[-1][:2], depth)
    assert (np.diff(got[-1][0]) > 0).all() and len(np.unique(ids)) == len(ids)


# ------------------------------------------------------------------------------------ the builder
def model_logits(model, depth, center, scale, view=None):
    """The model at the restatement's centres, all cells in code order."""
    points = dev(dref.cell_centers(0, 8 ** (depth - 1), center, scale, depth))
    was = model.training
    model.eval()
    with torch.no_grad():
        if view is None:
            out = model(points)
        else:
            v = torch.tensor(view, dtype=torch.float32, device="cuda")
            out = model(points, v.expand(points.shape[0], 3).contiguous())
    model.train(was)
    return out.reshape(-1, 4).to(torch.float32).contiguous()


def check_tree(tree, model, depth, center, scale, tol, view=None, alpha_threshold=0.01):
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    baked = ops.octree_bake(model_logits(model, depth, center, scale, view)).cpu().numpy()
    nodes, leaves, data = dref.build(baked, depth, scale, alpha_threshold, tol)
    state = tree.state_dict
    assert np.array_equal(state["node_index"], nodes) and np.array_equal(state["leaf_index"], leaves)
    assert state["node_index"].dtype == state["leaf_index"].dtype == np.int64
    got = tree.leaf_data()
    assert got.dtype == F and got.shape == (len(leaves), 4)
    assert np.array_equal(bits(got), bits(data))
    assert tree.scale == float(F(scale)) and tree.point_leaf_ids is None
    assert np.array_equal(F(tree.center), F(center))
    assert np.array_equal(tree.query(tree.leaf_centers()), np.arange(tree.num_leaves))
    again = ffn.OcTree.load(tree.state_dict)
    assert np.array_equal(again.state_dict["leaf_index"], leaves) and again.center is None
    return nodes, leaves, data


@functools.lru_cache(maxsize=None)
def ball():
    return opaque_ball(16).to("cuda")


@pytest.mark.parametrize("tol", [None, (1.0, 1e9)])
def test_build_from_model_on_the_opaque_ball(tol, tmp_path):
    import fourier_feature_nets as ffn
    model, depth = ball(), 5
    model.train()
    tree = ffn.OcTree.build_from_model(model, depth, merge_tolerance=tol)
    assert model.training
    _, leaves, data = check_tree(tree, model, depth, (0, 0, 0), 1.0, tol)
    small = ffn.OcTree.build_from_model(model, depth, merge_tolerance=tol, batch_size=1000)
    for key in ("node_index", "leaf_index"):
        assert np.array_equal(small.state_dict[key], tree.state_dict[key])
    assert np.array_equal(bits(small.leaf_data()), bits(data))
    depths = tree.leaf_depths()
    if tol is None:
        assert (depths == depth - 1).all()
        # the leaves already hold what bake stores
        assert np.array_equal(bits(tree.bake(model).leaf_data()), bits(data))
        assert np.array_equal(bits(tree.bake(model, batch_size=777).leaf_data()), bits(data))
        # the ball of radius 0.45 in the cube of half side 1: about 4.8 % of 4096 cells
        assert 100 < tree.num_leaves < 400
    else:
        assert len(set(depths.tolist())) >= 2 and depths.min() < depth - 1     # the interior merged
        fine = ffn.OcTree.build_from_model(model, depth)
        assert tree.num_leaves < fine.num_leaves
        # re-baking keeps the structure and samples the merged cells at their own centres
        rebaked = tree.bake(model)
        assert np.array_equal(rebaked.state_dict["leaf_index"], leaves)
        at_finest = depths == depth - 1
        assert np.array_equal(bits(rebaked.leaf_data()[at_finest]), bits(data[at_finest]))
    path = str(tmp_path / "density.npz")
    tree.save(path)
    loaded = ffn.OcTree.load(path)
    assert np.array_equal(loaded.state_dict["leaf_index"], leaves)
    assert np.array_equal(bits(loaded.leaf_data()), bits(data))
    with np.load(path) as f:
        assert sorted(f.files) == ["leaf_data", "leaf_index", "node_index", "scale"]
    rng = np.random.default_rng(4)
    o = rng.normal(size=(500, 3)).astype(F)
    o = (o / np.linalg.norm(o, axis=1, keepdims=True) * 3).astype(F)
    d = ((rng.random((500, 3)).astype(F) - F(0.5)) * F(0.6) - o).astype(F)
    out = tree.render_volume(o, d)
    assert np.isfinite(out.color).all() and 0.2 < (out.alpha > 0.99).mean() <= 1.0
    for a, b in zip(out, loaded.render_volume(o, d)):
        assert np.array_equal(bits(a), bits(b))


def test_build_from_model_moved_and_scaled():
    """A cube that is neither centred nor of unit size: the chain rounds, and only part of the
    ball is inside."""
    import fourier_feature_nets as ffn
    model, depth = ball(), 4
    tree = ffn.OcTree.build_from_model(model, depth, center=CENTER, scale=0.35,
                                       alpha_threshold=0.5)
    check_tree(tree, model, depth, CENTER, 0.35, None, alpha_threshold=0.5)
    assert np.array_equal(bits(tree.bake(model).leaf_data()), bits(tree.leaf_data()))
    with pytest.raises(ValueError, match="no leaf"):
        ffn.OcTree.build_from_model(model, 3, center=(0.9, 0.9, 0.9), scale=0.05)
    one = ffn.OcTree.build_from_model(model, 1, scale=0.2)           # the root is the one cell
    assert one.state_dict["leaf_index"].tolist() == [0] and len(one.state_dict["node_index"]) == 0
    full = ffn.OcTree.build_from_model(model, 3, scale=0.2, merge_tolerance=(1.0, 1e9))
    assert full.state_dict["leaf_index"].tolist() == [0]            # 64 -> 8 -> 1


def test_build_from_a_model_with_a_view_direction():
    import fourier_feature_nets as ffn
    torch.manual_seed(5)
    model = ffn.NeRF(4, 64, 4, 4, 2, 4, [2], True).to("cuda")
    assert model.use_view
    view, depth = (0.6, 0.0, 0.8), 4
    tree = ffn.OcTree.build_from_model(model, depth, alpha_threshold=0.0, view=view,
                                       batch_size=200)
    check_tree(tree, model, depth, (0, 0, 0), 1.0, None, view=view, alpha_threshold=0.0)
    assert np.array_equal(bits(tree.bake(model, view=view).leaf_data()), bits(tree.leaf_data()))
    other = tree.bake(model, view=(0.0, 1.0, 0.0)).leaf_data()
    assert not np.array_equal(bits(other[:, :3]), bits(tree.leaf_data()[:, :3]))


# ------------------------------------------------------------------------------------ end to end
def psnr(a, b, mask=None):
    err = (np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2
    if mask is not None:
        err = err[mask]
    return float(-10 * np.log10(max(err.mean(), 1e-12)))


def test_density_tree_shows_the_model_better_than_the_shell_tree():
    """Two 64 x 64 cameras at distance 4, depth 6.  The yardstick is the route there was before:
    the model's surface points (alpha > 0.3) through ``build_from_samples`` and ``bake``, same
    depth, same rays.  The density tree has to be strictly better on the alpha map and on the
    colour where the model is opaque; no absolute figure is fixed."""
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    model, depth, side = ball(), 6, 64
    cams = []
    for k, eye in enumerate([(0.0, 0.0, -4.0), (2.4, 1.6, 2.8)]):
        eye = np.array(eye) * 4 / np.linalg.norm(eye)
        intr, pose = look_at_camera(eye, side, side)
        cams.append(ffn.CameraInfo.create("c%d" % k, ffn.Resolution(side, side), intr, pose))
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        sampler = ffn.RaySampler(bounds, cams, 128, device="cuda")
    caster = ffn.Raycaster(model)
    index = sampler.valid_index(torch.arange(len(sampler), device="cuda"))
    with torch.no_grad():
        color, alpha, depth_map = caster.render(sampler.sample(index, None), True)
    starts, dirs = sampler.starts[index].contiguous(), sampler.directions[index].contiguous()
    positions, kept, count = ops.octree_surface_points(alpha.contiguous(), depth_map.contiguous(),
                                                       starts, dirs, 0.3, color.contiguous())
    count = int(count.item())
    shell = ffn.OcTree.build_from_samples(positions[:count].contiguous(), depth, 1,
                                          kept[:count].contiguous()).bake(model)
    dense = ffn.OcTree.build_from_model(model, depth)
    want_c, want_a = color.cpu().numpy(), alpha.cpu().numpy()
    opaque = want_a >= 0.99
    assert 100 < opaque.sum() < len(want_a) - 100
    figures = {}
    for name, tree in (("shell", shell), ("density", dense)):
        shift = torch.tensor(tree.center, dtype=torch.float32, device="cuda")
        out = tree.render_volume((starts - shift).contiguous(), dirs)
        got_c, got_a = out.color.cpu().numpy(), out.alpha.cpu().numpy()
        figures[name] = (float(np.abs(got_a - want_a).mean()), psnr(got_c, want_c),
                         psnr(got_c, want_c, opaque))
        print("%s tree, %d leaves: mean |alpha diff| %.4f, PSNR all pixels %.2f dB, where the "
              "model is opaque %.2f dB" % ((name, tree.num_leaves) + figures[name]))
    assert figures["density"][0] < figures["shell"][0]
    assert figures["density"][2] > figures["shell"][2]
