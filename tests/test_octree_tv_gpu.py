"""K20 on the GPU: the face adjacency (``OcTree.neighbors``), the plan, the Charbonnier energy and
its per-leaf gradient (``ops.octree_tv``) and the ``tv_weight`` of the fit loops against the float64 /
pure-Python restatement (tests/octree_tv_reference.py).  Every leaf's row is held against its budget,
derived in the restatement.  No reference file is read."""

import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_tv_reference as tref
from tests.octree_lattice_helpers import grid_tree, level_cells, mixed_tree
from tests.octree_render_helpers import SCENE, TREES as GOLDEN_TREES, big_cloud, load_tree
from tests.octree_sh_helpers import SIZES, eight_leaves, mixed_depth4
from tests.octree_volume_helpers import hand_case
from tests.octree_walk_helpers import opaque_ball, two_level_tree

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPSILONS = [1e-3, 1e-1]
STRIDES = [4, 16, 28]


def bits(x):
    if torch.is_tensor(x):
        x = x.detach().cpu().numpy()
    return np.ascontiguousarray(x, np.float32).view(np.uint32)


def cuda(x, dtype=np.float32):
    return torch.from_numpy(np.ascontiguousarray(x, dtype)).cuda()


def bare_tree(scale, nodes, leaves):
    import fourier_feature_nets as ffn
    tree = ffn.OcTree(float(scale), nodes, leaves)
    tree._device = torch.device("cuda")
    return tree


def root_only():
    return np.float32(1.0), np.zeros(0, np.int64), np.array([0], np.int64)


def isolated_pair():
    """Leaves 1 and 5 touch across x; 65 and 72 touch nothing: rows without an incidence among rows
    with one."""
    nodes, leaves = grid_tree(3, [(1, 0, 0, 0), (1, 1, 0, 0), (2, 2, 2, 2), (2, 3, 3, 3)])
    return np.float32(1.0), nodes, leaves


def truncated_grid(count):
    """The first ``count`` cells of the 16^3 grid as leaves (the rest of the cube is empty)."""
    nodes, leaves = grid_tree(5, level_cells(4)[:count])
    return np.float32(1.0), nodes, leaves


def skew_tree():
    """Octant 0 a level-1 leaf; octants 4, 2 and 1, its +x, +y and +z neighbours, full level-5 grids:
    the coarse leaf has 3 * 256 incidences, every other leaf at most six."""
    side = 16
    codes = [(1, 0, 0, 0)]
    for ox, oy, oz in ((1, 0, 0), (0, 1, 0), (0, 0, 1)):
        cells = level_cells(4)
        cells[:, 0] = 5
        cells[:, 1:] += np.array([ox, oy, oz]) * side
        codes += cells.tolist()
    nodes, leaves = grid_tree(6, codes)
    return np.float32(1.0), nodes, leaves


@functools.lru_cache(maxsize=None)
def cloud_tree():
    import fourier_feature_nets as ffn
    depth = 6
    tree = ffn.OcTree.build_from_samples(torch.from_numpy(big_cloud(depth)).cuda(), depth, 4)
    state = tree.state_dict
    return np.float32(state["scale"]), state["node_index"], state["leaf_index"]


def golden_tree(name):
    state = load_tree(name).state_dict
    return np.float32(state["scale"]), state["node_index"], state["leaf_index"]


STRUCTURES = dict(eight=eight_leaves, mixed4=mixed_depth4, two_level=two_level_tree,
                  root_only=root_only, cloud6=cloud_tree, mixed5=mixed_tree, isolated=isolated_pair,
                  skew=skew_tree)
for _name in GOLDEN_TREES:
    STRUCTURES["golden_" + _name] = functools.partial(golden_tree, _name)
for _count in SIZES:
    STRUCTURES["grid_%d" % _count] = functools.partial(truncated_grid, _count)


@functools.lru_cache(maxsize=None)
def structure(name):
    """-> scale, node_index, leaf_index, the restatement's neighbours and edges (computed once)."""
    scale, nodes, leaves = STRUCTURES[name]()
    nb, edge_list = tref.tree_edges(nodes, leaves)
    return scale, nodes, leaves, nb, edge_list


def random_rows(leaves, stride, seed):
    return np.random.default_rng(seed).normal(size=(leaves, stride)).astype(np.float32)


def weight_vector(stride):
    """Some columns carry weight 0: the green column of a plain row, the higher bands and the padding
    of an SH row."""
    from fourier_feature_nets_amd import ops
    if stride == 4:
        return np.float32([1.0, 0.0, 0.5, 2.0])
    return ops.octree_tv_weights((1.0, 0.0, 2.0), stride, {16: 1, 28: 2}[stride])


def check_against_restatement(name, stride, eps, seed=3):
    from fourier_feature_nets_amd import ops
    scale, nodes, leaves, nb, edge_list = structure(name)
    tree = bare_tree(scale, nodes, leaves)
    plan = tree._tv_plan()
    assert plan.num_edges == len(edge_list) and plan.num_leaves == len(leaves)
    assert np.array_equal(torch.stack([plan.edge_i, plan.edge_j], 1).cpu().numpy(), edge_list)
    rows = random_rows(len(leaves), stride, seed)
    lam = weight_vector(stride)
    want = tref.total_variation(rows, edge_list, lam, eps)
    assert plan.longest == int(want["incidences"].max())
    value, grad = ops.octree_tv(cuda(rows), plan, lam, eps)
    value, grad = float(value.item()), grad.cpu().numpy()
    err = np.abs(grad.astype(np.float64) - want["grad"])
    worst = float((err / np.maximum(want["budget"], 1e-300)).max()) if err.any() else 0.0
    print("%s stride %d eps %g: L %d, E %d, longest list %d; R %.9g (restatement %.9g, off by %.3g of "
          "a budget of %.3g); worst row entry at %.3g of its budget"
          % (name, stride, eps, len(leaves), len(edge_list), plan.longest, value, want["value"],
             abs(value - want["value"]), want["value_budget"], worst))
    assert abs(value - want["value"]) <= want["value_budget"]
    assert (err <= want["budget"]).all()
    assert not bits(grad[:, lam == 0]).any()                     # exactly +0
    assert not bits(grad[want["incidences"] == 0]).any()
    return tree, plan, rows, lam, want, value, grad


# ------------------------------------------------------------------------------- adjacency
@pytest.mark.parametrize("name", ["golden_" + n for n in GOLDEN_TREES] +
                         ["eight", "mixed4", "two_level", "root_only", "cloud6"])
def test_neighbors_equal_the_restatement(name):
    scale, nodes, leaves, nb, edge_list = structure(name)
    tree = bare_tree(scale, nodes, leaves)
    got = tree.neighbors()
    assert got.dtype == np.int64 and got.shape == (len(leaves), 6)
    assert np.array_equal(got, nb)
    assert tree.neighbors() is got                                # cached
    if name == "root_only":
        assert (got == -1).all()
    if name == "cloud6":
        level = tref.levels(leaves)
        assert len(set(level.tolist())) >= 3 and (level[edge_list[:, 0]] > level[edge_list[:, 1]]).any()
    print("%s: %d leaves, %d edges" % (name, len(leaves), len(edge_list)))


@pytest.mark.parametrize("count", SIZES)
def test_sizes(count):
    name = "grid_%d" % count
    scale, nodes, leaves, nb, _ = structure(name)
    assert len(leaves) == count
    assert np.array_equal(bare_tree(scale, nodes, leaves).neighbors(), nb)
    check_against_restatement(name, 4, 1e-1)
    check_against_restatement(name, 28, 1e-3)


def test_skew_case():
    scale, nodes, leaves, nb, edge_list = structure("skew")
    assert len(leaves) == 1 + 3 * 4096 and leaves[0] == 1
    assert len(edge_list) == 3 * 11520 + 768
    tree, plan, rows, lam, want, value, grad = check_against_restatement("skew", 4, 1e-1)
    assert np.array_equal(tree.neighbors(), nb)
    assert want["incidences"][0] == 768 and plan.longest == 768          # three levels of 16
    assert (want["incidences"][1:] <= 6).all()
    coarse = np.abs(grad[0].astype(np.float64) - want["grad"][0])
    print("skew: the coarse leaf's row", grad[0], "restatement", want["grad"][0], "error", coarse,
          "budget", want["budget"][0])
    assert (coarse <= want["budget"][0]).all() and want["grad"][0, [0, 2, 3]].all()
    check_against_restatement("skew", 16, 1e-3)


# ------------------------------------------------------------------------------- values
@pytest.mark.parametrize("eps", EPSILONS)
@pytest.mark.parametrize("stride", STRIDES)
def test_values(stride, eps):
    from fourier_feature_nets_amd import ops
    tree, plan, rows, lam, want, value, grad = check_against_restatement("mixed5", stride, eps)
    assert (want["incidences"] > 16).any()                      # more than one run of a leaf
    dev_rows = cuda(rows)
    # two calls: equal bits
    value2, grad2 = ops.octree_tv(dev_rows, plan, lam, eps)
    assert np.array_equal(bits(grad2), bits(grad)) and bits(value2) == bits(np.float32(value))
    # accumulate: the prior content plus the sum, one add per element
    prior = random_rows(len(rows), stride, 77)
    out = cuda(prior)
    value3, back = ops.octree_tv(dev_rows, plan, lam, eps, out, accumulate=True)
    assert back is out and bits(value3) == bits(np.float32(value))
    expect = prior.astype(np.float64) + grad.astype(np.float64)
    assert (np.abs(out.cpu().numpy().astype(np.float64) - expect)
            <= np.spacing(np.abs(expect).astype(np.float32))).all()
    # without accumulate a d_rows passed in is overwritten
    out = cuda(prior)
    ops.octree_tv(dev_rows, plan, lam, eps, out)
    assert np.array_equal(bits(out), bits(grad))
    # identical rows: nothing to smooth
    same = np.tile(random_rows(1, stride, 5), (len(rows), 1))
    value0, grad0 = ops.octree_tv(cuda(same), plan, lam, eps)
    assert float(value0.item()) == 0.0 and not bits(grad0).any()


@pytest.mark.parametrize("name", ["isolated", "two_level", "root_only", "mixed4"])
def test_rows_without_an_incidence(name):
    tree, plan, rows, lam, want, value, grad = check_against_restatement(name, 4, 1e-1)
    if name in ("two_level", "root_only"):
        assert plan.num_edges == 0 and value == 0.0 and not bits(grad).any()
        prior = cuda(random_rows(len(rows), 4, 9))
        from fourier_feature_nets_amd import ops
        ops.octree_tv(cuda(rows), plan, lam, 1e-1, prior, accumulate=True)
        assert np.array_equal(bits(prior), bits(random_rows(len(rows), 4, 9)))
    if name == "isolated":
        assert want["incidences"].tolist() == [1, 1, 0, 0] and grad[:2, 0].all()


def test_total_variation_of_a_tree():
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import ops
    scale, nodes, leaves, _, edge_list = structure("mixed4")
    data = np.abs(random_rows(len(leaves), 4, 21))
    tree = ffn.OcTree(float(scale), nodes, leaves, data)
    want = tref.total_variation(data, edge_list, np.float32([2, 2, 2, 0.5]), 1e-2)
    got = tree.total_variation((2, 0.5))
    assert abs(got - want["value"]) <= want["value_budget"]
    ones = tref.total_variation(data, edge_list, np.ones(4, np.float32), 1e-2)
    assert abs(tree.total_variation() - ones["value"]) <= ones["value_budget"]
    # an SH tree: the file layout goes through the device layout
    sh = np.random.default_rng(8).normal(size=(len(leaves), 13)).astype(np.float32)
    sh[:, -1] = np.abs(sh[:, -1])
    sh_tree = ffn.OcTree(float(scale), nodes, leaves, sh, sh_degree=1)
    lam = ops.octree_tv_weights((1, 0.25, 3), 16, 1)
    want = tref.total_variation(ops.octree_sh_device_layout(sh, 1), edge_list, lam, 0.05)
    got = sh_tree.total_variation((1, 0.25, 3), eps=0.05)
    assert abs(got - want["value"]) <= want["value_budget"] and got > 0
    with pytest.raises(ValueError, match="leaf_data"):
        ffn.OcTree(float(scale), nodes, leaves).total_variation()


# ------------------------------------------------------------------------------- refusals
def test_refusals():
    from fourier_feature_nets_amd import ops
    scale, nodes, leaves, _, _ = structure("mixed4")
    plan = bare_tree(scale, nodes, leaves)._tv_plan()
    count = len(leaves)
    rows = cuda(random_rows(count, 4, 1))
    lam = np.ones(4, np.float32)
    with pytest.raises(ValueError, match="stride"):
        ops.octree_tv(cuda(random_rows(count, 6, 1)), plan, np.ones(6, np.float32), 0.01)
    shifted = torch.zeros((count * 4 + 1,), dtype=torch.float32, device="cuda")[1:].view(count, 4)
    assert shifted.is_contiguous() and shifted.data_ptr() % 16 != 0
    with pytest.raises(ValueError, match="aligned"):
        ops.octree_tv(shifted, plan, lam, 0.01)
    with pytest.raises(ValueError, match="aligned"):
        ops.octree_tv(rows, plan, lam, 0.01, shifted)
    for eps in (0.0, -0.01, float("nan")):
        with pytest.raises(ValueError, match="eps"):
            ops.octree_tv(rows, plan, lam, eps)
    for bad in (np.float32([1, np.nan, 1, 1]), np.float32([1, 1, -1, 1]), np.ones(5, np.float32)):
        with pytest.raises(ValueError, match="weights"):
            ops.octree_tv(rows, plan, bad, 0.01)
    other = structure("eight")
    with pytest.raises(ValueError, match="plan"):
        ops.octree_tv(rows, bare_tree(*other[:3])._tv_plan(), lam, 0.01)
    with pytest.raises(ValueError, match="accumulate"):
        ops.octree_tv(rows, plan, lam, 0.01, None, accumulate=True)


# ------------------------------------------------------------------------------- wiring
@functools.lru_cache(maxsize=None)
def scene():
    """scene16's training images and a small density tree of the opaque ball (depth 4), plain and
    with SH leaves of degree 1."""
    import fourier_feature_nets as ffn
    model = opaque_ball().to("cuda")
    dataset = ffn.ImageDataset.load(SCENE, "train", 64, True, False, None, device="cuda")
    tree = ffn.OcTree.build_from_model(model, 4)
    assert 8 < tree.num_leaves < 4096 and tree._tv_plan().num_edges > 0
    return dataset, tree, tree.bake_sh(model, 1, 8)


def fitters(kind):
    import fourier_feature_nets as ffn
    dataset, plain, sh = scene()
    if kind == "plain":
        return dataset, plain, ffn.fit_octree, ffn.OctreeField, (0.0, 0.0), (0.5, 0.25)
    return dataset, sh, ffn.fit_octree_sh, ffn.OctreeSHField, (0.0, 0.0, 0.0), (0.5, 0.125, 0.25)


@pytest.mark.parametrize("kind", ["plain", "sh"])
def test_zero_weight_is_todays_fit(kind):
    dataset, tree, fit, _, zero, _ = fitters(kind)
    kwargs = dict(num_steps=12, report_interval=5, verbose=False)
    fitted, log = fit(tree, dataset, dataset, 1024, **kwargs)
    again, log2 = fit(tree, dataset, dataset, 1024, tv_weight=zero, tv_eps=0.5, **kwargs)
    assert np.array_equal(bits(again.leaf_data()), bits(fitted.leaf_data()))
    assert np.array_equal(bits([e.loss for e in log2]), bits([e.loss for e in log]))
    assert np.array_equal(bits([e.val_psnr for e in log2]), bits([e.val_psnr for e in log]))
    assert not np.array_equal(bits(fitted.leaf_data()), bits(tree.leaf_data()))
    with pytest.raises(ValueError, match="weights"):
        fit(tree, dataset, None, 1024, num_steps=1, verbose=False, tv_weight=(1.0,))
    with pytest.raises(ValueError, match="eps"):
        fit(tree, dataset, None, 1024, num_steps=1, verbose=False, tv_weight=zero, tv_eps=0.0)


@pytest.mark.parametrize("kind", ["plain", "sh"])
def test_one_step_is_the_hand_composition(kind):
    from fourier_feature_nets_amd import octree_fit, ops
    dataset, tree, fit, field_type, _, weight = fitters(kind)
    batch, eps, seed = 1024, 0.02, 11
    fitted, log = fit(tree, dataset, None, batch, num_steps=1, verbose=False, seed=seed,
                      tv_weight=weight, tv_eps=eps)
    plain, _ = fit(tree, dataset, None, batch, num_steps=1, verbose=False, seed=seed)
    sampler = dataset.sampler
    dev = sampler.starts.device
    field = field_type(tree, tree.center, dev)
    data = field.data.detach()
    flat = data.view(-1)
    grads = torch.empty_like(data)
    exp_avg, exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
    generator = torch.Generator(device=dev)
    generator.manual_seed(seed)
    rays = torch.randperm(sampler.num_cameras * sampler.rays_per_camera, generator=generator,
                          device=dev)[:batch]
    count = int(rays.numel())
    shift = torch.tensor(field.center, dtype=torch.float32, device=dev)
    starts = (sampler.starts[rays] - shift).contiguous()
    directions = sampler.directions[rays].contiguous()
    color, alpha, _ = field._render(data, starts, directions, 0.0, (0.0, 0.0, 0.0), 0.0)
    alphas = dataset._gt_alphas()
    aw = float(dataset.alpha_weight) if alphas is not None else 0.0
    sums, d_color, d_alpha = ops.mse_loss(color, alpha, dataset.colors, alphas, rays,
                                          1.0 / (3 * count), aw / count)
    field.backward(starts, directions, d_color, d_alpha, 0.0, (0.0, 0.0, 0.0), 0.0, data=data,
                   out=grads)
    data_term = grads.clone()
    field.tv_backward(weight, eps, data=data, out=grads, accumulate=True)
    assert not torch.equal(grads, data_term)
    ops.clip_adam(flat, grads.view(-1), exp_avg, exp_avg_sq, 1, octree_fit.LEARNING_RATE,
                  clip_value=octree_fit.CLIP_VALUE, max_norm=octree_fit.MAX_NORM,
                  scratch=torch.empty(((flat.numel() + 1023) // 1024,), dtype=torch.float32,
                                      device=dev))
    field._project(data)
    assert np.array_equal(bits(field.tree().leaf_data()), bits(fitted.leaf_data()))
    assert not np.array_equal(bits(plain.leaf_data()), bits(fitted.leaf_data()))
    # the logged loss is the data term
    assert bits([log[0].loss]) == bits(ops.loss_value(sums, count, aw))
    # the field's energy is the tree's
    tv = float(field.total_variation(None, eps).item())
    assert tv == field.tree().total_variation(None, eps) and tv > 0


def test_the_prior_smooths():
    import fourier_feature_nets as ffn
    dataset, tree, _ = scene()
    kwargs = dict(num_steps=50, report_interval=50, verbose=False)
    off, _ = ffn.fit_octree(tree, dataset, None, 1024, **kwargs)
    on, _ = ffn.fit_octree(tree, dataset, None, 1024, tv_weight=(1.0, 1.0), **kwargs)
    print("total variation after 50 steps: %.6g without the prior, %.6g with tv_weight 1 (start %.6g)"
          % (off.total_variation(), on.total_variation(), tree.total_variation()))
    assert on.total_variation() < off.total_variation()


def test_report_lines_carry_the_energy(capsys):
    import fourier_feature_nets as ffn
    dataset, tree, _ = scene()
    ffn.fit_octree(tree, dataset, dataset, 1024, num_steps=2, tv_weight=(0.1, 0.1))
    lines = [line for line in capsys.readouterr().out.splitlines() if "val_psnr" in line]
    assert len(lines) == 2 and all(" tv: " in line for line in lines)
    ffn.fit_octree(tree, dataset, dataset, 1024, num_steps=2)
    assert " tv: " not in capsys.readouterr().out


def test_train_octree_program_with_the_prior(tmp_path):
    import fourier_feature_nets as ffn
    data_path, tree_path, out_path = [str(tmp_path / name) for name in
                                      ("data.npz", "tree.npz", "out.npz")]
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "make_synthetic_npz.py"),
                          data_path, "--size", "8", "--cameras", "4"], capture_output=True,
                         text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    scale, nodes, leaves, data, _, _ = hand_case()
    ffn.OcTree(float(scale), nodes, leaves, data).save(tree_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "train_octree.py"),
                          tree_path, data_path, out_path, "--center", "0", "0", "0", "--steps",
                          "20", "--batch-size", "64", "--tv-weight", "0.1", "0.2", "--tv-eps",
                          "0.05"], capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert "total-variation prior: 0.1 0.2 eps 0.05" in res.stdout and " tv: " in res.stdout
    assert "3 leaves fitted" in res.stdout
    fitted = ffn.OcTree.load(out_path)
    assert np.array_equal(fitted.state_dict["leaf_index"], leaves)
    out = fitted.leaf_data()
    assert out.shape == (3, 4) and out.dtype == np.float32 and not np.array_equal(out, data)
