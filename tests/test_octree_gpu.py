"""The K12 octree kernels on the GPU: build_from_samples against trees the reference built
(tests/golden/octree.npz) and, on clouds of 1 M and 16 M points, against the numpy restatement
(tests/octree_reference.py); query; surface points of a render batch against the numpy expression
of voxelize_model.py:71-77; prune / save / load; scripts/voxelize_model.py as a program.

Structure (ids, order, scale bits, centres, depths, query answers, surface points) is compared
for EQUALITY.  Leaf means are compared with the float64 mean of the same rows within
(n + 1) * 2^-24 * mean|x| per component, n the leaf's point count: the first-order bound of an
f32 sum of n terms in any order plus the division (tests/test_octree_cpu.py holds the
reference's own f32 means to the same bound)."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import octree_reference as oref
from tests.test_octree_cpu import mean_bound

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SCENE = os.path.join(HERE, "golden", "scene16.npz")
CLOUDS = ["shell", "planes", "tiny", "depth1", "nodata"]


@pytest.fixture(scope="module")
def fixture():
    with np.load(os.path.join(HERE, "golden", "octree.npz")) as g:
        return {k: g[k] for k in g.files}


def cloud(fixture, name):
    return {k.split("/", 1)[1]: v for k, v in fixture.items() if k.startswith(name + "/")}


def build(g):
    import fourier_feature_nets as ffn
    return ffn.OcTree.build_from_samples(g["positions"].copy(), int(g["depth"]),
                                         int(g["min_leaf_size"]), g.get("data"))


def check_means(tree, expect, data):
    got = tree.leaf_data()
    assert got.dtype == np.float32 and got.shape == expect["leaf_data"].shape
    bound = mean_bound(data, expect["point_leaf"], expect["leaf_index"], expect["leaf_count"])
    err = np.abs(got.astype(np.float64) - expect["leaf_data"])
    print("leaf means: max err / bound = %.3f over %d leaves" % ((err / bound).max(), len(got)))
    assert (err <= bound).all()


@pytest.mark.parametrize("name", CLOUDS)
def test_build_equals_the_reference_tree(fixture, name):
    g = cloud(fixture, name)
    before = g["positions"].copy()
    tree = build(g)
    state = tree.state_dict
    assert np.array_equal(state["node_index"], g["node_index"])
    assert np.array_equal(state["leaf_index"], g["leaf_index"])
    assert state["leaf_index"].dtype == np.int64 and state["node_index"].dtype == np.int64
    assert np.float32(state["scale"]).tobytes() == g["scale"].tobytes()
    expect = oref.build(before, int(g["depth"]), int(g["min_leaf_size"]), g.get("data"))
    assert np.array_equal(tree.point_leaf_ids.cpu().numpy(), expect["point_leaf"])
    if "data" in g:
        check_means(tree, expect, g["data"])
    else:
        assert tree.leaf_data() is None and "leaf_data" not in state
    if "leaf_centers" in g:
        assert tree.leaf_centers().tobytes() == g["leaf_centers"].tobytes()
        assert tree.leaf_depths().dtype == np.int32
        assert np.array_equal(tree.leaf_depths(), g["leaf_depths"])
    else:       # the root is the only leaf: reported as itself, with the real scale
        assert np.array_equal(tree.leaf_centers(), np.zeros((1, 3), np.float32))
        assert np.array_equal(tree.leaf_depths(), [0])
        assert tree.query(np.zeros((1, 3), np.float32))[0] == 0
        assert tree.query(np.full((1, 3), 2 * tree.scale, np.float32))[0] == -1
    assert tree.num_leaves == len(g["leaf_index"])
    assert len(tree) == len(g["leaf_index"]) + len(g["node_index"])


def test_device_tensors_in_and_the_callers_array_untouched(fixture):
    import fourier_feature_nets as ffn
    g = cloud(fixture, "shell")
    pos = torch.from_numpy(g["positions"]).cuda()
    data = torch.from_numpy(g["data"]).cuda()
    keep = pos.clone()
    tree = ffn.OcTree.build_from_samples(pos, int(g["depth"]), int(g["min_leaf_size"]), data)
    assert torch.equal(pos, keep)
    assert np.array_equal(tree.state_dict["leaf_index"], g["leaf_index"])
    answers = tree.query(torch.from_numpy(g["query"]).cuda())
    assert torch.is_tensor(answers) and answers.is_cuda and answers.dtype == torch.int64
    assert np.array_equal(answers.cpu().numpy(), g["query_result"])


@pytest.mark.parametrize("depth", list(range(1, 12)))
def test_every_depth_from_1_to_11(depth):
    import fourier_feature_nets as ffn
    rng = np.random.default_rng(depth)
    pos = (rng.normal(size=(30000, 3)) * [1.0, 0.6, 0.3]).astype(np.float32)
    data = rng.random((30000, 2)).astype(np.float32)
    expect = oref.build(pos, depth, 2, data)
    tree = ffn.OcTree.build_from_samples(pos, depth, 2, data)
    assert np.array_equal(tree.state_dict["node_index"], expect["node_index"])
    assert np.array_equal(tree.state_dict["leaf_index"], expect["leaf_index"])
    assert tree.depth <= depth
    check_means(tree, expect, data)


def test_inputs_the_tree_cannot_hold_raise():
    import fourier_feature_nets as ffn
    pos = np.random.default_rng(0).normal(size=(100, 3)).astype(np.float32)
    with pytest.raises(ValueError, match="depth"):
        ffn.OcTree.build_from_samples(pos, 40, 4)
    with pytest.raises(ValueError, match="depth"):
        ffn.OcTree.build_from_samples(pos, 0, 4)
    with pytest.raises(ValueError, match="no leaf"):
        ffn.OcTree.build_from_samples(pos[:3], 1, 4)
    with pytest.raises(ValueError, match="empty"):
        ffn.OcTree.build_from_samples(pos[:0], 4, 4)


@pytest.mark.parametrize("count", [1 << 20, 1 << 24])
def test_large_random_clouds_against_the_restatement(count):
    import fourier_feature_nets as ffn
    rng = np.random.default_rng(count)
    # dense at the centre, sparse towards the faces: leaves at several depths at either size
    pos = (rng.random((count, 3), dtype=np.float32) * np.float32(2) - np.float32(1)) ** 5
    data = rng.random((count, 3), dtype=np.float32)
    expect = oref.build(pos, 8, 4, data)
    dev_pos, dev_data = torch.from_numpy(pos).cuda(), torch.from_numpy(data).cuda()
    tree = ffn.OcTree.build_from_samples(dev_pos, 8, 4, dev_data)
    assert np.array_equal(tree.state_dict["node_index"], expect["node_index"])
    assert np.array_equal(tree.state_dict["leaf_index"], expect["leaf_index"])
    assert np.float32(tree.scale).tobytes() == np.float32(expect["scale"]).tobytes()
    assert np.array_equal(tree.point_leaf_ids.cpu().numpy(), expect["point_leaf"])
    assert len(np.unique(tree.leaf_depths())) >= 2
    check_means(tree, expect, data)
    again = ffn.OcTree.build_from_samples(dev_pos, 8, 4, dev_data)
    for key, value in tree.state_dict.items():
        assert np.asarray(again.state_dict[key]).tobytes() == np.asarray(value).tobytes(), key
    assert torch.equal(again.point_leaf_ids, tree.point_leaf_ids)


@pytest.mark.parametrize("name", ["shell", "planes", "nodata"])
def test_query_equals_the_reference_answers(fixture, name):
    g = cloud(fixture, name)
    tree = build(g)
    answers = tree.query(g["query"])
    assert answers.dtype == np.int64 and np.array_equal(answers, g["query_result"])
    assert tree.query(g["query"][0])[0] == g["query_result"][0]        # a single (3,) position


def query_positions(scale, own):
    """1 M positions: a third outside the cube, 50 000 on faces and splitting planes (dyadic
    multiples of the scale), some of the cloud's own points."""
    rng = np.random.default_rng(11)
    n = 1 << 20
    q = (rng.random((n, 3), dtype=np.float32) * np.float32(2) - np.float32(1)) * scale
    third = n // 3
    far = (np.float32(1) + rng.random(third, dtype=np.float32)) * scale
    q[np.arange(third), rng.integers(0, 3, third)] = far * rng.choice(np.float32([-1, 1]), third)
    q[third:third + 50000] = (rng.integers(-16, 17, size=(50000, 3)) / 16).astype(np.float32) * scale
    q[third + 50000:third + 50000 + len(own)] = own
    return q


def test_query_a_million_positions(fixture):
    g = cloud(fixture, "shell")
    tree = build(g)
    scale = np.float32(tree.scale)
    q = query_positions(scale, g["positions"][:400] - oref.root_cube(g["positions"])[0])
    state = tree.state_dict
    expect = oref.query(scale, state["node_index"], state["leaf_index"], q)
    outside = (np.abs(q) > scale).any(1)
    assert outside.mean() > 0.3 and (expect >= 0).sum() > 1000
    assert ((np.abs(q) == scale).any(1) & ~outside).sum() > 100
    assert np.array_equal(tree.query(q), expect)


def opaque_ball(side=16):
    """A Voxels checkpoint with an opaque ball in empty space: rays through it end with
    alpha ~ 1, the others with alpha ~ 0."""
    import fourier_feature_nets as ffn
    model = ffn.Voxels(side, 1.0)
    axis = (np.arange(side) + 0.5) / side * 2 - 1
    x, y, z = np.meshgrid(axis, axis, axis, indexing="ij")
    inside = x * x + y * y + z * z < 0.45 ** 2
    rng = np.random.default_rng(3)
    volume = rng.normal(size=(1, 4, side, side, side)).astype(np.float32)
    volume[0, 3] = np.where(inside, 12.0, -12.0)
    with torch.no_grad():
        model.voxels.copy_(torch.from_numpy(volume))
        model.bias.zero_()
    return model


def render_batches(model, batch_size):
    """alpha, depth, colour, starts, directions of every training ray of scene16, rendered in
    the batches scripts/voxelize_model.py uses."""
    import fourier_feature_nets as ffn
    dataset = ffn.ImageDataset.load(SCENE, "train", 400, 128, False, None, device="cuda")
    sampler = dataset.sampler
    caster = ffn.Raycaster(model.to("cuda"))
    out = []
    with torch.no_grad():
        for start in range(0, len(sampler), batch_size):
            index = torch.arange(start, min(start + batch_size, len(sampler)), dtype=torch.int64,
                                 device="cuda")
            color, alpha, depth = caster.render(sampler.sample(index, None), True)
            out.append((alpha.contiguous(), depth.contiguous(), color.contiguous(),
                        sampler.starts[index].contiguous(),
                        sampler.directions[index].contiguous()))
    return out


def numpy_surface(alpha, depth, color, starts, dirs, threshold):
    """voxelize_model.py:71-77: the old name of ``octree_reference.surface_points``, on tensors."""
    alpha, depth, color, starts, dirs = [t.cpu().numpy() for t in (alpha, depth, color, starts, dirs)]
    return oref.surface_points(alpha, depth, starts, dirs, color, threshold)


def test_surface_points_equal_the_numpy_expression():
    from fourier_feature_nets_amd import ops
    (alpha, depth, color, starts, dirs), = render_batches(opaque_ball(), 4096)
    n = alpha.shape[0]
    present = float(alpha.min().item())                          # an alpha of this batch
    for threshold, kind in [(0.3, "some"), (present, "some"), (2.0, "none"), (-1.0, "all")]:
        pos, col, count = ops.octree_surface_points(alpha, depth, starts, dirs, threshold, color)
        assert count.dtype == torch.int32 and count.is_cuda
        k = int(count.item())
        want_pos, want_col = numpy_surface(alpha, depth, color, starts, dirs, threshold)
        print("threshold %r: %d of %d rays kept" % (threshold, k, n))
        assert k == len(want_pos)
        assert {"some": 0 < k < n, "none": k == 0, "all": k == n}[kind]
        assert pos[:k].cpu().numpy().tobytes() == want_pos.tobytes()
        assert col[:k].cpu().numpy().tobytes() == want_col.tobytes()
    # strict '>': the ray whose alpha IS the threshold is dropped
    keep = (alpha > present).sum().item()
    assert (alpha >= present).sum().item() > keep
    # without colours
    pos, col, count = ops.octree_surface_points(alpha, depth, starts, dirs, 0.3)
    assert col is None and int(count.item()) == len(numpy_surface(alpha, depth, color, starts,
                                                                  dirs, 0.3)[0])


def test_prune_save_load(fixture, tmp_path):
    import fourier_feature_nets as ffn
    g = cloud(fixture, "shell")
    tree = build(g)
    pruned = tree.prune()
    assert np.array_equal(pruned.state_dict["node_index"], g["pruned_node_index"])
    assert np.array_equal(pruned.state_dict["leaf_index"], g["pruned_leaf_index"])
    assert pruned.leaf_data().shape == g["pruned_leaf_data"].shape
    # (bit equality of prune itself is the CPU test's, from the reference's own leaf means; here
    # its input means differ from the reference's by their summation order: each within
    # (n + 1) 2^-24 of values below 1, n <= 20000 points in all, and prune averages them)
    np.testing.assert_allclose(pruned.leaf_data(), g["pruned_leaf_data"], rtol=0,
                               atol=20001 * 2.0 ** -24)
    assert pruned.depth == tree.depth - 1
    path = str(tmp_path / "tree.npz")
    tree.save(path)
    with np.load(path) as f:
        assert sorted(f.files) == ["leaf_data", "leaf_index", "node_index", "scale"]
        assert f["node_index"].dtype == np.int64 and f["leaf_index"].dtype == np.int64
        assert f["leaf_data"].dtype == np.float32 and f["scale"].dtype == np.float32
        assert f["scale"].shape == ()
    back = ffn.OcTree.load(path)
    for key, value in tree.state_dict.items():
        assert np.asarray(back.state_dict[key]).tobytes() == np.asarray(value).tobytes(), key
    assert np.array_equal(back.query(g["query"]), g["query_result"])
    assert back.leaf_centers().tobytes() == g["leaf_centers"].tobytes()


def test_voxelize_model_end_to_end(tmp_path):
    """scripts/voxelize_model.py as a program on scene16 with a small saved model: the saved
    tree is the restatement's tree of the cloud extracted here from the same renders."""
    model_path, out_path = str(tmp_path / "voxels.pt"), str(tmp_path / "tree.npz")
    opaque_ball().save(model_path)
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "voxelize_model.py"),
                          model_path, SCENE, out_path, "--voxel-depth", "5", "--batch-size", "300",
                          "--min-leaf-size", "2", "--scenepic-path", str(tmp_path / "tree.html")],
                         capture_output=True, text=True, cwd=ROOT)
    assert res.returncode == 0, res.stderr[-2000:]
    assert not os.path.exists(str(tmp_path / "tree.html")) and "scenepic" in res.stderr
    import fourier_feature_nets as ffn
    clouds = [numpy_surface(*batch, 0.3) for batch in render_batches(ffn.load_model(model_path), 300)]
    positions = np.concatenate([c[0] for c in clouds])
    colors = np.concatenate([c[1] for c in clouds])
    assert 50 < len(positions) < 1024
    assert "%d points in cloud" % len(positions) in res.stdout
    expect = oref.build(positions, 5, 2, colors)
    with np.load(out_path) as f:
        assert np.array_equal(f["node_index"], expect["node_index"])
        assert np.array_equal(f["leaf_index"], expect["leaf_index"])
        assert f["scale"].tobytes() == np.float32(expect["scale"]).tobytes()
        bound = mean_bound(colors, expect["point_leaf"], expect["leaf_index"], expect["leaf_count"])
        assert (np.abs(f["leaf_data"].astype(np.float64) - expect["leaf_data"]) <= bound).all()
    assert len(expect["node_index"]) > 0
