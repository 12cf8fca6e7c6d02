"""K22 on the GPU: ``ops.mesh_sample`` against the numpy restatement (tests/mesh_reference.py) BIT
FOR BIT on positions, UVs and colours -- the kernel's operation order is fixed and the subdivision
rounds are exact, so there is no tolerance to choose -- at the sample counts, triangle layouts,
digit boundaries, texture shapes and UVs where the kernel takes another path; then
``OcTree.build_from_triangles`` end to end and the two scripts as programs."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_reference as mref

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    assert x.dtype == np.float32
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(got, want):
    return got.shape == want.shape and np.array_equal(bits(got), bits(want))


def run_kernel(vertices, triangles, uvs, counts, texture, want_uvs=True):
    from fourier_feature_nets_amd import ops
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    dev = torch.device("cuda")
    return ops.mesh_sample(torch.from_numpy(np.ascontiguousarray(vertices, np.float32)).to(dev),
                           torch.from_numpy(np.ascontiguousarray(triangles, np.int32)).to(dev),
                           torch.from_numpy(np.ascontiguousarray(uvs, np.float32)).to(dev),
                           torch.from_numpy(offsets).to(dev),
                           torch.from_numpy(np.ascontiguousarray(texture)).to(dev), want_uvs)


def check(vertices, triangles, uvs, counts, texture):
    """Kernel == restatement on all three outputs; -> the restatement's arrays."""
    want = mref.mesh_sample(vertices, triangles, uvs, counts, texture)
    got = run_kernel(vertices, triangles, uvs, counts, texture)
    assert len(got) == 3
    for name, g, w in zip(("positions", "colors", "sample_uvs"), got, want):
        assert g.dtype == torch.float32 and tuple(g.shape) == w.shape, name
        differ = np.flatnonzero((bits(g) != bits(w)).any(-1))
        assert len(differ) == 0, "%s: %d of %d samples differ, first %d: %r != %r" % (
            name, len(differ), len(w), differ[0], g[int(differ[0])].tolist(), w[differ[0]].tolist())
    return want


def random_mesh(num_vertices, num_triangles, seed, texture_shape=(5, 4, 3)):
    rng = np.random.default_rng(seed)
    vertices = rng.uniform(-0.8, 0.8, (num_vertices, 3)).astype(np.float32)
    uvs = rng.uniform(0.0, 1.0, (num_vertices, 2)).astype(np.float32)
    triangles = np.stack([rng.permutation(num_vertices)[:3] for _ in range(num_triangles)])
    texture = rng.integers(0, 256, texture_shape, dtype=np.uint8)
    return vertices, triangles.astype(np.int32), uvs, texture


# ------------------------------------------------------------------------------- counts
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 5000])
def test_sample_counts_around_the_launch_block(n):
    vertices, triangles, uvs, texture = random_mesh(12, 7, seed=1)
    counts = np.random.default_rng(n).multinomial(n, np.full(7, 1 / 7))
    positions, colors, _ = check(vertices, triangles, uvs, counts, texture)
    assert positions.shape == (n, 3) and colors.shape == (n, 3)


@pytest.mark.parametrize("counts", [
    [0, 3, 0, 5, 0, 0, 7, 0, 0, 0, 0, 0, 2, 0],          # first, last, runs of 1, 2 and 5
    [0, 0, 300, 1],
    [9],                                                 # F = 1
    [1],
    [0] * 37 + [700] + [0] * 63,                         # one among 100 empty ones
    [700] + [0] * 100,
    [0] * 100 + [700],
], ids=["runs", "leading", "one_triangle", "one_sample", "middle_of_100", "first_of_101",
        "last_of_101"])
def test_zero_count_triangles(counts):
    vertices, triangles, uvs, texture = random_mesh(40, len(counts), seed=2)
    check(vertices, triangles, uvs, np.array(counts), texture)


def test_digit_boundaries():
    """One triangle with 70 000 samples next to triangles with 1 and 2: the sample numbers run
    through 3|4, 15|16, 255|256, 4095|4096 and 65535|65536, where n gains a base-4 digit pair (up
    to 9 digits), and the binary search steps over a large and two tiny ranges."""
    vertices, triangles, uvs, texture = random_mesh(9, 3, seed=3)
    counts = np.array([1, 70000, 2])
    _, number = mref.sample_numbers(counts)
    assert number.max() == 70000 and {3, 4, 15, 16, 255, 256, 4095, 4096, 65535, 65536} <= set(
        number.tolist())
    positions, _, _ = check(vertices, triangles, uvs, counts, texture)
    # all 16 rounds matter: the points of one triangle are distinct
    assert len(np.unique(mref.triangle_points(number[1:70001]), axis=0)) == 70000
    # and the samples lie in their triangle's plane, inside it (a property, to float32 rounding)
    corners = vertices[triangles[1]].astype(np.float64)
    edges = np.stack([corners[0] - corners[2], corners[1] - corners[2]], -1)
    solved, *_ = np.linalg.lstsq(edges, (positions[1:70001].astype(np.float64) - corners[2]).T,
                                 rcond=None)
    assert solved.min() > -1e-6 and solved.sum(0).max() < 1 + 1e-6
    np.testing.assert_allclose(edges @ solved, (positions[1:70001] - corners[2]).T, atol=1e-6)


# ------------------------------------------------------------------------------- textures
@pytest.mark.parametrize("shape", [(1, 1), (2, 3), (5, 4)], ids=lambda s: "%dx%d" % s)
def test_textures_and_channels(shape):
    vertices, triangles, uvs, rgba = random_mesh(12, 7, seed=4, texture_shape=shape + (4,))
    counts = np.array([50, 0, 120, 33, 64, 1, 200])
    rgb = np.ascontiguousarray(rgba[..., :3])
    _, colors3, _ = check(vertices, triangles, uvs, counts, rgb)
    _, colors4, _ = check(vertices, triangles, uvs, counts, rgba)
    assert same_bits(colors3, colors4)              # the fourth channel is ignored
    assert colors3.min() >= 0.0
    if shape == (1, 1):
        # one texel: its colour, after eight roundings of positive terms (two factors, their
        # product, the product with the texel, three sums, the division)
        np.testing.assert_allclose(colors3, np.broadcast_to(rgb[0, 0] / 255.0, colors3.shape),
                                   rtol=8 * 2.0 ** -24)


def uv_mesh():
    """Triangles whose three corners share one UV, so that the samples' UVs sit at (or within a
    rounding of) that value: 0, exactly 1, 1 - 2^-24, slightly negative, 1.5, and mixed ones."""
    below_one = np.float32(1) - np.float32(2.0 ** -24)
    values = [(0.0, 0.0), (1.0, 1.0), (below_one, below_one), (-1e-3, 0.5), (0.5, -1e-3),
              (1.5, 0.25), (0.25, 1.5), (-0.75, 1.0), (1.0, 0.0)]
    rng = np.random.default_rng(5)
    vertices = rng.uniform(-0.8, 0.8, (3 * len(values) + 3, 3)).astype(np.float32)
    uvs = np.repeat(np.float32(values), 3, axis=0)
    # and one triangle that runs from inside the image to outside on both sides
    uvs = np.concatenate([uvs, np.float32([[-0.2, -0.2], [1.3, 0.4], [0.4, 1.3]])])
    triangles = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    return vertices, triangles, uvs


def test_uvs_and_clamping():
    vertices, triangles, uvs = uv_mesh()
    texture = np.random.default_rng(6).integers(0, 256, (5, 4, 3), dtype=np.uint8)
    counts = np.full(len(triangles), 64)
    counts[-1] = 1024
    _, colors, sample_uvs = check(vertices, triangles, uvs, counts, texture)
    # the cases are there: u = 0, u = 1 exactly (col = W, one past the last texel), just below 1,
    # below 0 (floor = -1) and past the image
    u = sample_uvs[:, 0]
    assert (u == 0).any() and (u == 1).any() and ((u < 1) & (u > 1 - 2.0 ** -22)).any()
    assert (u < 0).any() and (u > 1.25).any() and (sample_uvs[:, 1] > 1.25).any()
    assert (sample_uvs[:, 1] < 0).any() and (sample_uvs[:, 1] == 1).any()
    assert np.isfinite(colors).all()
    assert colors.min() >= 0.0 and colors.max() <= 1.0


def test_saturated_texture_stays_at_one():
    """Every texel 255: a colour is 255 times the sum of the four rounded weights, over 255 -- 1.0
    to the rounding of the weights and their sum, within 2 float32 ulp."""
    vertices, triangles, uvs = uv_mesh()
    texture = np.full((5, 4, 3), 255, np.uint8)
    counts = np.full(len(triangles), 256)
    _, colors, _ = check(vertices, triangles, uvs, counts, texture)
    ulp = 2.0 ** -23
    assert np.abs(colors.astype(np.float64) - 1.0).max() <= 2 * ulp


def test_optional_uvs_and_repeatability():
    vertices, triangles, uvs, texture = random_mesh(12, 7, seed=7)
    counts = np.array([500, 0, 1200, 333, 64, 1, 2000])
    with_uvs = run_kernel(vertices, triangles, uvs, counts, texture, want_uvs=True)
    without = run_kernel(vertices, triangles, uvs, counts, texture, want_uvs=False)
    again = run_kernel(vertices, triangles, uvs, counts, texture, want_uvs=True)
    assert len(without) == 2
    assert same_bits(without[0], with_uvs[0]) and same_bits(without[1], with_uvs[1])
    for first, second in zip(with_uvs, again):
        assert same_bits(first, second)


def test_device_refusals():
    from fourier_feature_nets_amd import ops
    vertices, triangles, uvs, texture = random_mesh(12, 7, seed=8)
    bad = triangles.copy()
    bad[3, 1] = 12
    with pytest.raises(ValueError, match="triangles"):
        run_kernel(vertices, bad, uvs, np.full(7, 3), texture)
    with pytest.raises(ValueError, match="offsets"):
        run_kernel(vertices, triangles, uvs, np.array([3, 3, -1, 3, 3, 3, 3]), texture)
    # the ABI's own refusals (no launch): a null output, a texture with two channels
    from fourier_feature_nets_amd._lib import FfnError, c_i, c_i64
    dev = torch.device("cuda")
    t = {name: torch.from_numpy(np.ascontiguousarray(a)).to(dev) for name, a in
         dict(v=vertices, t=triangles, uv=uvs, o=np.arange(0, 22, 3, dtype=np.int32),
              tex=texture).items()}
    out = torch.empty((21, 3), dtype=torch.float32, device=dev)

    def call(channels, colors):
        ops._call("ffn_mesh_sample", ops._dev(t["v"]), c_i64(12), ops._dev(t["t"], torch.int32),
                  c_i64(7), ops._dev(t["uv"]), ops._dev(t["o"], torch.int32), c_i64(21),
                  ops._dev(t["tex"], torch.uint8), c_i(5), c_i(4), c_i(channels), ops._dev(out),
                  ops._dev(colors), ops._dev(None))
    with pytest.raises(FfnError, match="null"):
        call(3, None)
    with pytest.raises(FfnError, match="texture"):
        call(2, out.clone())
    call(3, out.clone())


# ------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def torus():
    from fourier_feature_nets import procedural_torus
    return procedural_torus(16, 8, 32)


@pytest.fixture(scope="module", params=[5, 6])
def torus_trees(request, torus):
    """(depth, tree from build_from_triangles, tree from build_from_samples on the restatement's
    cloud, that cloud): built once per depth."""
    import fourier_feature_nets as ffn
    depth, min_leaf_size = request.param, 4
    vertices, triangles, uvs, texture = torus
    tree = ffn.OcTree.build_from_triangles(vertices, triangles, uvs, texture, depth, min_leaf_size)
    points = ffn.normalize_points(vertices, (0, 1, 0))
    counts = ffn.triangle_counts(points, triangles, 8 ** (depth - 2) * min_leaf_size, seed=0)
    positions, colors, _ = mref.mesh_sample(points, triangles, uvs, counts,
                                            np.ascontiguousarray(texture[::-1]))
    restated = ffn.OcTree.build_from_samples(positions, depth, min_leaf_size, colors)
    return depth, tree, restated, positions


def test_build_from_triangles_equals_restated_cloud(torus_trees):
    depth, tree, restated, positions = torus_trees
    assert len(positions) == 8 ** (depth - 2) * 4
    assert tree.scale == restated.scale and tree.center == restated.center
    got, want = tree.state_dict, restated.state_dict
    np.testing.assert_array_equal(got["node_index"], want["node_index"])
    np.testing.assert_array_equal(got["leaf_index"], want["leaf_index"])
    assert tree.leaf_data().shape == (tree.num_leaves, 3)
    assert same_bits(tree.leaf_data(), restated.leaf_data())
    assert tree.depth == depth and tree.num_leaves > 8 ** (depth - 3)
    assert 0.0 <= tree.leaf_data().min() and tree.leaf_data().max() <= 1.0


def test_leaves_lie_on_the_cloud(torus_trees):
    """A leaf holds at least min_leaf_size points of the cloud, all inside its cube, so its centre
    is within the cube's half diagonal of the nearest one."""
    from scipy.spatial import cKDTree
    _, tree, _, positions = torus_trees
    centers = tree.leaf_centers().astype(np.float64) + np.float64(tree.center)
    half_side = tree.scale / 2.0 ** tree.leaf_depths().astype(np.float64)
    distance, _ = cKDTree(positions.astype(np.float64)).query(centers)
    assert (distance <= np.sqrt(3.0) * half_side + 1e-6).all()


def test_same_seed_same_tree(torus, torus_trees):
    import fourier_feature_nets as ffn
    depth, tree, _, _ = torus_trees
    again = ffn.OcTree.build_from_triangles(*torus, depth, 4, seed=0)
    other = ffn.OcTree.build_from_triangles(*torus, depth, 4, seed=1)
    assert again.scale == tree.scale and again.center == tree.center
    for key in ("node_index", "leaf_index"):
        np.testing.assert_array_equal(again.state_dict[key], tree.state_dict[key])
    assert same_bits(again.leaf_data(), tree.leaf_data())
    assert (other.num_leaves != tree.num_leaves
            or not same_bits(other.leaf_data(), tree.leaf_data()))


def test_render_hits_the_torus(torus_trees):
    import contextlib
    import io
    import fourier_feature_nets as ffn
    from bench import synthetic_rig
    _, tree, _, _ = torus_trees
    intrinsics, poses = synthetic_rig(1, 32)
    camera = ffn.CameraInfo.create("c000", ffn.Resolution(32, 32), intrinsics, poses[0])
    with contextlib.redirect_stdout(io.StringIO()):
        sampler = ffn.RaySampler(np.diag([2, 2, 2, 1]).astype(np.float32), [camera], 8)
    image, alpha, depth = tree.render_image(sampler, 0, shading="flat", include_depth=True)
    assert image.shape == (32, 32, 3) and image.dtype == np.uint8 and alpha.shape == (32, 32)
    assert 0.0 < alpha.mean() < 1.0
    assert image[alpha > 0].max() > 0 and (image[alpha == 0] == 0).all()
    assert np.isfinite(depth[alpha > 0]).all() and depth[alpha > 0].min() > 0


# ------------------------------------------------------------------------------- scripts
def run_script(script, *args):
    res = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", script)] + list(args),
                         capture_output=True, text=True, cwd=ROOT, timeout=300)
    assert res.returncode == 0, res.stderr[-2000:]
    return res.stdout


def test_make_mesh_npz_program(tmp_path):
    import contextlib
    import io
    import fourier_feature_nets as ffn
    path, tree_path = str(tmp_path / "torus.npz"), str(tmp_path / "tree.npz")
    out = run_script("make_mesh_npz.py", path, "--voxel-depth", "5", "--size", "16", "--cameras",
                     "4", "--tree", tree_path)
    assert "--center" in out
    data = np.load(path)
    assert data["images"].shape == (4, 16, 16, 4) and data["images"].dtype == np.uint8
    assert data["intrinsics"].shape == (4, 3, 3) and data["extrinsics"].shape == (4, 4, 4)
    assert data["bounds"].shape == (4, 4) and data["split_counts"].tolist() == [2, 1, 1]
    assert data["split_counts"].dtype == np.int32
    alpha = data["images"][..., 3]
    assert set(np.unique(alpha)) == {0, 255}
    assert (data["images"][..., :3][alpha == 0] == 0).all()
    with contextlib.redirect_stdout(io.StringIO()):
        train = ffn.ImageDataset.load(path, "train", 8, True, False)
    assert train is not None and train.num_cameras == 2
    assert ffn.OcTree.load(tree_path).depth == 5


def test_mesh_to_octree_program(tmp_path, torus):
    import fourier_feature_nets as ffn
    from PIL import Image
    vertices, triangles, uvs, texture = torus
    Image.fromarray(texture).save(tmp_path / "skin.png")
    (tmp_path / "torus.mtl").write_text("newmtl skin\nmap_Kd skin.png\n")
    lines = ["mtllib torus.mtl", "usemtl skin"]
    lines += ["v %r %r %r" % tuple(float(x) for x in v) for v in vertices]
    lines += ["vt %r %r" % tuple(float(x) for x in t) for t in uvs]
    lines += ["f " + " ".join("%d/%d" % (i + 1, i + 1) for i in t) for t in triangles]
    (tmp_path / "torus.obj").write_text("\n".join(lines) + "\n")
    out_path = str(tmp_path / "tree.npz")
    out = run_script("mesh_to_octree.py", str(tmp_path / "torus.obj"), out_path, "--voxel-depth",
                     "5")
    assert "--center" in out
    loaded = ffn.OcTree.load(out_path)
    # the reader numbers the vertices in the order the faces use them, so the float64 mean of the
    # normalisation, and with it the cloud, can differ in last bits from the arrays' own tree:
    # the same tree up to a few boundary leaves, not bit for bit
    direct = ffn.OcTree.build_from_triangles(vertices, triangles, uvs, texture, 5, 4)
    assert loaded.depth == 5 and abs(loaded.scale - direct.scale) < 1e-5
    assert loaded.leaf_data().shape == (loaded.num_leaves, 3)
    assert abs(loaded.num_leaves - direct.num_leaves) <= 0.05 * direct.num_leaves
    assert 0.0 <= loaded.leaf_data().min() and loaded.leaf_data().max() <= 1.0
