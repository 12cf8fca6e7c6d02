"""K33 on the GPU: the three kernels against the numpy restatement of their contract
(tests/mesh_texture_reference.py) bit for bit (NaN compared as equal), on the image and texture
sizes, UV placements and meshes the contract names; the same bits over calls, chunk sizes and
accumulation; the tie to K31c's textured colour and the adjoint identity on the device's own
outputs; ``texture_mesh_from_images`` and ``fit_mesh_texture`` on a tiny dataset drawn here;
scripts/texture_mesh.py as a program."""

import contextlib
import io
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest
import torch

from tests import mesh_raster_grad_reference as Rg
from tests import mesh_raster_reference as ref
from tests import mesh_texture_reference as Rt
from tests import stream_order_cases_mesh_fit  # noqa: F401  (the table as the whole suite has it)
from tests import stream_order_cases_mesh_texture  # noqa: F401  (adds K33's stream-order cases)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def on_gpu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def assert_bits(got, want, name):
    """The same bits, any NaN counting as any other NaN."""
    assert got.dtype == want.dtype and got.shape == want.shape, name
    if got.dtype.kind == "f":
        both_nan = np.isnan(got) & np.isnan(want)
        got, want = np.where(both_nan, 0, got).view(np.uint32), np.where(both_nan, 0, want).view(
            np.uint32)
    np.testing.assert_array_equal(got, want, err_msg=name)


def view(width, height, **kwargs):
    from fourier_feature_nets_amd.cameras import projection_matrices
    return projection_matrices([ref.camera(width, height, **kwargs)])[0]


def noise(count, seed=0):
    return np.random.default_rng(seed).standard_normal((count, 3)).astype(np.float32)


def device_k33(vertices, triangles, uvs, proj, width, height, size, texture, d_color,
               batch_size=1 << 22, replace_ids=None, background=(0.25, 0.5, 0.75)):
    """K31a-c for the ids, then K33a, the sort, K33b and K33c through the public wrappers ->
    numpy.  ``replace_ids`` maps the ids of K31c to the ones K33a is given."""
    from fourier_feature_nets_amd import mesh, ops
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    record = ops.mesh_raster_setup(v, t, proj, width, height)[0]
    ids = mesh.rasterize_mesh(v, t, proj, ref.ORIGIN, width, height, colors=v,
                              batch_size=batch_size)[3]
    if replace_ids is not None:
        ids = on_gpu(replace_ids(ids.cpu().numpy()), "int32")
    tap_texel, tap_weight = ops.mesh_texture_taps(record, ids, t, on_gpu(uvs, "float32"), size[0],
                                                  size[1], width, height)
    sorted_texels, order = torch.sort(tap_texel.reshape(-1), stable=True)
    order = order.to(torch.int32)
    color, alpha = ops.mesh_texture_gather(tap_texel, tap_weight, on_gpu(texture, "float32"),
                                           background)
    grad, weight = ops.mesh_texture_grad(sorted_texels, order, tap_weight,
                                         on_gpu(d_color, "float32"), size[0] * size[1])
    out = dict(ids=ids, tap_texel=tap_texel, tap_weight=tap_weight, sorted_texels=sorted_texels,
               order=order, color=color, alpha=alpha, grad=grad, weight=weight)
    return types.SimpleNamespace(**{k: x.cpu().numpy() for k, x in out.items()})


NAMES = ("tap_texel", "tap_weight", "sorted_texels", "order", "color", "alpha", "grad", "weight")


def both(vertices, triangles, uvs, proj, width, height, size, seed=0, replace_ids=None):
    """The device against the restatement, bit for bit -> the device's results."""
    rng = np.random.default_rng(seed)
    texture = rng.uniform(0, 1, (size[0] * size[1], 3)).astype(np.float32)
    d_color = noise(width * height, seed + 1)
    background = (0.25, 0.5, 0.75)
    got = device_k33(vertices, triangles, uvs, proj, width, height, size, texture, d_color,
                     replace_ids=replace_ids, background=background)
    state, ids = Rg.raster_ids(vertices, triangles, proj, width, height)
    if replace_ids is not None:
        ids = replace_ids(ids)
    np.testing.assert_array_equal(got.ids, ids)
    want = types.SimpleNamespace()
    want.tap_texel, want.tap_weight = Rt.taps(state, ids, uvs, size[0], size[1], width)
    want.sorted_texels, want.order = Rt.sort_taps(want.tap_texel)
    want.color, want.alpha = Rt.gather(want.tap_texel, want.tap_weight, texture, background)
    want.grad, want.weight = Rt.grad(want.sorted_texels, want.order, want.tap_weight, d_color,
                                     size[0] * size[1])
    for name in NAMES:
        assert_bits(getattr(got, name), getattr(want, name), name)
    got.state, got.texture, got.d_color = state, texture, d_color
    got.covered = got.tap_texel[:, 0] >= 0
    return got


ONE = np.array([[0, 1, 2]], np.int32)
COVER = ref.flat([(-1, -1), (200, -1), (-1, 200)])           # covers every image up to 100 a side
COVER_UVS = np.array([[0.1, 0.2], [0.9, 0.3], [0.4, 1.2]], np.float32)


@pytest.mark.parametrize("size", [(1, 1), (2, 2), (8, 4)])
@pytest.mark.parametrize("width,height", [(1, 1), (5, 3), (48, 40)])
def test_image_and_texture_sizes(width, height, size):
    """1 x 1 and 5 x 3: one triangle over the whole image; 48 x 40: ``scene(3, 40)`` with UVs in
    [-0.5, 1.5], so that taps clamp and repeat at every border of the texture."""
    if (width, height) == (48, 40):
        vertices, triangles, _, uvs = ref.scene(3, 40)
        out = both(vertices, triangles, uvs, view(width, height), width, height, size)
        assert 0.15 < out.covered.mean() < 0.9
        used = np.unique(out.tap_texel[out.covered])
        # texel 0 and texel T - 1 are not empty: the two ends of the binary search
        assert used.min() == 0 and used.max() == size[0] * size[1] - 1
        assert out.weight[0] > 0 and out.weight[-1] > 0
    else:
        out = both(COVER, ONE, COVER_UVS, ref.PIXEL_PROJ, width, height, size)
        assert out.covered.all() and (out.alpha == 1).all()


def test_uvs_on_integer_texels_and_on_the_last_row_and_column():
    """Under PIXEL_PROJ at depth 1 the triangle (0,0) (16,0) (0,16) has b_i = E_i / 256 exactly, so
    u = px / 8 and v = py / 8 are exact and col = px, row = py on an 8 x 8 texture: dj = di = 0 at
    every pixel, and from pixel 7 on the taps clamp to the last column and row and repeat."""
    vertices = ref.flat([(0, 0), (16, 0), (0, 16)])
    uvs = np.array([[0, 0], [2, 0], [0, 2]], np.float32)
    out = both(vertices, ONE, uvs, ref.PIXEL_PROJ, 12, 12, (8, 8))
    hit = np.flatnonzero(out.covered)
    px, py = hit % 12, hit // 12
    assert len(hit) > 100 and (px + py <= 16).all()
    np.testing.assert_array_equal(out.tap_weight[hit], np.tile([1.0, 0, 0, 0], (len(hit), 1)))
    np.testing.assert_array_equal(out.tap_texel[hit, 0], np.minimum(py, 7) * 8 + np.minimum(px, 7))
    last = (px >= 7) & (py >= 7)
    assert last.any() and (out.tap_texel[hit][last] == 63).all()
    # a zero weight is skipped: every texel's weight is its number of pixels
    counts = np.bincount(out.tap_texel[hit, 0], minlength=64).astype(np.float32)
    np.testing.assert_array_equal(out.weight, counts)


def test_nan_and_infinite_uvs_reach_no_texel():
    """``scene(3, 40)`` with NaN UVs on one visible triangle and infinite ones on another: their
    weights are NaN in K33a's output, their colour is NaN in K33b's, and K33c stays finite."""
    vertices, triangles, _, uvs = ref.scene(3, 40)
    _, ids = Rg.raster_ids(vertices, triangles, view(48, 40), 48, 40)
    seen = np.argsort(np.bincount(ids[ids >= 0], minlength=40))[::-1][:2]
    uvs = uvs.copy()
    uvs[triangles[seen[0]]] = np.nan
    uvs[triangles[seen[1]]] = [np.inf, -np.inf]
    out = both(vertices, triangles, uvs, view(48, 40), 48, 40, (8, 4))
    bad = np.isin(out.ids, seen)
    assert bad.sum() > 20 and np.isnan(out.tap_weight[bad]).all()
    assert np.isnan(out.color[bad]).all() and np.isfinite(out.color[~bad]).all()
    assert (out.tap_texel[bad] >= 0).all() and (out.tap_texel[bad] < 32).all()
    assert np.isfinite(out.grad).all() and np.isfinite(out.weight).all()
    covered = int((out.covered & ~bad).sum())
    assert abs(float(out.weight.astype(np.float64).sum()) - covered) < 1e-3 * covered


def test_an_empty_image():
    vertices = ref.flat([(-30, -30), (-20, -30), (-25, -12)])
    out = both(vertices, ONE, COVER_UVS, ref.PIXEL_PROJ, 16, 8, (4, 4))
    assert (out.tap_texel == -1).all() and (out.sorted_texels == -1).all()
    assert not out.tap_weight.view(np.uint32).any() and not out.alpha.any()
    np.testing.assert_array_equal(out.color, np.tile(np.float32([0.25, 0.5, 0.75]), (128, 1)))
    assert not out.grad.view(np.uint32).any() and not out.weight.view(np.uint32).any()


def test_one_triangle_over_the_whole_image_and_one_texel_under_all_of_it():
    out = both(COVER, ONE, COVER_UVS, ref.PIXEL_PROJ, 33, 17, (4, 4))
    assert out.covered.all()
    # a 1 x 1 texture under 32 x 32 pixels: one row with every tap, 4096 slots
    out = both(COVER, ONE, COVER_UVS, ref.PIXEL_PROJ, 32, 32, (1, 1))
    assert out.covered.all() and (out.tap_texel == 0).all()
    assert abs(float(out.weight[0]) - 1024) < 1e-2


def test_foreign_ids_are_uncovered():
    vertices, triangles, _, uvs = ref.scene(3, 40)

    def replace(ids):
        ids = ids.copy()
        hit = np.flatnonzero(ids >= 0)
        ids[hit[::3]] = -7
        ids[hit[1::3]] = len(triangles)
        ids[np.flatnonzero(ids < 0)[:5]] = 2 ** 31 - 1
        return ids
    out = both(vertices, triangles, uvs, view(48, 40), 48, 40, (8, 4), replace_ids=replace)
    foreign = (out.ids < 0) | (out.ids >= len(triangles))
    assert (out.ids == -7).sum() > 50 and (out.ids == len(triangles)).sum() > 50
    assert (out.tap_texel[foreign] == -1).all() and not out.tap_weight[foreign].any()
    assert not out.alpha[foreign].any() and out.covered.sum() > 50


def test_an_occluded_triangle_keeps_its_unoccluded_pixels_only():
    near = ref.flat([(4, 4), (12, 4), (4, 12)], 1.0)
    far = ref.flat([(2, 2), (20, 2), (2, 20)], 2.0)
    vertices = np.concatenate([far, near])
    triangles = np.arange(6, dtype=np.int32).reshape(2, 3)
    # the far triangle reads the lower half of the texture, the near one the upper half
    uvs = np.array([[0, 0], [1, 0], [0, 0.45], [0, 0.55], [1, 0.55], [0, 1]], np.float32)
    out = both(vertices, triangles, uvs, ref.PIXEL_PROJ, 24, 24, (8, 8))
    image = out.ids.reshape(24, 24)
    assert image[5, 5] == 1 and image[3, 3] == 0 and image[14, 4] == 0
    rows = out.tap_texel // 8
    assert (rows[out.ids == 0] <= 4).all() and (rows[out.ids == 1] >= 4).all()
    lower = float(out.weight.reshape(8, 8)[:4].astype(np.float64).sum())
    assert lower <= (out.ids == 0).sum() + 1e-3 < int(out.state["counts"][0])


def test_257_triangles_on_300_shared_vertices():
    rng = np.random.default_rng(32)
    vertices = rng.uniform(-0.8, 0.8, (300, 3)).astype(np.float32)
    triangles = rng.integers(0, 300, (257, 3)).astype(np.int32)
    uvs = rng.uniform(0, 1, (300, 2)).astype(np.float32)
    out = both(vertices, triangles, uvs, view(64, 48), 64, 48, (16, 16))
    assert out.covered.mean() > 0.15


def _block_mesh():
    from tests.octree_mesh_cases import case
    from fourier_feature_nets_amd.octree import OcTree
    c = case("cuboid")
    tree = OcTree(c.scale, c.nodes, c.leaves, c.leaf_data, c.sh_degree)
    return tree.extract_mesh(placement="corners", center=(1.0, 0.25, -0.5))


@pytest.mark.parametrize("tile", [3, 4])
def test_the_block_mesh_of_a_lattice_tree_after_unwrap_mesh(tile):
    import fourier_feature_nets_amd as ffn
    surface = _block_mesh()
    flat_vertices = np.asarray(surface.vertices, np.float32)
    flat_triangles = np.asarray(surface.triangles, np.int32)
    vertices, triangles, uvs, vertex_map, size = ffn.unwrap_mesh(flat_vertices, flat_triangles, tile)
    want_triangles, texel, want_map, tile_of, want_size = Rt.unwrap(flat_triangles, tile)
    np.testing.assert_array_equal(triangles, want_triangles)
    np.testing.assert_array_equal(vertex_map, want_map)
    np.testing.assert_array_equal(uvs.astype(np.float64) * [size[1], size[0]], texel)
    assert size == want_size and len(np.unique(tile_of)) == len(flat_triangles) // 2
    out = both(vertices, triangles, uvs, view(64, 48, distance=4.5), 64, 48, size)
    hit = np.flatnonzero(out.covered)
    assert len(hit) > 300
    # every tap lies inside the tile of the triangle that won the pixel
    number = tile_of[out.ids[hit]]
    per_row = size[1] // tile
    assert ((out.tap_texel[hit] % size[1]) // tile == (number % per_row)[:, None]).all()
    assert ((out.tap_texel[hit] // size[1]) // tile == (number // per_row)[:, None]).all()


# ------------------------------------------------------------------------------- determinism
def test_the_same_bits_on_a_repeated_call_and_for_small_chunks():
    vertices, triangles, _, uvs = ref.scene(0, 60)
    proj, d_color = view(64, 48), noise(64 * 48, 3)
    texture = np.random.default_rng(4).uniform(0, 1, (64, 3)).astype(np.float32)
    first = device_k33(vertices, triangles, uvs, proj, 64, 48, (8, 8), texture, d_color)
    for batch in (1 << 22, 97):
        again = device_k33(vertices, triangles, uvs, proj, 64, 48, (8, 8), texture, d_color,
                           batch_size=batch)
        for name in NAMES:
            assert_bits(getattr(again, name), getattr(first, name), "%s, batch %d" % (name, batch))


def test_public_functions_and_accumulation_over_three_cameras():
    import fourier_feature_nets_amd as ffn
    vertices, triangles, _, uvs = ref.scene(3, 40)
    size = (8, 4)
    v, t, uv = on_gpu(vertices, "float32"), on_gpu(triangles, "int32"), on_gpu(uvs, "float32")
    cams = [ref.camera(48, 40, yaw=yaw) for yaw in (0.3, 1.3, 2.3)]
    d_colors = [noise(48 * 40, 20 + k) for k in range(3)]
    texture = np.random.default_rng(9).uniform(0, 1, size + (3,)).astype(np.float32)
    grad = torch.full(size + (3,), 7.0, device="cuda")                # overwritten by the first
    weight = torch.full(size, 7.0, device="cuda")
    want_grad, want_weight = None, None
    for k, (cam, g) in enumerate(zip(cams, d_colors)):
        taps = ffn.mesh_texture_taps(v, t, uv, cam, size, batch_size=97 if k == 1 else 1 << 22)
        assert isinstance(taps, ffn.MeshTaps) and (taps.height, taps.width) == size
        tap_texel, tap_weight, sorted_texels, order, _, _ = Rt.camera_taps(
            vertices, triangles, uvs, view(48, 40, yaw=(0.3, 1.3, 2.3)[k]), 48, 40, size)
        for name, want in (("tap_texel", tap_texel), ("tap_weight", tap_weight),
                           ("sorted_texels", sorted_texels), ("tap_order", order)):
            assert_bits(getattr(taps, name).cpu().numpy(), want, name)
        # the forward: a tensor gives tensors, numpy gives numpy, the same bits
        frame = ffn.render_mesh_texture(taps, on_gpu(texture, "float32"), (0.1, 0.2, 0.3))
        color, alpha = Rt.gather(tap_texel, tap_weight, texture.reshape(-1, 3), (0.1, 0.2, 0.3))
        assert torch.is_tensor(frame.color) and frame.depth is None
        assert_bits(frame.color.cpu().numpy(), color, "color")
        assert_bits(ffn.render_mesh_texture(taps, texture, (0.1, 0.2, 0.3)).alpha, alpha, "alpha")
        # the backward, alone and accumulated
        alone = ffn.render_mesh_texture_backward(taps, g)
        one = Rt.grad(sorted_texels, order, tap_weight, g, 32)
        assert alone[0].shape == size + (3,) and alone[1].shape == size
        assert_bits(alone[0].reshape(-1, 3), one[0], "grad alone")
        out = ffn.render_mesh_texture_backward(taps, on_gpu(g, "float32"), grad, weight,
                                               accumulate=k > 0)
        assert out[0] is grad and out[1] is weight
        want_grad, want_weight = Rt.grad(sorted_texels, order, tap_weight, g, 32, want_grad,
                                         want_weight, accumulate=k > 0)
        assert_bits(grad.cpu().numpy().reshape(-1, 3), want_grad, "running grad %d" % k)
        assert_bits(weight.cpu().numpy().reshape(-1), want_weight, "running weight %d" % k)


def test_the_taps_reproduce_k31c_on_the_device():
    """The colour formed from the device's taps and a uint8 texture, divided by 255 after the
    blend, is ``ops.mesh_raster_resolve``'s textured colour bit for bit."""
    from fourier_feature_nets_amd import mesh
    vertices, triangles, _, uvs = ref.scene(3, 40)
    proj = view(48, 40)
    size = (8, 4)
    bytes_ = ref.texture(33, size[0], size[1], 3)
    out = device_k33(vertices, triangles, uvs, proj, 48, 40, size, np.zeros((32, 3), np.float32),
                     noise(48 * 40))
    want = mesh.rasterize_mesh(on_gpu(vertices, "float32"), on_gpu(triangles, "int32"), proj,
                               ref.ORIGIN, 48, 40, uvs=on_gpu(uvs, "float32"),
                               texture=on_gpu(bytes_, "uint8"))[0].cpu().numpy()
    hit = np.flatnonzero(out.ids >= 0)
    t = bytes_.reshape(-1, 3).astype(np.float32)[out.tap_texel[hit]]
    w = out.tap_weight[hit][:, :, None]
    got = (((w[:, 0] * t[:, 0] + w[:, 1] * t[:, 1]) + w[:, 2] * t[:, 2])
           + w[:, 3] * t[:, 3]) / np.float32(255.0)
    assert len(hit) > 300
    assert_bits(got, want[hit], "K31c's textured colour")


def test_adjoint_identity_on_the_devices_own_outputs():
    vertices, triangles, _, uvs = ref.scene(3, 40)
    out = both(vertices, triangles, uvs, view(48, 40), 48, 40, (8, 4), seed=11)
    hit = out.covered
    left = float((out.color[hit].astype(np.float64) * out.d_color[hit].astype(np.float64)).sum())
    right = float((out.texture.astype(np.float64) * out.grad.astype(np.float64)).sum())
    depth = Rt.longest_row(out.sorted_texels, 32)
    budget = Rt.adjoint_budget(out.tap_texel, out.tap_weight, out.texture, out.d_color, depth)
    print("adjoint on the device: difference %.3g, budget %.3g, share %.3f"
          % (abs(left - right), budget, abs(left - right) / budget))
    assert abs(left - right) <= budget


# ------------------------------------------------------------------------------- stream order
@pytest.mark.parametrize("scenario", ["A", "B"])
@pytest.mark.parametrize("name", ["mesh_texture_taps", "mesh_texture_gather", "mesh_texture_grad"])
def test_k33_launches_on_the_callers_stream(name, scenario, monkeypatch):
    """The three cases of tests/stream_order_cases_mesh_texture.py under the harness of
    tests/test_stream_order_gpu.py, run from here as well: K33's share of the stream contract is
    held whenever this file runs, whatever else was collected and in whatever order."""
    from fourier_feature_nets_amd import _lib
    from tests import stream_helpers as sh
    from tests.stream_order_cases import CASES
    case, = [c for c in CASES if c.name == name]
    hook = sh.Hook(_lib.call)
    monkeypatch.setattr(_lib, "call", hook)
    reached = sh.run_case(case, scenario, hook, monkeypatch)
    assert set(case.reaches) <= set(reached)


# ------------------------------------------------------------------------------- the tiny dataset
SIZE, CAMERAS, TILE = 32, 4, 4


@pytest.fixture(scope="module")
def torus():
    """``procedural_torus(16, 8)`` with its quads' triangles side by side, unwrapped with tile 4,
    and a random float texture for the truth, drawn from 4 cameras at 32 x 32: the uint8 images
    through ``texture_to_uint8`` and K31 (alpha 255 where covered), the exact float frames of
    K33b, and an ``ImageDataset``, as tests/test_mesh_fit_gpu.py builds its own."""
    import fourier_feature_nets_amd as ffn
    from bench import synthetic_rig
    vertices, triangles, _, _ = ffn.procedural_torus(rings=16, sides=8)
    vertices = ffn.normalize_points(vertices)
    triangles = np.ascontiguousarray(triangles.reshape(2, -1, 3).transpose(1, 0, 2).reshape(-1, 3))
    vertices, triangles, uvs, _, size = ffn.unwrap_mesh(vertices, triangles, TILE)
    assert size == (32, 64) and len(vertices) == 4 * 128
    truth = np.random.default_rng(16).uniform(0, 1, size + (3,)).astype(np.float32)
    intr, poses = synthetic_rig(CAMERAS, SIZE)
    cams = [ffn.CameraInfo.create("c%d" % i, ffn.Resolution(SIZE, SIZE), intr, p)
            for i, p in enumerate(poses)]
    images = np.zeros((CAMERAS, SIZE, SIZE, 4), np.uint8)
    frames = []
    for index, cam in enumerate(cams):
        color, alpha, _ = ffn.render_mesh_image(vertices, triangles, cam, uvs=uvs,
                                                texture=ffn.texture_to_uint8(truth),
                                                include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.rint(255 * alpha)
        taps = ffn.mesh_texture_taps(vertices, triangles, uvs, cam, size)
        frames.append(ffn.render_mesh_texture(taps, truth).color)
    assert 0.1 < (images[..., 3] > 0).mean() < 0.9
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset("torus", images, bounds, cams, 2, True, False)
    images.setflags(write=False)                     # shared by the tests below: not written into
    return types.SimpleNamespace(vertices=vertices, triangles=triangles, uvs=uvs, size=size,
                                 truth=truth, cams=cams, images=images, frames=np.stack(frames),
                                 dataset=dataset, intrinsics=np.stack([intr] * CAMERAS),
                                 poses=np.stack(poses), bounds=bounds)


def _exact_targets(torus):
    """The dataset with the float frames for targets: what K33b drew, not its bytes."""
    import fourier_feature_nets_amd as ffn
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset("exact", torus.images, torus.bounds, torus.cams, 2, True, False)
    dataset.colors = on_gpu(torus.frames.reshape(-1, 3), "float32")
    return dataset


@pytest.mark.parametrize("threshold", [0.5, 0.0])
def test_texture_mesh_from_images_is_the_restatement(torus, threshold):
    """Alpha bytes of 100 in a window of every image: left out at 0.5 (128), kept at 0 (1)."""
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd.cameras import projection_matrices
    images = torus.images.copy()
    window = images[:, 10:20, 8:24, 3]
    window[window > 0] = 100
    data = types.SimpleNamespace(images=images, cameras=torus.cams, color_space="RGB")
    got, weights = ffn.texture_mesh_from_images(torus.vertices, torus.triangles, torus.uvs, data,
                                                torus.size, alpha_threshold=threshold)
    want, want_weights = Rt.texture_from_images(torus.vertices, torus.triangles, torus.uvs,
                                                projection_matrices(torus.cams), images, torus.size,
                                                alpha_threshold=threshold)
    assert_bits(weights, want_weights, "weights")
    assert_bits(got, want, "texture")
    seen = weights > 0
    assert seen.sum() > 200 and not seen.all()
    assert got[seen].min() >= 0.0 and got[seen].max() <= 1.0 + 1e-5
    # a texel nobody saw keeps the colour it was given; tensors stay tensors; RGB images mask nothing
    given = on_gpu(torus.truth, "float32")
    kept, w = ffn.texture_mesh_from_images(on_gpu(torus.vertices, "float32"),
                                           on_gpu(torus.triangles, "int32"),
                                           on_gpu(torus.uvs, "float32"), data, torus.size, given,
                                           alpha_threshold=threshold)
    assert torch.is_tensor(kept) and kept.is_cuda and kept.shape == given.shape
    assert_bits(w.cpu().numpy(), want_weights, "weights of the tensor call")
    assert_bits(kept.cpu().numpy()[seen], want[seen], "seen")
    assert_bits(kept.cpu().numpy()[~seen], torus.truth[~seen], "unseen")
    if threshold == 0.0:
        masked = Rt.texture_from_images(torus.vertices, torus.triangles, torus.uvs,
                                        projection_matrices(torus.cams), images, torus.size,
                                        alpha_threshold=0.5)[1]
        assert (masked < weights).any()


def test_a_fit_started_at_the_truth_stays_there(torus):
    """Zero d_color gives a zero gradient, which gives a zero Adam update."""
    import fourier_feature_nets_amd as ffn
    got, log = ffn.fit_mesh_texture(torus.vertices, torus.triangles, torus.uvs, torus.truth,
                                    _exact_targets(torus), num_steps=6, learning_rate=1e-2,
                                    verbose=False)
    assert len(log) == 6 and [entry.step for entry in log] == list(range(6))
    assert all(entry.loss == 0.0 for entry in log), [entry.loss for entry in log]
    assert_bits(got, torus.truth, "texture")


def test_one_step_from_grey_is_the_step_done_by_hand_with_and_without_the_cache(torus):
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import mesh, ops
    from fourier_feature_nets_amd.cameras import projection_matrices
    grey = np.full(torus.size + (3,), 0.5, dtype=np.float32)
    train = torus.dataset
    got, log = ffn.fit_mesh_texture(torus.vertices, torus.triangles, torus.uvs, grey, train,
                                    num_steps=1, learning_rate=1e-2, cameras_per_step=2, seed=5,
                                    verbose=False)

    v, t = on_gpu(torus.vertices, "float32"), on_gpu(torus.triangles, "int32")
    uv = on_gpu(torus.uvs, "float32")
    data = on_gpu(grey, "float32").reshape(-1, 3)
    num_texels = data.shape[0]
    projections = projection_matrices(torus.cams)
    grads, weight = torch.empty_like(data), torch.empty((num_texels,), device="cuda")
    per = SIZE * SIZE
    pixels = torch.arange(per, dtype=torch.int64, device="cuda")
    chosen = torch.randperm(CAMERAS, generator=torch.Generator().manual_seed(5)).tolist()[:2]
    count = 2 * per
    for number, camera in enumerate(chosen):
        ids = mesh.rasterize_mesh(v, t, projections[camera], ref.ORIGIN, SIZE, SIZE, colors=v)[3]
        record = ops.mesh_raster_setup(v, t, projections[camera], SIZE, SIZE)[0]
        tap_texel, tap_weight = ops.mesh_texture_taps(record, ids, t, uv, torus.size[0],
                                                      torus.size[1], SIZE, SIZE)
        sorted_texels, order = torch.sort(tap_texel.reshape(-1), stable=True)
        color, alpha = ops.mesh_texture_gather(tap_texel, tap_weight, data)
        sums, d_color, _ = ops.mse_loss(color, alpha, train.colors, train.alphas,
                                        pixels + camera * per, 1.0 / (3 * count), 0.0)
        ops.mesh_texture_grad(sorted_texels, order.to(torch.int32), tap_weight, d_color,
                              num_texels, grads, weight, accumulate=number > 0)
        total = sums if number == 0 else total + sums
    loss = float(ops.loss_value(total, count, 0.0).item())
    exp_avg, exp_avg_sq = torch.zeros_like(data.view(-1)), torch.zeros_like(data.view(-1))
    ops.clip_adam(data.view(-1), grads.view(-1), exp_avg, exp_avg_sq, 1, 1e-2)
    data.clamp_(0, 1)
    assert log[0].loss == loss and loss > 0
    assert_bits(got, data.cpu().numpy().reshape(grey.shape), "texture after one step")
    assert (got != grey).any()

    # five steps: the cache changes nothing
    runs = [ffn.fit_mesh_texture(torus.vertices, torus.triangles, torus.uvs, grey, train,
                                 num_steps=5, learning_rate=1e-2, cameras_per_step=3, seed=5,
                                 alpha_threshold=0.5, cache_taps=cache, verbose=False)
            for cache in (True, False)]
    assert_bits(runs[0][0], runs[1][0], "cache_taps")
    assert [e.loss for e in runs[0][1]] == [e.loss for e in runs[1][1]]


def _psnr(torus, texture):
    import fourier_feature_nets_amd as ffn
    error = 0.0
    truth = torus.images[..., :3].astype(np.float64) / 255
    for index, cam in enumerate(torus.cams):
        taps = ffn.mesh_texture_taps(torus.vertices, torus.triangles, torus.uvs, cam, torus.size)
        frame = ffn.render_mesh_texture(taps, texture).color
        error += float(((frame.astype(np.float64) - truth[index].reshape(-1, 3)) ** 2).mean())
    return -10.0 * np.log10(error / len(torus.cams))


def test_100_steps_from_grey_improve_loss_and_psnr(torus, capsys):
    """Only the strict improvement is asserted; the values are printed."""
    import fourier_feature_nets_amd as ffn
    grey = np.full(torus.size + (3,), 0.5, dtype=np.float32)
    got, log = ffn.fit_mesh_texture(torus.vertices, torus.triangles, torus.uvs, grey,
                                    torus.dataset, val_dataset=torus.dataset, num_steps=100,
                                    learning_rate=1e-2, cameras_per_step=CAMERAS,
                                    report_interval=99, verbose=True)
    printed = capsys.readouterr().out
    assert "val_psnr:" in printed and "0000099" in printed
    before, after = _psnr(torus, grey), _psnr(torus, got)
    with capsys.disabled():
        print("texture fit from grey: loss %.6f -> %.6f, psnr %.3f -> %.3f dB (val_psnr %.3f -> "
              "%.3f)" % (log[0].loss, log[-1].loss, before, after, log[0].val_psnr,
                         log[99].val_psnr))
    assert len(log) == 100 and log[-1].loss < log[0].loss
    assert after > before and log[99].val_psnr > log[0].val_psnr
    assert np.isnan(log[50].val_psnr) and got.min() >= 0 and got.max() <= 1


def test_texture_mesh_script_in_a_fresh_process(torus, tmp_path):
    import fourier_feature_nets_amd as ffn
    data, source, target = (str(tmp_path / name) for name in ("torus.npz", "in.obj", "out.obj"))
    np.savez(data, images=torus.images, intrinsics=torus.intrinsics, extrinsics=torus.poses,
             bounds=torus.bounds, split_counts=np.array([CAMERAS - 1, 1, 0], np.int32))
    flat, _, _, _ = ffn.procedural_torus(rings=16, sides=8)
    triangles = ffn.procedural_torus(rings=16, sides=8)[1]
    triangles = np.ascontiguousarray(triangles.reshape(2, -1, 3).transpose(1, 0, 2).reshape(-1, 3))
    ffn.save_obj(source, ffn.normalize_points(flat), triangles)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "texture_mesh.py"), source,
                          data, target, "--tile", "4", "--init", "images", "--fit", "20"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    found = dict(re.findall(r"^(before|after): train psnr ([0-9.+-]+)", out.stdout, re.M))
    assert set(found) == {"before", "after"}, out.stdout
    assert float(found["after"]) > float(found["before"])
    assert len(re.findall(r"held-out psnr ([0-9.+-]+)", out.stdout)) == 2, out.stdout
    # the OBJ loads with load_obj and renders with the existing textured path
    vertices, faces, uvs, texture = ffn.load_obj(target)
    assert texture.shape == (32, 64, 3) and texture.dtype == np.uint8
    assert vertices.shape == torus.vertices.shape and len(faces) == len(torus.triangles)
    np.testing.assert_array_equal(uvs.view(np.uint32), torus.uvs.view(np.uint32))
    frame, _ = ffn.render_mesh(vertices, faces, torus.cams[0], uvs=uvs, texture=texture)
    truth = torus.images[0, ..., :3].reshape(-1, 3).astype(np.float64) / 255
    error = float(((frame.color.astype(np.float64) - truth) ** 2).mean())
    assert -10 * np.log10(error) > float(found["before"])
    # --init colors on a mesh without vertex colours is refused before anything runs
    refused = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "texture_mesh.py"),
                              source, data, target, "--init", "colors"],
                             capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "colours" in refused.stderr
