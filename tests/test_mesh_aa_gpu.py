"""K34 on the GPU: the four kernels against the numpy restatement of their contract
(tests/mesh_aa_reference.py) bit for bit, on the sizes, placements and meshes the contract names;
the same bits over calls, chunk sizes and accumulation; the adjoint identity on the device's own
outputs; ``fit_mesh_geometry`` on a tiny dataset that K31 draws here; scripts/fit_mesh.py as a
program."""

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

from tests import mesh_aa_reference as A
from tests import mesh_raster_reference as ref
from tests import stream_order_cases_mesh_aa  # noqa: F401  (adds K34's stream-order cases)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24


def on_gpu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def assert_bits(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=name)


def view(width, height, **kwargs):
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    cam = ref.camera(width, height, **kwargs)
    return projection_matrices([cam])[0], eye_positions([cam], (0.0, 0.0, 0.0))[0]


def noise(width, height, seed=0):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((width * height, 3)).astype(np.float32),
            rng.standard_normal(width * height).astype(np.float32))


def device_k34(vertices, triangles, proj, eye, width, height, colors, g, batch_size=1 << 22,
               grad=None, background=(0, 0, 0)):
    """K31, then K34a, K34b, the sort and K34c through the public wrappers -> numpy."""
    from fourier_feature_nets_amd import mesh, ops
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    opposite = mesh.edge_opposites(t, len(vertices))
    record, color, alpha, _, ids, _, _, zbuf = mesh._rasterize_z(
        v, t, proj, eye, width, height, on_gpu(colors, "float32"), background=background,
        batch_size=batch_size)
    out_color, out_alpha = ops.mesh_aa_forward(record, zbuf, ids, opposite, v, proj, color, alpha,
                                               width, height)
    d_color, d_alpha, entry_vertex, entry_grad = ops.mesh_aa_backward(
        record, zbuf, ids, opposite, v, t, proj, color, alpha, on_gpu(g[0], "float32"),
        on_gpu(g[1], "float32"), width, height)
    sorted_vertex, order = torch.sort(entry_vertex, stable=True)
    accumulate = grad is not None
    grad = ops.mesh_aa_vertex_grad(sorted_vertex.contiguous(), order.to(torch.int32).contiguous(),
                                   entry_grad, v, proj, None if grad is None else on_gpu(grad, "float32"),
                                   accumulate)
    names = dict(ids=ids, zbuf=zbuf, color=color, alpha=alpha, out_color=out_color,
                 out_alpha=out_alpha, d_color=d_color, d_alpha=d_alpha, entry_vertex=entry_vertex,
                 entry_grad=entry_grad, grad=grad, opposite=opposite,
                 sorted_vertex=sorted_vertex, order=order.to(torch.int32))
    return types.SimpleNamespace(**{k: x.cpu().numpy() for k, x in names.items()})


OUTPUTS = ("out_color", "out_alpha", "d_color", "d_alpha", "entry_grad", "grad")


def both(vertices, triangles, proj, eye, width, height, colors=None, g=None, grad=None,
         background=(0, 0, 0)):
    """The device against the restatement, bit for bit -> the device's results, the restatement's
    frame and decisions."""
    colors = ref.grey(vertices, 5) if colors is None else colors
    g = noise(width, height) if g is None else g
    got = device_k34(vertices, triangles, proj, eye, width, height, colors, g, grad=grad,
                     background=background)
    opposite = A.opposites_brute(triangles, len(vertices)) if len(triangles) <= 64 else got.opposite
    np.testing.assert_array_equal(got.opposite, opposite)
    want_grad, d_color, d_alpha, fr, made, (entry_vertex, entry_grad) = A.geometry_backward(
        vertices, triangles, proj, eye, width, height, colors, opposite, g[0], g[1], grad,
        background)
    np.testing.assert_array_equal(got.ids, fr["ids"])
    np.testing.assert_array_equal(got.zbuf.view(np.uint64), fr["zbuf"])
    out_color, out_alpha = A.forward(fr, made)
    np.testing.assert_array_equal(got.entry_vertex, entry_vertex)
    sorted_vertex, order = A.sort_entries(entry_vertex)
    np.testing.assert_array_equal(got.sorted_vertex, sorted_vertex)
    np.testing.assert_array_equal(got.order, order)
    for name, want in zip(OUTPUTS, (out_color, out_alpha, d_color, d_alpha, entry_grad, want_grad)):
        assert_bits(getattr(got, name), want, name)
    got.frame, got.made = fr, made
    got.active = sum(pair is not None for pair in made)
    return got


def flat_scene(seed, count, width, height, shared=None):
    """``count`` triangles under PIXEL_PROJ with corners on a 1/4 px grid around the image, at three
    depths; with ``shared`` they draw their corners from that many common vertices."""
    rng = np.random.default_rng(seed)
    total = 3 * count if shared is None else shared
    points = np.stack([rng.integers(-8, 4 * width + 8, total), rng.integers(-8, 4 * height + 8, total)],
                      1) / 4.0
    depth = rng.choice([1.0, 1.5, 2.0], total)
    vertices = np.concatenate([points * depth[:, None], depth[:, None]], 1).astype(np.float32)
    triangles = np.arange(3 * count).reshape(-1, 3) if shared is None \
        else rng.integers(0, shared, (count, 3))
    return vertices, triangles.astype(np.int32)


# ------------------------------------------------------------------------------- shapes
@pytest.mark.parametrize("width,height", [(1, 1), (7, 9), (8, 8), (5, 13), (15, 17), (16, 16),
                                          (257, 1), (1, 48), (48, 1)])
def test_pixel_counts_at_the_wave_and_block_edges(width, height):
    """1, 63, 64, 65, 255, 256 and 257 pixels; 1 x 48 has no axis-0 pair and 48 x 1 no axis-1 one."""
    vertices, triangles = flat_scene(width * 100 + height, 6, width, height)
    out = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, width, height)
    if width * height > 1:
        assert out.active > 0
    if width == 1:
        assert (out.entry_vertex.reshape(-1, 4)[:, :2] == len(vertices)).all()
    if height == 1:
        assert (out.entry_vertex.reshape(-1, 4)[:, 2:] == len(vertices)).all()


@pytest.mark.parametrize("count", [1, 2, 64, 257])
def test_1_to_257_triangles_at_65_by_48(count):
    if count == 257:
        rng = np.random.default_rng(32)
        vertices = rng.uniform(-0.8, 0.8, (300, 3)).astype(np.float32)
        triangles = rng.integers(0, 300, (257, 3)).astype(np.int32)
        colors = None
    else:
        vertices, triangles, colors, _ = ref.scene(40 + count, count)
    out = both(vertices, triangles, *view(65, 48), 65, 48, colors)
    assert out.active >= 8 and (out.ids >= 0).any()


def test_shared_vertices_under_the_pixel_projection():
    vertices, triangles = flat_scene(9, 40, 33, 21, shared=30)
    out = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, 33, 21)
    assert out.active > 50 and (out.opposite >= 0).any()


def test_placements_stay_on_the_image():
    """Off the image, behind, across w = 0, outside the guard band, NaN, degenerate, tied depths."""
    vertices, triangles, status = ref.placement_scene(64, 48)
    out = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, 64, 48)
    assert (out.frame["state"]["status"] == status).all()
    drawn = set(np.flatnonzero(status == ref.DRAWN).tolist())
    assert {pair["f"] for pair in out.made if pair is not None} <= drawn
    assert np.isfinite(out.grad).all() and out.active > 30


def test_an_empty_image_comes_back_bit_for_bit():
    vertices = ref.flat([(-30, -30), (-20, -30), (-25, -12)])
    triangles = np.array([[0, 1, 2]], np.int32)
    out = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, 21, 13, background=(0.25, 0.5, 0.75))
    assert out.active == 0 and (out.ids == -1).all()
    assert_bits(out.out_color, out.color, "color")
    assert_bits(out.out_alpha, out.alpha, "alpha")
    assert (out.entry_vertex == 3).all() and not bits(out.entry_grad).any()
    assert (out.grad == 0).all()


def test_a_nan_in_g_outside_every_active_pair_reaches_only_its_own_d():
    vertices, triangles, colors, _ = ref.scene(3, 40)
    proj, eye = view(48, 40)
    g = noise(48, 40, 7)
    clean = both(vertices, triangles, proj, eye, 48, 40, colors, g)
    used = np.zeros(48 * 40, dtype=bool)
    for pair in clean.made:
        if pair is not None:
            used[[pair["a"], pair["b"]]] = True
    assert 20 < (~used).sum() < used.size
    dirty = (g[0].copy(), g[1].copy())
    dirty[0][~used] = [np.nan, np.inf, -np.inf]
    dirty[1][~used] = np.nan
    out = both(vertices, triangles, proj, eye, 48, 40, colors, dirty)
    assert_bits(out.d_color[used], clean.d_color[used], "d_color")
    assert_bits(out.d_alpha[used], clean.d_alpha[used], "d_alpha")
    assert_bits(out.d_color[~used], dirty[0][~used], "its own d_color")
    for name in ("entry_grad", "grad", "out_color", "out_alpha"):
        assert np.isfinite(getattr(out, name)).all(), name
        assert_bits(getattr(out, name), getattr(clean, name), name)


def _fan(valence, centre=(16.0, 16.0), radius=14.0):
    angle = 2 * np.pi * np.arange(valence + 1) / (valence + 1)
    rim = np.stack([centre[0] + radius * np.cos(angle), centre[1] + radius * np.sin(angle)], 1)
    k = np.arange(1, valence + 1)
    return (ref.flat(np.concatenate([[centre], rim])),
            np.stack([np.zeros_like(k), k, k + 1], 1).astype(np.int32))


def test_a_fan_of_valence_130_and_an_unreferenced_vertex():
    """The whole fan: its spokes continue the surface, so only the rim and the two spokes at the
    fan's one gap are silhouettes.  Every other triangle of it: every spoke is a boundary and the
    centre's row in K34c is long."""
    vertices, triangles = _fan(130)
    vertices = np.concatenate([vertices, ref.flat([(3, 3)])])        # no face uses the last
    out = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, 32, 32)
    assert (out.entry_vertex == 0).sum() < 64 and out.active > 40
    assert (out.grad[-1] == 0).all()
    out = both(vertices, triangles[::2], ref.PIXEL_PROJ, ref.ORIGIN, 32, 32)
    assert (out.entry_vertex == 0).sum() > 256, (out.entry_vertex == 0).sum()
    assert (out.grad[-1] == 0).all() and (out.grad[0] != 0).any()


def _block_mesh():
    from tests.octree_mesh_cases import case
    from fourier_feature_nets_amd.octree import OcTree
    c = case("cuboid")
    tree = OcTree(c.scale, c.nodes, c.leaves, c.leaf_data, c.sh_degree)
    return tree.extract_mesh(placement="corners", center=(1.0, 0.25, -0.5))


def test_the_block_mesh_of_a_lattice_tree():
    surface = _block_mesh()
    vertices = np.asarray(surface.vertices, np.float32)
    triangles = np.asarray(surface.triangles, np.int32)
    out = both(vertices, triangles, *view(64, 48, distance=4.5), 64, 48)
    assert (out.ids >= 0).sum() > 300 and out.active > 40 and (out.opposite >= 0).mean() > 0.9
    # inside the blocks' faces the surface goes on: far fewer active pairs than id changes
    ids = out.ids.reshape(48, 64)
    changes = int((ids[:, 1:] != ids[:, :-1]).sum() + (ids[1:] != ids[:-1]).sum())
    assert out.active < changes


def test_the_same_bits_on_a_repeated_call_and_for_chunks_of_64_and_4096():
    vertices, triangles, colors, _ = ref.scene(0, 60)
    proj, eye = view(64, 48)
    g = noise(64, 48, 3)
    first = device_k34(vertices, triangles, proj, eye, 64, 48, colors, g)
    for batch in (1 << 22, 64, 4096):
        again = device_k34(vertices, triangles, proj, eye, 64, 48, colors, g, batch_size=batch)
        np.testing.assert_array_equal(again.entry_vertex, first.entry_vertex)
        for name in OUTPUTS:
            assert_bits(getattr(again, name), getattr(first, name), "%s, batch %d" % (name, batch))


def test_accumulate_adds_two_cameras_in_order():
    from fourier_feature_nets_amd import edge_opposites, render_mesh_geometry_backward
    vertices, triangles, colors, _ = ref.scene(3, 40)
    v, t, c = on_gpu(vertices, "float32"), on_gpu(triangles, "int32"), on_gpu(colors, "float32")
    cams = [ref.camera(48, 40, yaw=yaw) for yaw in (0.3, 1.3)]
    gs = [noise(48, 40, 20 + k) for k in range(2)]
    opposite = edge_opposites(t, len(vertices))
    alone = [render_mesh_geometry_backward(v, t, cam, c, on_gpu(g[0], "float32"),
                                           on_gpu(g[1], "float32"), opposite)
             for cam, g in zip(cams, gs)]
    grad = torch.full((len(vertices), 3), 7.0, device="cuda")          # overwritten by the first
    for k, (cam, g) in enumerate(zip(cams, gs)):
        out = render_mesh_geometry_backward(v, t, cam, c, on_gpu(g[0], "float32"),
                                            on_gpu(g[1], "float32"), opposite, grad,
                                            accumulate=k > 0)
        assert out[0] is grad
    assert_bits(grad.cpu().numpy(), alone[0][0].cpu().numpy() + alone[1][0].cpu().numpy(), "grad")
    # the restatement, accumulated the same way; numpy in, numpy out, the same bits
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    want = None
    for cam, g in zip(cams, gs):
        want, d_color = A.geometry_backward(
            vertices, triangles, projection_matrices([cam])[0],
            eye_positions([cam], (0.0, 0.0, 0.0))[0], 48, 40, colors,
            A.opposites_brute(triangles, len(vertices)), g[0], g[1], want)[:2]
    assert_bits(grad.cpu().numpy(), want, "grad of the restatement")
    host = render_mesh_geometry_backward(vertices, triangles, cams[1], colors, *gs[1])
    assert_bits(host[0], alone[1][0].cpu().numpy(), "numpy grad")
    assert_bits(host[1], d_color, "d_color_plain")


def test_the_laplacian_is_the_restatement():
    from fourier_feature_nets_amd import ops, vertex_neighbors
    rng = np.random.default_rng(50)
    for count, faces in ((1, 1), (257, 300), (300, 257)):
        triangles = rng.integers(0, count, (faces, 3)).astype(np.int32)
        values = rng.standard_normal((count, 3)).astype(np.float32)
        starts, neighbors = vertex_neighbors(on_gpu(triangles, "int32"), count)
        want_starts, want_neighbors = A.neighbors_brute(triangles, count)
        np.testing.assert_array_equal(starts.cpu().numpy(), want_starts)
        np.testing.assert_array_equal(neighbors.cpu().numpy(), want_neighbors)
        got = ops.mesh_laplacian(on_gpu(values, "float32"), starts, neighbors, 0.3)
        want = A.laplacian(values, want_starts, want_neighbors, 0.3)
        assert_bits(got.cpu().numpy(), want, "laplacian")
        again = ops.mesh_laplacian(on_gpu(values, "float32"), starts, neighbors, -1.7, got,
                                   accumulate=True)
        assert again is got
        assert_bits(got.cpu().numpy(), A.laplacian(values, want_starts, want_neighbors, -1.7, want),
                    "accumulated")
    # ids outside 0 .. V - 1 are skipped, rows are clamped into the array
    starts = torch.tensor([0, 2, 9], dtype=torch.int32, device="cuda")
    neighbors = torch.tensor([1, 5, 0, -1], dtype=torch.int32, device="cuda")
    values = on_gpu([[1, 2, 3], [5, 7, 11]], "float32")
    got = ops.mesh_laplacian(values, starts, neighbors).cpu().numpy()
    np.testing.assert_array_equal(got, [[-4, -5, -8], [4, 5, 8]])


def test_render_mesh_antialias_on_both_paths_and_under_supersampling():
    import fourier_feature_nets_amd as ffn
    vertices, triangles, colors, uvs = ref.scene(3, 20)
    cam = ref.camera(40, 30)
    proj, eye = view(40, 30)
    plain, plain_ids, _ = ffn.render_mesh(vertices, triangles, cam, colors=colors, return_ids=True)
    smooth, ids, _ = ffn.render_mesh(vertices, triangles, cam, colors=colors, return_ids=True,
                                     antialias=True)
    fr = A.frame(vertices, triangles, proj, eye, 40, 30, colors)
    want = A.forward(fr, A.decisions(fr, A.opposites_brute(triangles, len(vertices))))
    assert_bits(smooth.color, want[0], "color")
    assert_bits(smooth.alpha, want[1], "alpha")
    assert_bits(smooth.depth, plain.depth, "depth")
    np.testing.assert_array_equal(ids, plain_ids)
    assert ((smooth.alpha > 0) & (smooth.alpha < 1)).sum() > 20
    # the textured path: the same blend weights on K31c's textured colours
    texture = ref.texture(4, 16, 8, 3)
    textured, _ = ffn.render_mesh(vertices, triangles, cam, uvs=uvs, texture=texture,
                                  antialias=True)
    fr = A.frame(vertices, triangles, proj, eye, 40, 30, uvs=uvs, texture=texture[::-1])
    want = A.forward(fr, A.decisions(fr, A.opposites_brute(triangles, len(vertices))))
    assert_bits(textured.color, want[0], "textured color")
    assert_bits(textured.alpha, smooth.alpha, "textured alpha")
    # supersample 2: the pass runs on the 80 x 60 image, then the reduction
    fine, _ = ffn.render_mesh(vertices, triangles, cam, colors=colors, antialias=True,
                              supersample=2)
    coarse, _ = ffn.render_mesh(vertices, triangles, cam, colors=colors, supersample=2)
    assert fine.alpha.shape == (1200,) and (fine.alpha != coarse.alpha).any()
    image = ffn.render_mesh_image(vertices, triangles, cam, colors=colors, antialias=True)
    assert image.shape == (30, 40, 3) and image.dtype == np.uint8


def test_adjoint_identity_on_the_devices_own_outputs():
    """K34a is linear in (color, alpha) for fixed ids and z-buffer: <J delta, g> against
    <delta, J^T g> with J delta from K34a on delta and J^T g K34b's d, both as the device gives
    them.  Budget: an output is at most four blends of three roundings each on values of at most
    (1 + 4 * 0.5 * 2) = 5 times the largest input, so every element of J delta and of J^T g is off
    by at most 12 * 5 u times that; summed over the 4 P elements of both products:
    4 P * 120 u * max|delta| * max|g|."""
    from fourier_feature_nets_amd import mesh, ops
    vertices, triangles, colors, _ = ref.scene(3, 40)
    width, height = 48, 40
    proj, eye = view(width, height)
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    opposite = mesh.edge_opposites(t, len(vertices))
    record, _, _, _, ids, _, _, zbuf = mesh._rasterize_z(v, t, proj, eye, width, height,
                                                        on_gpu(colors, "float32"))
    delta, g = noise(width, height, 11), noise(width, height, 12)
    forward = ops.mesh_aa_forward(record, zbuf, ids, opposite, v, proj, on_gpu(delta[0], "float32"),
                                  on_gpu(delta[1], "float32"), width, height)
    back = ops.mesh_aa_backward(record, zbuf, ids, opposite, v, t, proj,
                                on_gpu(delta[0], "float32"), on_gpu(delta[1], "float32"),
                                on_gpu(g[0], "float32"), on_gpu(g[1], "float32"), width, height)
    j_delta = A.channels(forward[0].cpu().numpy(), forward[1].cpu().numpy()).astype(np.float64)
    jt_g = A.channels(back[0].cpu().numpy(), back[1].cpu().numpy()).astype(np.float64)
    g64, delta64 = A.channels(*g).astype(np.float64), A.channels(*delta).astype(np.float64)
    left, right = float((j_delta * g64).sum()), float((delta64 * jt_g).sum())
    budget = 4 * width * height * 120 * U * np.abs(delta64).max() * np.abs(g64).max()
    print("adjoint on the device: difference %.3g, budget %.3g, share %.4f"
          % (abs(left - right), budget, abs(left - right) / budget))
    assert (j_delta != delta64).any() and abs(left - right) <= budget


# ------------------------------------------------------------------------------- stream order
@pytest.mark.parametrize("scenario", ["A", "B"])
@pytest.mark.parametrize("name", ["mesh_aa_forward", "mesh_aa_backward", "mesh_aa_vertex_grad",
                                  "mesh_laplacian"])
def test_k34_launches_on_the_callers_stream(name, scenario, monkeypatch):
    """The four cases of tests/stream_order_cases_mesh_aa.py under the harness of
    tests/test_stream_order_gpu.py, run from here as well."""
    from fourier_feature_nets_amd import _lib
    from tests import stream_helpers as sh
    from tests.stream_order_cases import CASES
    case, = [c for c in CASES if c.name == name]
    hook = sh.Hook(_lib.call)
    monkeypatch.setattr(_lib, "call", hook)
    reached = sh.run_case(case, scenario, hook, monkeypatch)
    assert set(case.reaches) <= set(reached)


# ------------------------------------------------------------------------------- the tiny dataset
SIZE, CAMERAS = 32, 4


@pytest.fixture(scope="module")
def torus():
    """``procedural_torus(16, 8)`` with per-vertex colours, drawn by K31 from 4 cameras at 32 x 32:
    the uint8 images (alpha 255 where covered), the exact antialiased float frames, and an
    ``ImageDataset``: the dataset of tests/test_mesh_fit_gpu.py, rebuilt here."""
    import fourier_feature_nets_amd as ffn
    from bench import synthetic_rig
    vertices, triangles, _, _ = ffn.procedural_torus(rings=16, sides=8)
    vertices = ffn.normalize_points(vertices)
    colors = np.random.default_rng(16).uniform(0, 1, (len(vertices), 3)).astype(np.float32)
    intr, poses = synthetic_rig(CAMERAS, SIZE)
    cams = [ffn.CameraInfo.create("c%d" % i, ffn.Resolution(SIZE, SIZE), intr, p)
            for i, p in enumerate(poses)]
    images = np.zeros((CAMERAS, SIZE, SIZE, 4), np.uint8)
    frames, alphas = [], []
    for index, cam in enumerate(cams):
        color, alpha, _ = ffn.render_mesh_image(vertices, triangles, cam, colors=colors,
                                                include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.rint(255 * alpha)
        smooth = ffn.render_mesh(vertices, triangles, cam, colors=colors, antialias=True)[0]
        frames.append(smooth.color)
        alphas.append(smooth.alpha)
    assert 0.1 < (images[..., 3] > 0).mean() < 0.9
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset("torus", images, bounds, cams, 2, True, False)
    images.setflags(write=False)                     # shared by the tests below: not written into
    return types.SimpleNamespace(vertices=vertices, triangles=triangles, colors=colors, cams=cams,
                                 images=images, frames=np.stack(frames), alphas=np.stack(alphas),
                                 dataset=dataset, intrinsics=np.stack([intr] * CAMERAS),
                                 poses=np.stack(poses), bounds=bounds)


def _shrunk(torus, factor=0.9):
    centre = torus.vertices.mean(0, keepdims=True)
    return (centre + factor * (torus.vertices - centre)).astype(np.float32)


def test_a_fit_started_at_the_truth_does_not_raise_its_loss(torus):
    """The targets are the antialiased float frames of the truth: the loss is 0, its gradient is 0
    and the Adam update of a zero gradient is 0."""
    import fourier_feature_nets_amd as ffn
    with contextlib.redirect_stdout(io.StringIO()):
        exact = ffn.ImageDataset("exact", torus.images, torus.bounds, torus.cams, 2, True, False)
    exact.colors = on_gpu(torus.frames.reshape(-1, 3), "float32")
    exact.alphas = on_gpu(torus.alphas.reshape(-1), "float32")
    got, log = ffn.fit_mesh_geometry(torus.vertices, torus.triangles, torus.colors, exact,
                                     num_steps=6, learning_rate=1e-3, laplacian_weight=0.5,
                                     verbose=False)
    losses = [entry.loss for entry in log]
    print("fit at the truth: losses", losses)
    assert len(log) == 6 and losses[-1] <= losses[0]
    assert all(loss == 0.0 for loss in losses), losses
    assert_bits(got, torus.vertices, "vertices")


def test_one_step_is_the_step_done_by_hand(torus):
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import mesh, ops
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    start = _shrunk(torus)
    train = torus.dataset
    weight, bound = 0.25, 0.0008
    got, log = ffn.fit_mesh_geometry(start, torus.triangles, torus.colors, train, num_steps=1,
                                     learning_rate=1e-3, cameras_per_step=2, seed=5,
                                     laplacian_weight=weight, max_displacement=bound,
                                     verbose=False)

    v0, t = on_gpu(start, "float32"), on_gpu(torus.triangles, "int32")
    colors = on_gpu(torus.colors, "float32")
    data = v0.clone()
    projections = projection_matrices(torus.cams)
    eyes = eye_positions(torus.cams, (0.0, 0.0, 0.0))
    opposite = mesh.edge_opposites(t, len(start))
    starts, neighbors = mesh.vertex_neighbors(t, len(start))
    grads = torch.empty_like(data)
    per = SIZE * SIZE
    pixels = torch.arange(per, dtype=torch.int64, device="cuda")
    chosen = torch.randperm(CAMERAS, generator=torch.Generator().manual_seed(5)).tolist()[:2]
    count = 2 * per
    aw = float(train.alpha_weight)
    assert aw > 0
    for number, camera in enumerate(chosen):
        record, color, alpha, _, ids, _, _, zbuf = mesh._rasterize_z(
            data, t, projections[camera], eyes[camera], SIZE, SIZE, colors)
        smooth = ops.mesh_aa_forward(record, zbuf, ids, opposite, data, projections[camera], color,
                                     alpha, SIZE, SIZE)
        sums, g_color, g_alpha = ops.mse_loss(smooth[0], smooth[1], train.colors, train.alphas,
                                              pixels + camera * per, 1.0 / (3 * count), aw / count)
        _, _, entry_vertex, entry_grad = ops.mesh_aa_backward(
            record, zbuf, ids, opposite, data, t, projections[camera], color, alpha, g_color,
            g_alpha, SIZE, SIZE)
        sorted_vertex, order = torch.sort(entry_vertex, stable=True)
        ops.mesh_aa_vertex_grad(sorted_vertex.contiguous(), order.to(torch.int32).contiguous(),
                                entry_grad, data, projections[camera], grads, accumulate=number > 0)
        total = sums if number == 0 else total + sums
    ops.mesh_laplacian(data - v0, starts, neighbors, weight / len(start), grads, accumulate=True)
    loss = float(ops.loss_value(total, count, aw).item())
    exp_avg, exp_avg_sq = torch.zeros_like(data.view(-1)), torch.zeros_like(data.view(-1))
    ops.clip_adam(data.view(-1), grads.view(-1), exp_avg, exp_avg_sq, 1, 1e-3)
    data = torch.maximum(torch.minimum(data, v0 + bound), v0 - bound)
    assert log[0].loss == loss and loss > 0
    assert_bits(got, data.cpu().numpy(), "vertices after one step")
    moved = np.abs(got - start)
    assert (moved > 0).any() and moved.max() <= bound + 1e-6 and (moved >= bound - 1e-6).any()


def _measures(torus, vertices):
    """(mean squared colour error against the exact frames, silhouette IoU against the images' alpha,
    mean distance of the vertices from the truth)."""
    import fourier_feature_nets_amd as ffn
    errors, ious = [], []
    for index, cam in enumerate(torus.cams):
        out, ids, _ = ffn.render_mesh(vertices, torus.triangles, cam, colors=torus.colors,
                                      return_ids=True)
        truth = torus.images[index][..., 3].reshape(-1) > 0
        drawn = ids >= 0
        ious.append((drawn & truth).sum() / max((drawn | truth).sum(), 1))
        errors.append(float(((out.color - torus.frames[index]) ** 2).mean()))
    return (float(np.mean(errors)), float(np.mean(ious)),
            float(np.linalg.norm(vertices - torus.vertices, axis=1).mean()))


def test_100_steps_from_a_shrunk_torus_lower_the_loss(torus, capsys):
    """The vertices scaled by 0.9 about their centroid, 100 steps at the default arguments: only the
    mean training loss of the last 10 steps against that of the first 10 is asserted; the loss, the
    silhouette IoU and the mean vertex distance before and after are printed."""
    import fourier_feature_nets_amd as ffn
    start = _shrunk(torus)
    got, log = ffn.fit_mesh_geometry(start, torus.triangles, torus.colors, torus.dataset,
                                     num_steps=100)
    losses = [entry.loss for entry in log]
    before, after = _measures(torus, start), _measures(torus, got)
    with capsys.disabled():
        print("geometry fit: loss %.6f -> %.6f (first 10 %.6f, last 10 %.6f), image mse %.6f -> "
              "%.6f, silhouette iou %.4f -> %.4f, mean vertex distance %.5f -> %.5f"
              % (losses[0], losses[-1], np.mean(losses[:10]), np.mean(losses[-10:]), before[0],
                 after[0], before[1], after[1], before[2], after[2]))
    assert len(log) == 100 and np.isfinite(got).all()
    assert np.mean(losses[-10:]) < np.mean(losses[:10])


def test_fit_mesh_script_in_a_fresh_process(torus, tmp_path):
    import fourier_feature_nets_amd as ffn
    data, source, target = (str(tmp_path / name) for name in ("torus.npz", "in.obj", "out.obj"))
    np.savez(data, images=torus.images, intrinsics=torus.intrinsics, extrinsics=torus.poses,
             bounds=torus.bounds, split_counts=np.array([CAMERAS - 1, 1, 0], np.int32))
    ffn.save_obj(source, _shrunk(torus), torus.triangles)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fit_mesh.py"), source,
                          data, target, "--steps", "10", "--color-steps", "3",
                          "--laplacian-weight", "0.1", "--max-displacement", "0.05"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    found = dict((label, (float(a), float(b), float(c))) for label, a, b, c in re.findall(
        r"^(before|after): mean psnr ([0-9.+-]+), held-out psnr ([0-9.+-]+), silhouette iou "
        r"([0-9.]+)$", out.stdout, re.M))
    assert set(found) == {"before", "after"}, out.stdout
    assert re.search(r"^fit: 10 steps, loss [0-9.]+ -> [0-9.]+, mean displacement", out.stdout, re.M)
    vertices, triangles, _, _, colors = ffn.load_obj(target, return_colors=True)
    assert colors is not None and colors.shape == (len(torus.vertices), 3)
    assert vertices.shape == torus.vertices.shape and len(triangles) == len(torus.triangles)
    # (load_obj orders the vertices its own way: the clamp is read off the script's own report)
    largest = float(re.search(r"largest ([0-9.]+)$", out.stdout, re.M).group(1))
    assert 0 < largest <= 0.05 * np.sqrt(3) + 1e-4
    refused = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "fit_mesh.py"),
                              source, data, target, "--steps", "-1"],
                             capture_output=True, text=True, timeout=300)
    assert refused.returncode == 2 and "--steps" in refused.stderr
