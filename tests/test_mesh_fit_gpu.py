"""K32 on the GPU: the two kernels against the numpy restatement of their contract
(tests/mesh_raster_grad_reference.py) bit for bit, on the box sizes, placements and meshes the
contract names; the same bits over calls, chunk sizes and accumulation; the adjoint identity on the
device's own outputs; ``color_mesh_from_images`` and ``fit_mesh_colors`` on a tiny dataset that K31
draws here; scripts/color_mesh.py as a program."""

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
from tests import stream_order_cases_mesh_fit  # noqa: F401  (adds K32's stream-order cases)

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def on_gpu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def assert_bits(got, want, name):
    assert got.dtype == want.dtype and got.shape == want.shape, name
    np.testing.assert_array_equal(bits(got), bits(want), err_msg=name)


def view(width, height, **kwargs):
    from fourier_feature_nets_amd.cameras import projection_matrices
    return projection_matrices([ref.camera(width, height, **kwargs)])[0]


def noise(width, height, seed=0):
    return np.random.default_rng(seed).standard_normal((width * height, 3)).astype(np.float32)


def device_k32(vertices, triangles, proj, width, height, d_color, batch_size=1 << 22):
    """K31a-c for the ids, then K32a and K32b through the public wrappers -> numpy."""
    from fourier_feature_nets_amd import mesh, ops
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    record = ops.mesh_raster_setup(v, t, proj, width, height)[0]
    ids = mesh.rasterize_mesh(v, t, proj, ref.ORIGIN, width, height, colors=v,
                              batch_size=batch_size)[3]
    sums = ops.mesh_raster_face_sums(record, ids, on_gpu(d_color, "float32"), width, height)
    order, starts = mesh.vertex_adjacency(t, len(vertices))
    grad, weight = ops.mesh_vertex_gather(sums, order, starts)
    return types.SimpleNamespace(sums=sums.cpu().numpy(), grad=grad.cpu().numpy(),
                                 weight=weight.cpu().numpy(), ids=ids.cpu().numpy(),
                                 order=order.cpu().numpy(), starts=starts.cpu().numpy())


def both(vertices, triangles, proj, width, height, d_color=None):
    """The device against the restatement, bit for bit -> the device's results and the state."""
    if d_color is None:
        d_color = noise(width, height)
    got = device_k32(vertices, triangles, proj, width, height, d_color)
    state, ids = Rg.raster_ids(vertices, triangles, proj, width, height)
    np.testing.assert_array_equal(got.ids, ids)
    order, starts = Rg.adjacency(triangles, len(vertices))
    np.testing.assert_array_equal(got.order, order)
    np.testing.assert_array_equal(got.starts, starts)
    sums = Rg.face_sums(state, ids, d_color, width, height)
    grad, weight = Rg.vertex_gather(sums, order, starts)
    assert_bits(got.sums, sums, "face_sums")
    assert_bits(got.grad, grad, "grad")
    assert_bits(got.weight, weight, "weight")
    got.state = state
    return got


ONE = np.array([[0, 1, 2]], np.int32)
COVER = ref.flat([(-1, -1), (200, -1), (-1, 200)])           # covers every image up to 100 a side


@pytest.mark.parametrize("width,height", [(64, 64), (67, 33), (1, 1), (5, 3)])
def test_one_triangle_over_the_whole_image(width, height):
    """64 x 64: 4096 box pixels, 64 full segments; 67 x 33: 2211, a partial last segment."""
    out = both(COVER, ONE, ref.PIXEL_PROJ, width, height)
    assert out.state["counts"][0] == width * height and (out.ids == 0).all()
    # the weights of a pixel sum to 1 within a few roundings: a coarse check that all were added
    assert abs(float(out.weight.astype(np.float64).sum()) - width * height) < 1e-3 * width * height


def test_boxes_of_1_63_64_and_65_pixels():
    groups, x = [], 2.0
    for bw, bh in [(1, 1), (9, 7), (8, 8), (13, 5)]:
        # corners strictly inside the outermost pixels' cells: the box is bw x bh
        groups.append(ref.flat([(x - 0.25, 1.75), (x + bw - 0.75, 1.8), (x + 0.1, bh + 1.25)]))
        x += bw + 2
    vertices = np.concatenate(groups)
    triangles = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    out = both(vertices, triangles, ref.PIXEL_PROJ, 48, 24)
    assert out.state["counts"].tolist() == [1, 63, 64, 65]
    assert set(out.ids[out.ids >= 0].tolist()) == {0, 1, 2, 3}
    assert (out.sums[:, 9:].sum(1) > 0).all()


def test_a_sliver_without_a_centre_gives_a_zero_row():
    out = both(ref.SLIVER, ONE, ref.PIXEL_PROJ, 32, 32)
    assert out.state["counts"][0] == 20 and (out.ids == -1).all()
    assert not bits(out.sums).any() and not bits(out.grad).any() and not bits(out.weight).any()


def test_the_shared_diagonal_goes_to_the_lower_id():
    vertices, triangles = ref.quad_scene()
    out = both(vertices, triangles, ref.PIXEL_PROJ, 16, 14)
    image = out.ids.reshape(14, 16)
    assert (image[[3, 6, 9], [2, 6, 10]] == 0).all() and (out.ids == 1).any()
    # 63 covered pixels in all; each row's weights count its own pixels
    counts = [int((out.ids == f).sum()) for f in (0, 1)]
    assert sum(counts) == 63
    for f in (0, 1):
        assert abs(float(out.sums[f, 9:].astype(np.float64).sum()) - counts[f]) < 1e-3


def test_an_occluded_triangle_keeps_its_unoccluded_pixels_only():
    near = ref.flat([(4, 4), (12, 4), (4, 12)], 1.0)
    far = ref.flat([(2, 2), (20, 2), (2, 20)], 2.0)
    vertices = np.concatenate([far, near])
    triangles = np.arange(6, dtype=np.int32).reshape(2, 3)
    d_color = noise(24, 24)
    out = both(vertices, triangles, ref.PIXEL_PROJ, 24, 24, d_color)
    image = out.ids.reshape(24, 24)
    assert image[5, 5] == 1 and image[3, 3] == 0 and image[14, 4] == 0
    mine = int((out.ids == 0).sum())
    assert 0 < mine < int(out.state["counts"][0])
    assert abs(float(out.sums[0, 9:].astype(np.float64).sum()) - mine) < 1e-3
    # what lies behind the near triangle does not reach the far one's sums
    hidden = d_color.copy()
    hidden[out.ids == 1] += 100.0
    again = device_k32(vertices, triangles, ref.PIXEL_PROJ, 24, 24, hidden)
    assert_bits(again.sums[0], out.sums[0], "the far triangle's row")


def test_placements_give_zero_rows_and_stay_on_the_image():
    width, height = 64, 48
    vertices, triangles, expected = ref.placement_scene(width, height)
    out = both(vertices, triangles, ref.PIXEL_PROJ, width, height)
    np.testing.assert_array_equal(out.state["status"], expected)
    assert not bits(out.sums[expected != ref.DRAWN]).any()
    assert set(out.ids[out.ids >= 0].tolist()) == {0, 1, 2, 3, 13, 14}
    for f in (0, 1, 2, 3):                                    # the faces partly off the image
        assert out.sums[f, 9:].sum() > 0
    assert np.isfinite(out.sums).all() and np.isfinite(out.grad).all()


def test_257_triangles_on_300_shared_vertices():
    rng = np.random.default_rng(32)
    vertices = rng.uniform(-0.8, 0.8, (300, 3)).astype(np.float32)
    triangles = rng.integers(0, 300, (257, 3)).astype(np.int32)
    out = both(vertices, triangles, view(64, 48), 64, 48)
    assert (out.ids >= 0).mean() > 0.15 and np.diff(out.starts).max() >= 4


def _fan(valence, centre=(16.0, 16.0), radius=14.0):
    angle = 2 * np.pi * np.arange(valence + 1) / (valence + 1)
    rim = np.stack([centre[0] + radius * np.cos(angle), centre[1] + radius * np.sin(angle)], 1)
    k = np.arange(1, valence + 1)
    return (ref.flat(np.concatenate([[centre], rim])),
            np.stack([np.zeros_like(k), k, k + 1], 1).astype(np.int32))


def test_a_fan_of_valence_130_and_an_unreferenced_vertex():
    vertices, triangles = _fan(130)
    vertices = np.concatenate([vertices, ref.flat([(3, 3)])])        # no face uses the last
    out = both(vertices, triangles, ref.PIXEL_PROJ, 32, 32)
    assert out.starts[1] - out.starts[0] == 130 and out.starts[-1] == out.starts[-2]
    assert out.weight[0] > 1 and not bits(out.grad[-1]).any() and not bits(out.weight[-1]).any()
    assert (out.ids >= 0).sum() > 300


def test_a_perspective_scene_and_nan_behind_the_background():
    """``scene(3, 40)`` from ``camera(48, 40)``; then the same with NaN and infinities in d_color at
    every pixel no triangle owns: not read, so every output stays finite and the same."""
    vertices, triangles, _, _ = ref.scene(3, 40)
    d_color = noise(48, 40, 7)
    clean = both(vertices, triangles, view(48, 40), 48, 40, d_color)
    dirty = d_color.copy()
    dirty[clean.ids < 0] = [np.nan, np.inf, -np.inf]
    out = both(vertices, triangles, view(48, 40), 48, 40, dirty)
    for name in ("sums", "grad", "weight"):
        assert np.isfinite(getattr(out, name)).all(), name
        assert_bits(getattr(out, name), getattr(clean, name), name)


def _block_mesh():
    from tests.octree_mesh_cases import case
    from fourier_feature_nets_amd.octree import OcTree
    c = case("cuboid")
    tree = OcTree(c.scale, c.nodes, c.leaves, c.leaf_data, c.sh_degree)
    return tree.extract_mesh(placement="corners", center=(1.0, 0.25, -0.5))


def test_the_block_mesh_of_a_lattice_tree():
    surface = _block_mesh()
    out = both(np.asarray(surface.vertices, np.float32), np.asarray(surface.triangles, np.int32),
               view(64, 48, distance=4.5), 64, 48)
    assert (out.ids >= 0).sum() > 300 and np.diff(out.starts).max() >= 4


def test_the_same_bits_on_a_repeated_call_and_for_small_chunks():
    vertices, triangles, _, _ = ref.scene(0, 60)
    proj, d_color = view(64, 48), noise(64, 48, 3)
    first = device_k32(vertices, triangles, proj, 64, 48, d_color)
    for batch in (1 << 22, 97):
        again = device_k32(vertices, triangles, proj, 64, 48, d_color, batch_size=batch)
        for name in ("sums", "grad", "weight"):
            assert_bits(getattr(again, name), getattr(first, name), "%s, batch %d" % (name, batch))


def test_accumulate_adds_in_camera_order():
    from fourier_feature_nets_amd import render_mesh_backward, vertex_adjacency
    vertices, triangles, _, _ = ref.scene(3, 40)
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    cams = [ref.camera(48, 40, yaw=yaw) for yaw in (0.3, 1.3, 2.3)]
    d_colors = [on_gpu(noise(48, 40, 20 + k), "float32") for k in range(3)]
    adjacency = vertex_adjacency(t, len(vertices))
    alone = [render_mesh_backward(v, t, cam, g, adjacency) for cam, g in zip(cams, d_colors)]
    grad = torch.full((len(vertices), 3), 7.0, device="cuda")          # overwritten by the first
    weight = torch.full((len(vertices),), 7.0, device="cuda")
    for k, (cam, g) in enumerate(zip(cams, d_colors)):
        out = render_mesh_backward(v, t, cam, g, adjacency, grad, weight, accumulate=k > 0)
        assert out[0] is grad and out[1] is weight
    want_grad = (alone[0][0].cpu().numpy() + alone[1][0].cpu().numpy()) + alone[2][0].cpu().numpy()
    want_weight = (alone[0][1].cpu().numpy() + alone[1][1].cpu().numpy()) + alone[2][1].cpu().numpy()
    assert_bits(grad.cpu().numpy(), want_grad, "grad")
    assert_bits(weight.cpu().numpy(), want_weight, "weight")
    # numpy in, numpy out, the same bits
    host = render_mesh_backward(vertices, triangles, cams[0], d_colors[0].cpu().numpy())
    assert_bits(host[0], alone[0][0].cpu().numpy(), "numpy grad")


def test_adjoint_identity_on_the_devices_own_outputs():
    """The budget of tests/test_mesh_fit_cpu.py (``Rg.adjoint_budget``), on K31's image and K32's
    gradient as the device gives them."""
    from fourier_feature_nets_amd import render_mesh, render_mesh_backward
    vertices, triangles, colors, _ = ref.scene(3, 40)
    cam = ref.camera(48, 40)
    g = noise(48, 40, 11)
    image, ids, _ = render_mesh(vertices, triangles, cam, colors=colors, return_ids=True)
    grad, _ = render_mesh_backward(vertices, triangles, cam, g)
    hit = ids >= 0
    left = float((image.color[hit].astype(np.float64) * g[hit].astype(np.float64)).sum())
    right = float((colors.astype(np.float64) * grad.astype(np.float64)).sum())
    state, own = Rg.raster_ids(vertices, triangles, view(48, 40), 48, 40)
    np.testing.assert_array_equal(ids, own)
    budget = Rg.adjoint_budget(state, own, 48, colors, g, Rg.adjacency(triangles, len(vertices))[1])
    print("adjoint on the device: difference %.3g, budget %.3g, share %.3f"
          % (abs(left - right), budget, abs(left - right) / budget))
    assert abs(left - right) <= budget


# ------------------------------------------------------------------------------- stream order
@pytest.mark.parametrize("scenario", ["A", "B"])
@pytest.mark.parametrize("name", ["mesh_raster_face_sums", "mesh_vertex_gather"])
def test_k32_launches_on_the_callers_stream(name, scenario, monkeypatch):
    """The two cases of tests/stream_order_cases_mesh_fit.py under the harness of
    tests/test_stream_order_gpu.py, run from here as well: K32's share of the stream contract is
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
SIZE, CAMERAS = 32, 4


@pytest.fixture(scope="module")
def torus():
    """``procedural_torus(16, 8)`` with per-vertex colours, drawn by K31 from 4 cameras at 32 x 32:
    the uint8 images (alpha 255 where covered), the exact float frames, and an ``ImageDataset``."""
    import fourier_feature_nets_amd as ffn
    from bench import synthetic_rig
    vertices, triangles, _, _ = ffn.procedural_torus(rings=16, sides=8)
    vertices = ffn.normalize_points(vertices)
    colors = np.random.default_rng(16).uniform(0, 1, (len(vertices), 3)).astype(np.float32)
    intr, poses = synthetic_rig(CAMERAS, SIZE)
    cams = [ffn.CameraInfo.create("c%d" % i, ffn.Resolution(SIZE, SIZE), intr, p)
            for i, p in enumerate(poses)]
    images = np.zeros((CAMERAS, SIZE, SIZE, 4), np.uint8)
    frames = []
    for index, cam in enumerate(cams):
        color, alpha, _ = ffn.render_mesh_image(vertices, triangles, cam, colors=colors,
                                                include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.rint(255 * alpha)
        frames.append(ffn.render_mesh(vertices, triangles, cam, colors=colors)[0].color)
    assert 0.1 < (images[..., 3] > 0).mean() < 0.9
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset("torus", images, bounds, cams, 2, True, False)
    images.setflags(write=False)                     # shared by the tests below: not written into
    return types.SimpleNamespace(vertices=vertices, triangles=triangles, colors=colors, cams=cams,
                                 images=images, frames=np.stack(frames), dataset=dataset,
                                 intrinsics=np.stack([intr] * CAMERAS), poses=np.stack(poses),
                                 bounds=bounds)


def _exact_targets(torus):
    """The dataset with the float frames for targets: what K31 drew, not its bytes."""
    import fourier_feature_nets_amd as ffn
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset("exact", torus.images, torus.bounds, torus.cams, 2, True, False)
    dataset.colors = on_gpu(torus.frames.reshape(-1, 3), "float32")
    return dataset


@pytest.mark.parametrize("threshold", [0.5, 0.0])
def test_color_mesh_from_images_is_the_restatement(torus, threshold):
    """Alpha bytes of 100 in a window of every image: left out at 0.5 (128), kept at 0 (1)."""
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd.cameras import projection_matrices
    images = torus.images.copy()
    window = images[:, 10:20, 8:24, 3]
    window[window > 0] = 100
    data = types.SimpleNamespace(images=images, cameras=torus.cams, color_space="RGB")
    got, weights = ffn.color_mesh_from_images(torus.vertices, torus.triangles, data,
                                              alpha_threshold=threshold)
    want, want_weights = Rg.color_mesh(torus.vertices, torus.triangles,
                                       projection_matrices(torus.cams), images,
                                       alpha_threshold=threshold)
    assert_bits(weights, want_weights, "weights")
    assert_bits(got, want, "colors")
    seen = weights > 0
    # a seen vertex holds a mean with weights >= 0 of colours in [0, 1]
    assert seen.sum() > 50 and got[seen].min() >= 0.0 and got[seen].max() <= 1.0 + 1e-5
    # a vertex nobody saw keeps the colour it was given; tensors stay tensors
    given = on_gpu(torus.colors, "float32")
    kept, w = ffn.color_mesh_from_images(on_gpu(torus.vertices, "float32"),
                                         on_gpu(torus.triangles, "int32"), data, given,
                                         alpha_threshold=threshold)
    assert torch.is_tensor(kept) and kept.is_cuda
    assert_bits(w.cpu().numpy(), want_weights, "weights of the tensor call")
    assert_bits(kept.cpu().numpy()[seen], want[seen], "seen")
    assert_bits(kept.cpu().numpy()[~seen], torus.colors[~seen], "unseen")
    if threshold == 0.0:
        masked = Rg.color_mesh(torus.vertices, torus.triangles, projection_matrices(torus.cams),
                               images, alpha_threshold=0.5)[1]
        assert (masked < weights).any()


def test_a_fit_started_at_the_truth_stays_there(torus):
    """Zero d_color gives a zero gradient, which gives a zero Adam update."""
    import fourier_feature_nets_amd as ffn
    got, log = ffn.fit_mesh_colors(torus.vertices, torus.triangles, torus.colors,
                                   _exact_targets(torus), num_steps=6, learning_rate=1e-2,
                                   verbose=False)
    assert len(log) == 6 and [entry.step for entry in log] == list(range(6))
    assert all(entry.loss == 0.0 for entry in log), [entry.loss for entry in log]
    assert_bits(got, torus.colors, "colors")


def test_one_step_from_grey_is_the_step_done_by_hand(torus):
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import mesh, ops
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    grey = np.full((len(torus.vertices), 3), 0.5, dtype=np.float32)
    train = torus.dataset
    got, log = ffn.fit_mesh_colors(torus.vertices, torus.triangles, grey, train, num_steps=1,
                                   learning_rate=1e-2, cameras_per_step=2, seed=5, verbose=False)

    v, t = on_gpu(torus.vertices, "float32"), on_gpu(torus.triangles, "int32")
    data = on_gpu(grey, "float32")
    projections = projection_matrices(torus.cams)
    eyes = eye_positions(torus.cams, (0.0, 0.0, 0.0))
    order, starts = mesh.vertex_adjacency(t, len(torus.vertices))
    grads, weight = torch.empty_like(data), torch.empty((len(grey),), device="cuda")
    per = SIZE * SIZE
    pixels = torch.arange(per, dtype=torch.int64, device="cuda")
    chosen = torch.randperm(CAMERAS, generator=torch.Generator().manual_seed(5)).tolist()[:2]
    count = 2 * per
    for number, camera in enumerate(chosen):
        color, alpha, _, ids, _, _ = mesh.rasterize_mesh(v, t, projections[camera], eyes[camera],
                                                         SIZE, SIZE, colors=data)
        record = ops.mesh_raster_setup(v, t, projections[camera], SIZE, SIZE)[0]
        sums, d_color, _ = ops.mse_loss(color, alpha, train.colors, train.alphas,
                                        pixels + camera * per, 1.0 / (3 * count), 0.0)
        face_sums = ops.mesh_raster_face_sums(record, ids, d_color, SIZE, SIZE)
        ops.mesh_vertex_gather(face_sums, order, starts, grads, weight, accumulate=number > 0)
        total = sums if number == 0 else total + sums
    loss = float(ops.loss_value(total, count, 0.0).item())
    exp_avg, exp_avg_sq = torch.zeros_like(data.view(-1)), torch.zeros_like(data.view(-1))
    ops.clip_adam(data.view(-1), grads.view(-1), exp_avg, exp_avg_sq, 1, 1e-2)
    data.clamp_(0, 1)
    assert log[0].loss == loss and loss > 0
    assert_bits(got, data.cpu().numpy(), "colors after one step")
    assert (got != grey).any()


def _psnr(torus, colors):
    import fourier_feature_nets_amd as ffn
    error = 0.0
    truth = torus.images[..., :3].astype(np.float64) / 255
    for index, cam in enumerate(torus.cams):
        frame = ffn.render_mesh(torus.vertices, torus.triangles, cam, colors=colors)[0].color
        error += float(((frame.astype(np.float64) - truth[index].reshape(-1, 3)) ** 2).mean())
    return -10.0 * np.log10(error / len(torus.cams))


def test_100_steps_from_grey_improve_loss_and_psnr(torus, capsys):
    """Only the strict improvement is asserted; the values are printed."""
    import fourier_feature_nets_amd as ffn
    grey = np.full((len(torus.vertices), 3), 0.5, dtype=np.float32)
    got, log = ffn.fit_mesh_colors(torus.vertices, torus.triangles, grey, torus.dataset,
                                   val_dataset=torus.dataset, num_steps=100, learning_rate=1e-2,
                                   cameras_per_step=CAMERAS, report_interval=99, verbose=True)
    printed = capsys.readouterr().out
    assert "val_psnr:" in printed and "0000099" in printed
    before, after = _psnr(torus, grey), _psnr(torus, got)
    with capsys.disabled():
        print("fit from grey: loss %.6f -> %.6f, psnr %.3f -> %.3f dB (val_psnr %.3f -> %.3f)"
              % (log[0].loss, log[-1].loss, before, after, log[0].val_psnr, log[99].val_psnr))
    assert len(log) == 100 and log[-1].loss < log[0].loss
    assert after > before and log[99].val_psnr > log[0].val_psnr
    assert np.isnan(log[50].val_psnr) and got.min() >= 0 and got.max() <= 1


def test_color_mesh_script_in_a_fresh_process(torus, tmp_path):
    import fourier_feature_nets_amd as ffn
    data, source, target = (str(tmp_path / name) for name in ("torus.npz", "in.obj", "out.obj"))
    np.savez(data, images=torus.images, intrinsics=torus.intrinsics, extrinsics=torus.poses,
             bounds=torus.bounds, split_counts=np.array([CAMERAS, 0, 0], np.int32))
    ffn.save_obj(source, torus.vertices, torus.triangles)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "color_mesh.py"), source,
                          data, target, "--init", "images", "--fit", "20"],
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr
    found = dict(re.findall(r"^(before|after): mean psnr ([0-9.+-]+)", out.stdout, re.M))
    assert set(found) == {"before", "after"}, out.stdout
    assert float(found["after"]) > float(found["before"])
    vertices, triangles, _, _, colors = ffn.load_obj(target, return_colors=True)
    assert colors is not None and colors.shape == (len(torus.vertices), 3)
    assert vertices.shape == torus.vertices.shape and len(triangles) == len(torus.triangles)
    # a mesh without colours and without --init images is refused before anything runs
    refused = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "color_mesh.py"),
                              source, data, target, "--init", "given"],
                             capture_output=True, text=True, timeout=300)
    assert refused.returncode != 0 and "colours" in refused.stderr
