"""The explicit-buffer fits across an epoch boundary with a short last batch, replayed by hand from
the public pieces, bit for bit: ``fit_mesh_colors`` and ``fit_mesh_texture`` on the 4-camera torus
of their own test files (3 cameras a step: 3, then the 1 left over, then 3 of a fresh deal), and
``fit_octree`` / ``fit_octree_sh`` on the 700 rays of tests/test_octree_dist_gpu.py's ``fit_setup``
(256 a step: 256, 256, 188, then a fresh shuffle) with both priors on.  The one-step tests of those
files hold the first step; these hold what a loop can get wrong after it: the count of a short
batch, the second draw of the same generator, the Adam moments and the step number carried over."""

import numpy as np
import pytest
import torch

from tests.test_mesh_fit_gpu import torus as vertex_torus  # noqa: F401  (a fixture)
from tests.test_mesh_texture_gpu import torus as atlas_torus  # noqa: F401  (a fixture)
from tests.test_octree_dist_gpu import bits, fit_setup

pytestmark = pytest.mark.gpu

SIZE, CAMERAS = 32, 4


def on_gpu(x, dtype):
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def _vertex_pieces(torus):
    """-> (fit, start, forward, transpose) of the vertex colours, as
    tests/test_mesh_fit_gpu.py's one step composes them."""
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import mesh, ops
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    v, t = on_gpu(torus.vertices, "float32"), on_gpu(torus.triangles, "int32")
    projections = projection_matrices(torus.cams)
    eyes = eye_positions(torus.cams, (0.0, 0.0, 0.0))
    order, starts = mesh.vertex_adjacency(t, len(torus.vertices))

    def fit(start, **kwargs):
        return ffn.fit_mesh_colors(torus.vertices, torus.triangles, start, torus.dataset, **kwargs)

    def forward(camera, data):
        color, alpha, _, ids, _, _ = mesh.rasterize_mesh(v, t, projections[camera], eyes[camera],
                                                         SIZE, SIZE, colors=data)
        record = ops.mesh_raster_setup(v, t, projections[camera], SIZE, SIZE)[0]
        return color, alpha, (record, ids)

    def transpose(ctx, d_color, grads, weight, accumulate):
        face_sums = ops.mesh_raster_face_sums(ctx[0], ctx[1], d_color, SIZE, SIZE)
        ops.mesh_vertex_gather(face_sums, order, starts, grads, weight, accumulate=accumulate)

    return fit, np.full((len(torus.vertices), 3), 0.5, dtype=np.float32), forward, transpose


def _atlas_pieces(torus):
    """The same of the texture, as tests/test_mesh_texture_gpu.py's one step composes them."""
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import mesh, ops
    from fourier_feature_nets_amd.cameras import projection_matrices
    from tests import mesh_raster_reference as ref
    v, t = on_gpu(torus.vertices, "float32"), on_gpu(torus.triangles, "int32")
    uv = on_gpu(torus.uvs, "float32")
    projections = projection_matrices(torus.cams)
    num_texels = torus.size[0] * torus.size[1]

    def fit(start, **kwargs):
        return ffn.fit_mesh_texture(torus.vertices, torus.triangles, torus.uvs, start,
                                    torus.dataset, **kwargs)

    def forward(camera, data):
        ids = mesh.rasterize_mesh(v, t, projections[camera], ref.ORIGIN, SIZE, SIZE, colors=v)[3]
        record = ops.mesh_raster_setup(v, t, projections[camera], SIZE, SIZE)[0]
        tap_texel, tap_weight = ops.mesh_texture_taps(record, ids, t, uv, torus.size[0],
                                                      torus.size[1], SIZE, SIZE)
        sorted_texels, order = torch.sort(tap_texel.reshape(-1), stable=True)
        color, alpha = ops.mesh_texture_gather(tap_texel, tap_weight, data)
        return color, alpha, (sorted_texels, order.to(torch.int32), tap_weight)

    def transpose(ctx, d_color, grads, weight, accumulate):
        ops.mesh_texture_grad(ctx[0], ctx[1], ctx[2], d_color, num_texels, grads, weight,
                              accumulate=accumulate)

    return fit, np.full(torus.size + (3,), 0.5, dtype=np.float32), forward, transpose


@pytest.mark.parametrize("kind", ["colors", "texture"])
def test_mesh_fits_across_an_epoch_with_a_camera_left_over(kind, request):
    from fourier_feature_nets_amd import ops
    torus = request.getfixturevalue("vertex_torus" if kind == "colors" else "atlas_torus")
    fit, start, forward, transpose = (_vertex_pieces if kind == "colors" else _atlas_pieces)(torus)
    got, log = fit(start, num_steps=3, learning_rate=1e-2, cameras_per_step=3, seed=5,
                   alpha_threshold=0.5, verbose=False)

    generator = torch.Generator().manual_seed(5)
    first = torch.randperm(CAMERAS, generator=generator).tolist()
    second = torch.randperm(CAMERAS, generator=generator).tolist()
    batches = [first[:3], first[3:], second[:3]]
    assert [len(chosen) for chosen in batches] == [3, 1, 3]
    train = torus.dataset
    data = on_gpu(start, "float32").reshape(-1, 3)
    grads, weight = torch.empty_like(data), torch.empty((data.shape[0],), device="cuda")
    exp_avg, exp_avg_sq = torch.zeros_like(data.view(-1)), torch.zeros_like(data.view(-1))
    per = SIZE * SIZE
    pixels = torch.arange(per, dtype=torch.int64, device="cuda")
    losses = []
    for k, chosen in enumerate(batches):
        count = len(chosen) * per
        for number, camera in enumerate(chosen):
            color, alpha, ctx = forward(camera, data)
            sums, d_color, _ = ops.mse_loss(color, alpha, train.colors, train.alphas,
                                            pixels + camera * per, 1.0 / (3 * count), 0.0)
            # alpha_threshold 0.5 is the byte 128
            kept = torch.from_numpy(torus.images[camera][..., 3].reshape(-1, 1) >= 128).cuda()
            d_color = torch.where(kept, d_color, torch.zeros_like(d_color))
            transpose(ctx, d_color, grads, weight, number > 0)
            total = sums if number == 0 else total + sums
        losses.append(float(ops.loss_value(total, count, 0.0).item()))
        ops.clip_adam(data.view(-1), grads.view(-1), exp_avg, exp_avg_sq, k + 1, 1e-2)
        data.clamp_(0, 1)
    print("%s: losses %s by hand, %s logged" % (kind, losses, [entry.loss for entry in log]))
    assert [entry.loss for entry in log] == losses and min(losses) > 0
    want = data.cpu().numpy().reshape(start.shape)
    assert got.dtype == want.dtype and got.shape == want.shape
    assert np.array_equal(bits(got), bits(want))
    assert (got != start).any()


@pytest.mark.parametrize("degree", [None, 1])
def test_octree_fits_across_an_epoch_with_a_short_last_batch(degree):
    import fourier_feature_nets as ffn
    from fourier_feature_nets_amd import octree_fit, ops
    c, begin, dataset = fit_setup(degree)
    batch, steps, seed, dist_weight, eps = 256, 5, 77, 0.05, 0.02
    tv_weight = (0.5, 0.25) if degree is None else (0.5, 0.125, 0.25)
    fit = ffn.fit_octree if degree is None else ffn.fit_octree_sh
    fitted, log = fit(begin, dataset, None, batch_size=batch, num_steps=steps, seed=seed,
                      tv_weight=tv_weight, tv_eps=eps, dist_weight=dist_weight, verbose=False)

    sampler = dataset.sampler
    num_rays = len(c.starts)
    assert num_rays % batch != 0 and steps > -(-num_rays // batch)
    field = (ffn.OctreeField if degree is None else ffn.OctreeSHField)(begin, begin.center, "cuda")
    data = field.data.detach()
    flat = data.view(-1)
    grads = torch.empty_like(data)
    exp_avg, exp_avg_sq = torch.zeros_like(flat), torch.zeros_like(flat)
    scratch = torch.empty(((flat.numel() + 1023) // 1024,), dtype=torch.float32, device="cuda")
    shift = torch.tensor(field.center, dtype=torch.float32, device="cuda")
    aw = float(dataset.alpha_weight)
    generator = torch.Generator(device="cuda")
    generator.manual_seed(seed)
    losses, counts = [], []
    while len(losses) < steps:
        order = torch.randperm(num_rays, generator=generator, device="cuda")
        for start in range(0, num_rays, batch):
            if len(losses) == steps:
                break
            rays = order[start:start + batch]
            count = int(rays.numel())
            starts = (sampler.starts[rays] - shift).contiguous()
            directions = sampler.directions[rays].contiguous()
            color, alpha, _ = field._render(data, starts, directions, 0.0, (0.0, 0.0, 0.0), 0.0)
            sums, d_color, d_alpha = ops.mse_loss(color, alpha, dataset.colors, dataset.alphas,
                                                  rays, 1.0 / (3 * count), aw / count)
            field.backward(starts, directions, d_color, d_alpha, 0.0, (0.0, 0.0, 0.0), 0.0,
                           data=data, out=grads, dist_scale=dist_weight / count,
                           ray_distortion=torch.empty((count,), device="cuda"))
            field.tv_backward(tv_weight, eps, data=data, out=grads, accumulate=True)
            ops.clip_adam(flat, grads.view(-1), exp_avg, exp_avg_sq, len(losses) + 1,
                          octree_fit.LEARNING_RATE, clip_value=octree_fit.CLIP_VALUE,
                          max_norm=octree_fit.MAX_NORM, scratch=scratch)
            field._project(data)
            losses.append(ops.loss_value(sums, count, aw))
            counts.append(count)
    assert counts == [256, 256, 188, 256, 256]
    print("degree %s: losses %s" % (degree, [float(loss.item()) for loss in losses]))
    assert [entry.step for entry in log] == list(range(steps))
    assert np.array_equal(bits([entry.loss for entry in log]), bits(torch.stack(losses)))
    assert np.array_equal(bits(field.tree().leaf_data()), bits(fitted.leaf_data()))
    assert not np.array_equal(bits(fitted.leaf_data()), bits(begin.leaf_data()))
