"""K36 on the GPU: the four kernels of csrc/mesh_cast.hip against the numpy restatement of their
contract (tests/mesh_cast_reference.py), bit for bit on boxes, keys, nodes, hit ids, t, u, v, colour,
alpha and depth -- hipcc rounds f32 ``/`` correctly, so nothing needs a budget here; the float64
budgets are the CPU module's.  Then the shapes the contract names, the host functions
(``build_mesh_bvh``, ``cast_rays``, ``mesh_spans``, ``render_mesh_rays``, ``RaySampler.clip_to_mesh``)
and ``scripts/render_mesh.py --method rays`` as a program."""

import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from tests import mesh_cast_reference as C
from tests import mesh_raster_reference as ref
from tests import refusal_cases_mesh_cast  # noqa: F401  (the tables as the whole suite has them)
from tests import stream_order_cases_mesh_cast  # noqa: F401

pytestmark = pytest.mark.gpu

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SCENE = os.path.join(ROOT, "tests", "golden", "scene16.npz")
COUNTS = [1, 3, 4, 5, 63, 64, 65, 257, 300]
RAYS = 480


def on_gpu(x, dtype):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).cuda()


def bits(x):
    x = x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x)
    return x.view(np.uint32) if x.dtype == np.float32 else x


def assert_same(got, want, what=""):
    assert len(got) == len(want)
    for k, (g, w) in enumerate(zip(got, want)):
        g = g.cpu().numpy() if torch.is_tensor(g) else g
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k, g.dtype, w.dtype)
        np.testing.assert_array_equal(bits(g), bits(w), err_msg="%s output %d" % (what, k))


# ------------------------------------------------------------------------------- shared inputs
_MESHES, _RAYS, _WANT = {}, {}, {}


def mesh_of(count):
    if count not in _MESHES:
        vertices, triangles, colors, uvs = ref.scene(900 + count, count)
        _MESHES[count] = (vertices, triangles, colors, uvs)
    return _MESHES[count]


def rays_of(count):
    """480 rays: 300 random ones, 96 parallel to an axis, 72 whose origin lies on a box plane of
    the mesh's own tree, and 12 with a NaN, an infinite or an all-zero component."""
    if count not in _RAYS:
        vertices, triangles, _, _ = mesh_of(count)
        rng = np.random.default_rng(count)
        starts, directions = C.random_rays(1000 + count, RAYS)
        axis = rng.integers(0, 3, 96)
        directions[300:396] = 0.0
        directions[300 + np.arange(96), axis] = rng.choice([-1.0, 1.0, 0.5], 96)
        starts[300 + np.arange(96), axis] = -3.0 * np.sign(directions[300 + np.arange(96), axis])
        bvh = C.build(vertices, triangles, 4)
        planes = np.concatenate([bvh["boxes"], bvh["nodes"]])
        planes = planes[np.isfinite(planes).all(1)]
        rows, column = rng.integers(0, len(planes), 72), rng.integers(0, 6, 72)
        starts[396 + np.arange(72), column % 3] = planes[rows, column]
        directions[396:468:3, :][np.arange(24), (column % 3)[::3]] = 0.0
        starts[468, 0], starts[469, 2] = np.nan, np.inf
        directions[470, 1], directions[471, 0], directions[472] = np.nan, -np.inf, 0.0
        starts[473], directions[474] = np.nan, np.inf
        starts[475, 1], directions[476, 2] = -np.inf, np.inf
        _RAYS[count] = (starts, directions)
    return _RAYS[count]


def want_of(count, farthest, t_min=0.0):
    """The answer for ``rays_of(count)``, computed once: every triangle against every ray (what
    the tree gives for every ``leaf_size``, tests/test_mesh_cast_cpu.py)."""
    key = (count, farthest, t_min)
    if key not in _WANT:
        vertices, triangles, _, _ = mesh_of(count)
        _WANT[key] = C.brute(vertices, triangles, C.default_pad(vertices), *rays_of(count), t_min,
                             farthest)
    return _WANT[key]


def device_tree(vertices, triangles, leaf_size, order=None):
    """K36a and K36b through the wrappers, held to the restatement -> the tensors ``ops.mesh_cast``
    takes in front of the rays."""
    from fourier_feature_nets_amd import ops
    host = C.build(vertices, triangles, leaf_size, order=order)
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    boxes, keys = ops.mesh_cast_boxes(v, t, float(host["pad"]), host["grid_lo"],
                                      float(host["grid_scale"]))
    assert_same((boxes, keys), (host["boxes"], host["keys"]), "K36a")
    sorted_keys = torch.sort((keys.to(torch.int64) << 32)
                             | torch.arange(len(keys), device="cuda")).values
    if order is None:
        np.testing.assert_array_equal((sorted_keys & 0xFFFFFFFF).cpu().numpy(), host["order"])
    nodes = ops.mesh_cast_tree(boxes, on_gpu(host["order"], "int32"), leaf_size)
    assert_same((nodes,), (host["nodes"],), "K36b")
    assert nodes.shape[0] == (1 << ops.mesh_cast_levels(len(triangles), leaf_size)) - 1
    return nodes, boxes, on_gpu(host["order"], "int32"), v, t


# ------------------------------------------------------------------------------- bit for bit
@pytest.mark.parametrize("leaf_size", [1, 4, 8])
@pytest.mark.parametrize("count", COUNTS)
def test_the_cast_is_the_restatements_bit_for_bit(count, leaf_size):
    from fourier_feature_nets_amd import ops
    vertices, triangles, _, _ = mesh_of(count)
    starts, directions = rays_of(count)
    tree = device_tree(vertices, triangles, leaf_size)
    o, d = on_gpu(starts, "float32"), on_gpu(directions, "float32")
    for farthest in (False, True):
        got = ops.mesh_cast(*tree, o, d, leaf_size, 0.0, farthest)
        assert_same(got, want_of(count, farthest), "farthest" if farthest else "nearest")
        # the NaN, infinite and zero rays end (the walk has a trip bound) and miss
        assert (got[0][468:477] == -1).all() and not got[1][468:477].any()
    got = ops.mesh_cast(*tree, o, d, leaf_size, 1.5, False)
    assert_same(got, want_of(count, False, 1.5), "t_min")
    if count >= 63:
        assert int((want_of(count, False)[0] >= 0).sum()) > 100


@pytest.mark.parametrize("rays", [1, 63, 64, 65, 257, 480])
def test_every_number_of_rays(rays):
    from fourier_feature_nets_amd import ops
    vertices, triangles, _, _ = mesh_of(65)
    starts, directions = rays_of(65)
    pick = np.arange(RAYS)[::-1][:rays].copy()          # the odd rays first
    tree = device_tree(vertices, triangles, 4)
    for farthest in (False, True):
        got = ops.mesh_cast(*tree, on_gpu(starts[pick], "float32"),
                            on_gpu(directions[pick], "float32"), 4, 0.0, farthest)
        assert_same(got, [x[pick] for x in want_of(65, farthest)])


def test_ids_outside_the_vertices_are_clamped():
    from fourier_feature_nets_amd import ops
    vertices, triangles, _, _ = mesh_of(5)
    wild = triangles.copy()
    wild[1, 0], wild[3, 2], wild[4, 1] = -7, 10 ** 6, 15
    clamped = np.clip(wild, 0, len(vertices) - 1)
    starts, directions = rays_of(5)
    tree = device_tree(vertices, wild, 4)
    for farthest in (False, True):
        got = ops.mesh_cast(*tree, on_gpu(starts, "float32"), on_gpu(directions, "float32"), 4, 0.0,
                            farthest)
        assert_same(got, C.brute(vertices, clamped, C.default_pad(vertices), starts, directions,
                                 0.0, farthest))
    # ... and entries of order outside the triangles: the walk reads what the clamp leaves
    order = np.array([0, 9, -3, 2, 1], np.int32)
    host = C.build(vertices, clamped, 4, order=order)
    nodes = ops.mesh_cast_tree(tree[1], on_gpu(order, "int32"), 4)
    assert_same((nodes,), (host["nodes"],))
    got = ops.mesh_cast(nodes, tree[1], on_gpu(order, "int32"), tree[3], tree[4],
                        on_gpu(starts, "float32"), on_gpu(directions, "float32"), 4)
    assert_same(got, C.cast(host, vertices, clamped, starts, directions))


def test_repeated_calls_and_a_permuted_order_give_the_same_hits():
    """The same bits on every call; with the triangles renumbered at random the hits, mapped back,
    are the same (no two triangles of the scene are hit at one t by one ray, so no tie is broken
    the other way); with ``order`` random or reversed they are the same outright."""
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import ops
    vertices, triangles, _, _ = mesh_of(257)
    starts, directions = rays_of(257)
    o, d = on_gpu(starts, "float32"), on_gpu(directions, "float32")
    rng = np.random.default_rng(5)
    for farthest in (False, True):
        want = want_of(257, farthest)
        tree = device_tree(vertices, triangles, 4)
        first = ops.mesh_cast(*tree, o, d, 4, 0.0, farthest)
        for _ in range(3):
            assert_same(ops.mesh_cast(*tree, o, d, 4, 0.0, farthest), [x.cpu().numpy() for x in first])
        for order in (rng.permutation(257), np.arange(257)[::-1]):
            shuffled = device_tree(vertices, triangles, 4, order=order.astype(np.int32))
            assert_same(ops.mesh_cast(*shuffled, o, d, 4, 0.0, farthest), want)
        perm = rng.permutation(257)
        bvh = ffn.build_mesh_bvh(vertices, triangles[perm])
        hit = ffn.cast_rays(bvh, starts, directions, which="farthest" if farthest else "nearest")
        back = np.where(hit.triangles >= 0, perm[np.maximum(hit.triangles, 0)], -1).astype(np.int32)
        assert_same((back, hit.t, hit.u, hit.v), want)


# ------------------------------------------------------------------------------- the host functions
def test_build_cast_and_spans_through_the_host_functions():
    import fourier_feature_nets_amd as ffn
    vertices, triangles, _, _ = mesh_of(300)
    starts, directions = rays_of(300)
    host = C.build(vertices, triangles, 4)
    bvh = ffn.build_mesh_bvh(vertices, triangles)
    assert (bvh.levels, bvh.leaf_size, bvh.num_triangles) == (host["levels"], 4, 300)
    assert np.float32(bvh.pad) == host["pad"] and bvh.nodes.is_cuda
    assert_same((bvh.nodes, bvh.boxes, bvh.order), (host["nodes"], host["boxes"], host["order"]))
    near = ffn.cast_rays(bvh, starts, directions)
    far = ffn.cast_rays(bvh, starts, directions, which="farthest")
    assert isinstance(near.t, np.ndarray)                         # numpy in, numpy out
    assert_same(near, want_of(300, False))
    assert_same(far, want_of(300, True))
    as_tensors = ffn.cast_rays(bvh, on_gpu(starts, "float32"), on_gpu(directions, "float32"), 1.5)
    assert as_tensors.t.is_cuda
    assert_same(as_tensors, want_of(300, False, 1.5))
    # spans: the two casts, widened by the margin but not below t_min
    for t_min, margin in ((0.0, 0.0), (0.0, 0.125), (1.5, 0.25)):
        t_in, t_out, hit = ffn.mesh_spans(bvh, starts, directions, t_min, margin)
        first, last = want_of(300, False, t_min), C.brute(
            vertices, triangles, host["pad"], starts, directions, t_min, True)
        found = first[0] >= 0
        np.testing.assert_array_equal(hit, found)
        np.testing.assert_array_equal(found, last[0] >= 0)
        want_in = np.where(found, np.maximum(first[1] - F32(margin), F32(t_min)), F32(0))
        want_out = np.where(found, last[1] + F32(margin), F32(0))
        assert_same((t_in, t_out), (want_in.astype(F32), want_out.astype(F32)))
        assert (t_in <= t_out).all() and found.sum() > (100 if t_min == 0 else 50)
    with pytest.raises(ValueError, match="cast_rays: which"):
        ffn.cast_rays(bvh, starts, directions, which="any")
    with pytest.raises(ValueError, match="mesh_spans: margin"):
        ffn.mesh_spans(bvh, starts, directions, 0.0, -1.0)
    with pytest.raises(ValueError, match="cast_rays: starts"):
        ffn.cast_rays(bvh, starts[:, :2], directions)


TEXTURES = [(5, 7, 3), (1, 1, 3), (16, 9, 4)]


def test_shading_is_the_restatements_bit_for_bit_on_both_colour_paths():
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import ops
    vertices, triangles, colors, uvs = mesh_of(257)
    starts, directions = rays_of(257)
    hit, t, u, v = want_of(257, False)
    assert (hit >= 0).sum() > 100 and (hit < 0).sum() > 20
    device = [on_gpu(hit, "int32")] + [on_gpu(x, "float32") for x in (t, u, v)]
    tri = on_gpu(triangles, "int32")
    ground = (0.25, 0.5, 0.75)
    got = ops.mesh_cast_shade(*device, tri, on_gpu(colors, "float32"), None, None, ground)
    assert_same(got, C.shade(hit, t, u, v, triangles, colors=colors, background=ground), "colours")
    missed = got[1].cpu().numpy() == 0
    np.testing.assert_array_equal(missed, hit < 0)
    np.testing.assert_array_equal(got[0].cpu().numpy()[missed], np.float32([ground]).repeat(missed.sum(), 0))
    bvh = ffn.build_mesh_bvh(vertices, triangles)
    for number, shape in enumerate(TEXTURES):
        texture = ref.texture(60 + number, *shape)
        got = ops.mesh_cast_shade(*device, tri, None, on_gpu(uvs, "float32"),
                                  on_gpu(texture, "uint8"), ground)
        want = C.shade(hit, t, u, v, triangles, uvs=uvs, texture=texture, background=ground)
        assert_same(got, want, "texture %s" % (shape,))
        # render_mesh_rays takes the texture with row 0 at the top, as render_mesh does
        out = ffn.render_mesh_rays(bvh, starts, directions, uvs=uvs, texture=texture[::-1],
                                   background=ground)
        assert_same(tuple(out), want, "render_mesh_rays %s" % (shape,))
    out = ffn.render_mesh_rays(bvh, on_gpu(starts, "float32"), on_gpu(directions, "float32"),
                               colors=on_gpu(colors, "float32"))
    assert out.color.is_cuda
    assert_same(tuple(out), C.shade(hit, t, u, v, triangles, colors=colors))
    with pytest.raises(ValueError, match="render_mesh_rays: give"):
        ffn.render_mesh_rays(bvh, starts, directions)
    with pytest.raises(ValueError, match="render_mesh_rays: colors"):
        ffn.render_mesh_rays(bvh, starts, directions, colors=colors[:-1])


@pytest.mark.parametrize("seed,count", [(11, 40), (12, 150)])
def test_the_cast_sees_the_triangles_the_rasteriser_draws(seed, count):
    """``cast_rays`` on a camera's rays against ``render_mesh(..., return_ids=True)``: the same
    triangle on every pixel that ``undecided()`` does not set aside (the rasteriser snaps to 1/256
    pixel and orders by 1/w; the cast does neither)."""
    import fourier_feature_nets_amd as ffn
    width, height = 24, 20
    vertices, triangles, colors, _ = ref.scene(seed, count)
    cam = ref.camera(width, height)
    _, nearest, second = ref.raycast64(vertices, triangles, cam.intrinsics, cam.extrinsics, width,
                                       height)
    aside = ref.undecided(vertices, triangles, cam.intrinsics, cam.extrinsics, width, height,
                          nearest, second)
    assert aside.mean() <= 0.08
    _, ids, report = ffn.render_mesh(vertices, triangles, cam, colors=colors, return_ids=True)
    # (the rasteriser refuses none of them: the rest lie off the image)
    assert report["drawn"] + report["off_image"] == count and report["drawn"] > 0.9 * count
    hit = ffn.cast_rays(ffn.build_mesh_bvh(vertices, triangles), *C.camera_rays(cam))
    np.testing.assert_array_equal(hit.triangles[~aside], ids[~aside])
    assert (ids >= 0).mean() >= 0.45


def test_a_camera_inside_a_closed_box_sees_all_six_faces():
    """K31 has no near-plane clipping: from inside the box it draws the face in front of the
    camera and reports the four around it ``clipped``.  The cast has no camera plane."""
    import warnings

    import fourier_feature_nets_amd as ffn
    vertices, triangles = C.box_mesh(1.0)
    colors = ref.grey(vertices, 3)
    cam = ref.camera(24, 20, distance=0.0)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        _, report = ffn.render_mesh(vertices, triangles, cam, colors=colors)
    assert report["clipped"] == 8 and report["behind"] == 2 and report["drawn"] == 2
    bvh = ffn.build_mesh_bvh(vertices, triangles)
    rng = np.random.default_rng(4)
    directions = rng.normal(size=(600, 3)).astype(F32)
    directions[:6] = np.float32([[-1, 0, 0], [1, 0, 0], [0, -1, 0], [0, 1, 0], [0, 0, -1], [0, 0, 1]])
    starts = np.zeros_like(directions) + np.float32([0.125, -0.25, 0.375])
    out = ffn.render_mesh_rays(bvh, starts, directions, colors=colors, background=(1, 0, 1))
    hit = ffn.cast_rays(bvh, starts, directions)
    assert (out.alpha == 1).all() and (hit.triangles >= 0).all() and (out.depth > 0).all()
    assert (hit.triangles[:6] // 2).tolist() == [0, 1, 2, 3, 4, 5]
    assert set((hit.triangles // 2).tolist()) == set(range(6))
    assert_same(hit, C.brute(vertices, triangles, C.default_pad(vertices), starts, directions))
    # the hit point lies on the face the id names
    point = starts + hit.t[:, None] * directions
    face = hit.triangles // 2
    np.testing.assert_allclose(point[np.arange(600), face // 2], np.where(face % 2, 1.0, -1.0),
                               atol=1e-5)
    # from inside, the last hit is the first
    assert_same(ffn.cast_rays(bvh, starts, directions, which="farthest"), tuple(hit))


# ------------------------------------------------------------------------------- the sampler
def test_clip_to_mesh_on_a_small_sampler():
    import contextlib
    import io

    import fourier_feature_nets_amd as ffn
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset.load(SCENE, "train", 16, True, False, None, device="cuda")
    sampler = dataset.sampler
    vertices, triangles, _, _ = ffn.procedural_torus(24, 12, 8)
    vertices = (0.6 * ffn.normalize_points(vertices)).astype(F32)
    bvh = ffn.build_mesh_bvh(vertices, triangles)
    margin = 0.05
    before = [x.clone() for x in (sampler.starts, sampler.directions, sampler.near_far, sampler.valid)]
    clipped = sampler.clip_to_mesh(bvh, margin)
    for was, now in zip(before, (sampler.starts, sampler.directions, sampler.near_far, sampler.valid)):
        assert torch.equal(was, now)
    assert clipped is not sampler and len(clipped) == len(sampler)
    valid, old = clipped.valid != 0, sampler.valid != 0
    assert (valid <= old).all() and 0 < valid.sum().item() < old.sum().item()
    t_in, t_out, hit = ffn.mesh_spans(bvh, sampler.starts, sampler.directions, 0.0, margin)
    assert not valid[~hit].any()
    near, far = clipped.near_far
    assert torch.equal(near[valid], torch.maximum(sampler.near_far[0], t_in)[valid])
    assert torch.equal(far[valid], torch.minimum(sampler.near_far[1], t_out)[valid])
    assert (near < far)[valid].all()
    assert torch.equal(clipped.near_far[:, ~valid], sampler.near_far[:, ~valid])
    print("clip_to_mesh: %d of %d valid rays kept, mean span %.3f of %.3f"
          % (valid.sum().item(), old.sum().item(), (far - near)[valid].mean().item(),
             (sampler.near_far[1] - sampler.near_far[0])[valid].mean().item()))
    # every sample of a kept ray lies in its span
    index = clipped.valid_index(torch.arange(len(clipped), device="cuda"))
    assert index.numel() == int(valid.sum().item())
    samples = clipped.sample(index, None)
    assert (samples.t_values >= t_in[index, None]).all() and (samples.t_values <= t_out[index, None]).all()
    assert (samples.t_values >= near[index, None]).all() and (samples.t_values <= far[index, None]).all()
    # ... and the renderer runs under it, unchanged
    torch.manual_seed(7)
    mlp = ffn.PositionalFourierMLP(3, 4, 5.5, num_channels=64, embedding_size=48).to("cuda")
    caster = ffn.Raycaster(mlp)
    frame = caster.render_image(clipped, 0, 4096)
    full = caster.render_image(sampler, 0, 4096)
    assert frame.shape == full.shape == (sampler.image_height, sampler.image_width, 3)
    assert np.isfinite(frame).all()
    dropped = ~valid[:sampler.rays_per_camera].cpu().numpy()
    assert (frame.reshape(-1, 3)[dropped] == 0).all() and (full.reshape(-1, 3)[dropped] != 0).any()
    with pytest.raises(ValueError, match="clip_to_mesh: margin"):
        sampler.clip_to_mesh(bvh, -0.5)


# ------------------------------------------------------------------------------- the script
def test_render_mesh_py_casts_the_samplers_rays_in_a_fresh_process(tmp_path):
    """``render_mesh.py --method rays`` prints the lines of the default method and writes the frame
    ``render_mesh_rays`` gives for the dataset sampler's own rays."""
    import contextlib
    import io

    from PIL import Image

    import fourier_feature_nets_amd as ffn
    from tests.test_mesh_raster_gpu import run_script, write_textured_obj
    data = str(tmp_path / "torus.npz")
    run_script("make_mesh_npz.py", data, "--render", "mesh", "--size", "32", "--cameras", "3")
    vertices, triangles, uvs, texture = ffn.procedural_torus()
    obj, png, frames = str(tmp_path / "torus.obj"), str(tmp_path / "torus.png"), str(tmp_path / "out")
    write_textured_obj(obj, png, vertices, triangles, uvs, texture)
    text = run_script("render_mesh.py", obj, data, frames, "--normalize", "--texture", png,
                      "--method", "rays")
    assert "%d vertices, %d triangles, texture" % (len(vertices), len(triangles)) in text
    assert "camera 0 (" in text and "mean psnr over 1 cameras:" in text
    value = float(text.strip().rsplit(" ", 1)[-1])
    print("render_mesh.py --method rays: psnr %.3f" % value)
    frame = np.asarray(Image.open(os.path.join(frames, "frame_00000.png")))
    assert frame.shape == (32, 32, 3)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset.load(data, "val", 2, True, False, None, device="cuda")
    sampler = dataset.sampler
    loaded = ffn.load_obj(obj, png, return_colors=True)
    points = ffn.normalize_points(loaded[0], [0.0, 1.0, 0.0])
    out = ffn.render_mesh_rays(ffn.build_mesh_bvh(points, loaded[1]),
                               sampler.starts[:1024].contiguous(),
                               sampler.directions[:1024].contiguous(), uvs=loaded[2],
                               texture=loaded[3])
    image = ffn.ops.to_image(out.color.contiguous(), torch.arange(1024, device="cuda"), 32, 32)
    np.testing.assert_array_equal(frame, image.cpu().numpy())
    assert 0.05 < float(out.alpha.mean().item()) < 0.9
    # the options of the rasteriser are refused, not ignored
    bad = subprocess.run([sys.executable, os.path.join(ROOT, "scripts", "render_mesh.py"), obj, data,
                          frames, "--method", "rays", "--antialias"], capture_output=True, text=True,
                         timeout=300)
    assert bad.returncode == 1 and "--method raster" in bad.stderr
