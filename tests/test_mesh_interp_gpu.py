"""K35 on the GPU: the two kernels against the numpy restatement of their contract
(tests/mesh_interp_reference.py) bit for bit, at the smallest shapes where the organisation can go
wrong -- the segment edges of the wave loop, the waves-per-block and block edges, the grid-stride
loop entered twice, narrow and odd images, valences 0 and 65, a negative area, records that do not
belong to the image; ``render_mesh_geometry_backward(interior=True)`` as K34's restatement plus
K35's; one ``fit_mesh_geometry(interior=True)`` step done by hand; and the two stream-order cases
under both scenarios and under the guarded placement."""

import contextlib
import io
import types

import numpy as np
import pytest
import torch

from tests import mesh_aa_reference as A
from tests import mesh_interp_reference as I
from tests import mesh_raster_reference as ref
from tests import refusal_cases_mesh_interp  # noqa: F401  (adds K35's refusal rows)
from tests import stream_order_cases_mesh_interp  # noqa: F401  (adds K35's stream-order cases)

pytestmark = pytest.mark.gpu

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
    return cam, projection_matrices([cam])[0], eye_positions([cam], (0.0, 0.0, 0.0))[0]


def gradient(width, height, seed=0):
    return np.random.default_rng(seed).standard_normal((width * height, 3)).astype(np.float32)


def device_k35(vertices, triangles, proj, eye, width, height, colors, d_color, grad=None):
    """K31, then K35a and K35b through the public wrappers -> numpy (ids, face_grads, grad)."""
    from fourier_feature_nets_amd import mesh, ops
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    c = on_gpu(colors, "float32")
    record, _, _, _, ids, _, _, _ = mesh._rasterize_z(v, t, proj, eye, width, height, c)
    face_grads = ops.mesh_interp_face_grads(record, ids, on_gpu(d_color, "float32"), c, t, width,
                                            height)
    order, starts = mesh.vertex_adjacency(t, len(vertices))
    out = ops.mesh_interp_vertex_grad(face_grads, order, starts, v, proj,
                                      None if grad is None else on_gpu(grad, "float32"),
                                      grad is not None)
    return types.SimpleNamespace(ids=ids.cpu().numpy(), face_grads=face_grads.cpu().numpy(),
                                 grad=out.cpu().numpy(), order=order.cpu().numpy(),
                                 starts=starts.cpu().numpy(), record=record)


def both(vertices, triangles, proj, eye, width, height, colors=None, d_color=None, grad=None):
    """The device against the restatement, bit for bit -> the device's results and the state."""
    colors = ref.grey(vertices, 5) if colors is None else colors
    d_color = gradient(width, height) if d_color is None else d_color
    got = device_k35(vertices, triangles, proj, eye, width, height, colors, d_color, grad)
    state = ref.setup(vertices, triangles, proj, width, height)
    fr = A.frame(vertices, triangles, proj, eye, width, height, colors)
    np.testing.assert_array_equal(got.ids, fr["ids"])
    order, starts = I.adjacency(triangles, len(vertices))
    np.testing.assert_array_equal(got.order, order)
    np.testing.assert_array_equal(got.starts, starts)
    want = I.face_grads(state, fr["ids"], d_color, colors, width, height)
    assert_bits(got.face_grads, want, "face_grads")
    assert_bits(got.grad, I.vertex_grad(want, order, starts, vertices, proj, grad), "grad")
    got.state, got.winners = state, np.unique(fr["ids"][fr["ids"] >= 0])
    return got


def boxed(x0, y0, box_w, box_h, z=1.0):
    """A triangle under PIXEL_PROJ whose pixel box is box_w x box_h at (x0, y0)."""
    return ref.flat([(x0 - 0.5, y0 - 0.5), (x0 + box_w - 0.5, y0 - 0.375),
                     (x0 - 0.375, y0 + box_h - 0.5)], z)


# ------------------------------------------------------------------------------- the wave loop
@pytest.mark.parametrize("box_w,box_h", [(1, 1), (9, 7), (8, 8), (13, 5), (16, 8), (43, 3)],
                         ids=["1", "63", "64", "65", "128", "129"])
def test_the_segment_edges_of_the_wave_loop(box_w, box_h):
    width, height = 48, 48
    vertices, triangles = boxed(3, 2, box_w, box_h, 1.5), np.array([[0, 1, 2]], np.int32)
    got = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, width, height)
    assert got.state["counts"][0] == box_w * box_h and got.face_grads[0].all()


@pytest.mark.parametrize("count", [1, 4, 5, 257])
def test_the_waves_per_block_and_block_edges(count):
    width, height = 40, 31
    vertices, triangles, colors, _ = ref.scene(500 + count, count)
    _, proj, eye = view(width, height)
    got = both(vertices, triangles, proj, eye, width, height, colors)
    assert len(got.winners) >= min(count, 3)
    assert not got.face_grads[np.setdiff1d(np.arange(count), got.winners)].any()


def test_the_grid_stride_loop_entered_twice():
    """F = 4 * 2^16 + 2: the first wave of the first block and the second wave of it take a second
    triangle.  All but the first and the last two triangles lie off the image."""
    width, height = 16, 12
    count = 4 * (1 << 16) + 2
    off = ref.flat([(-30, -30), (-20, -30), (-25, -12)])
    vertices = np.tile(off, (count, 1))
    vertices[:3] = boxed(1, 1, 9, 7, 1.0)
    vertices[-6:-3] = boxed(5, 3, 8, 8, 2.0)
    vertices[-3:] = boxed(2, 6, 12, 5, 1.5)
    triangles = np.arange(3 * count, dtype=np.int32).reshape(-1, 3)
    colors = ref.grey(vertices, 6)
    d_color = gradient(width, height, 2)
    got = device_k35(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, width, height, colors, d_color)
    state = ref.setup(vertices, triangles, ref.PIXEL_PROJ, width, height)
    drawn = np.flatnonzero(state["status"] == ref.DRAWN)
    assert drawn.tolist() == [0, count - 2, count - 1]
    small = {key: value[drawn] for key, value in state.items()}
    ids = got.ids.copy()
    for new, old in enumerate(drawn):
        ids[got.ids == old] = new
    want = np.zeros((count, 9), np.float32)
    # (the rows of ``small`` still name their vertices in the full arrays)
    want[drawn] = I.face_grads(small, ids, d_color, colors, width, height)
    assert set(np.unique(got.ids).tolist()) == {-1, 0, count - 2, count - 1}
    assert_bits(got.face_grads, want, "face_grads")
    assert want[drawn].all(axis=1).all()
    moved = np.flatnonzero(got.grad.any(1))
    assert set(moved.tolist()) == set(triangles[drawn].reshape(-1).tolist())


@pytest.mark.parametrize("width", [1, 2, 63, 64, 65])
def test_images_from_1_x_48_to_65_x_48(width):
    height = 48
    vertices, triangles, colors, _ = ref.scene(600 + width, 9)
    _, proj, eye = view(width, height, focal=40.0)
    got = both(vertices, triangles, proj, eye, width, height, colors)
    assert len(got.winners) >= 1


# ------------------------------------------------------------------------------- meshes
def _fan(valence):
    """``valence`` triangles around vertex 0 (a cone seen from its tip's side), vertex 1 + valence
    + 1 used by nobody, under a perspective camera."""
    angles = np.linspace(0, 2 * np.pi, valence + 1)[:-1]
    ring = np.stack([0.7 * np.cos(angles), 0.7 * np.sin(angles), np.full(valence, 0.2)], 1)
    vertices = np.concatenate([[[0.05, -0.02, -0.3]], ring, [[0.3, 0.3, 0.0]]]).astype(np.float32)
    triangles = np.array([[0, 1 + i, 1 + (i + 1) % valence] for i in range(valence)], np.int32)
    return vertices, triangles


def test_valence_0_and_valence_65_and_accumulate():
    width, height = 33, 29
    vertices, triangles = _fan(65)
    _, proj, eye = view(width, height, yaw=0.0, pitch=0.0)
    got = both(vertices, triangles, proj, eye, width, height)
    assert got.starts[1] - got.starts[0] == 65 and got.starts[-1] - got.starts[-2] == 0
    assert got.grad[0].all() and not got.grad[-1].any() and len(got.winners) > 40
    start = np.random.default_rng(3).standard_normal(vertices.shape).astype(np.float32)
    again = both(vertices, triangles, proj, eye, width, height, grad=start)
    assert (again.grad != got.grad).any()
    assert_bits(again.face_grads, got.face_grads, "the same bits on every call")


def test_a_negative_area_triangle_and_its_mirror():
    """The same triangle with its winding reversed: sgn(A) is applied to the integers, so the rows
    of the corners that swapped places swap.  Only (q0 + q1) + q2 adds in another order: both
    rows lie within ``_entry_budget`` (tests/test_mesh_interp_cpu.py, without the
    central-difference term) of the same real numbers, so within the two budgets of each other."""
    from tests.test_mesh_interp_cpu import _entry_budget
    width, height = 20, 16
    one = ref.flat([(2.25, 1.5), (15.5, 3.0), (6.75, 13.25)], 1.25)
    colors = ref.grey(one, 2)
    d_color = gradient(width, height, 5)
    a = both(one, np.array([[0, 1, 2]], np.int32), ref.PIXEL_PROJ, ref.ORIGIN, width, height,
             colors, d_color)
    b = both(one, np.array([[0, 2, 1]], np.int32), ref.PIXEL_PROJ, ref.ORIGIN, width, height,
             colors, d_color)
    x, y = a.state["X"][0], a.state["Y"][0]
    assert (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]) > 0
    x, y = b.state["X"][0], b.state["Y"][0]
    assert (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0]) < 0
    assert a.face_grads[0].all()
    swapped = [0, 1, 2, 6, 7, 8, 3, 4, 5]
    budget_a, _ = _entry_budget(a.state, 0, a.ids, colors, d_color, width, height, 0.0)
    budget_b, _ = _entry_budget(b.state, 0, b.ids, colors, d_color, width, height, 0.0)
    difference = np.abs(b.face_grads[0][swapped].astype(np.float64) - a.face_grads[0])
    assert (difference <= budget_a + budget_b[swapped]).all()


def test_records_whose_box_does_not_belong_to_the_image():
    """Boxes that reach past the image on either side, or are turned inside out, are skipped:
    nothing outside the image is read and the row is +0.  (A box inside an image of at most
    16384 x 16384 pixels cannot hold more than 2^28: that bound is K32a's second line of defence.)"""
    from fourier_feature_nets_amd import ops
    width, height = 20, 16
    vertices = np.concatenate([boxed(2, 2, 9, 7), boxed(4, 3, 8, 8, 2.0), boxed(1, 5, 13, 5, 3.0),
                               boxed(3, 1, 6, 6, 4.0), boxed(8, 8, 5, 5, 0.5)])
    triangles = np.arange(15, dtype=np.int32).reshape(5, 3)
    colors = ref.grey(vertices, 7)
    d_color = gradient(width, height, 8)
    got = both(vertices, triangles, ref.PIXEL_PROJ, ref.ORIGIN, width, height, colors, d_color)
    record = got.record.clone()
    boxes = {0: (0, 0, width, 3), 1: (-1, 0, 4, 4), 2: (5, 6, 4, 9), 3: (0, 0, 16383, 16383)}
    for f, box in boxes.items():
        record[f, 9:13] = torch.tensor(box, dtype=torch.int32)
    ids = np.zeros(width * height, np.int32)             # every pixel claims triangle 0, then 1, ..
    for f in range(5):
        ids[f::5] = f
    rows = ops.mesh_interp_face_grads(record, on_gpu(ids, "int32"), on_gpu(d_color, "float32"),
                                      on_gpu(colors, "float32"), on_gpu(triangles, "int32"), width,
                                      height).cpu().numpy()
    state = dict(got.state)
    state["box"] = state["box"].copy()
    for f, box in boxes.items():
        state["box"][f] = box
    want = I.face_grads(state, ids, d_color, colors, width, height)
    assert_bits(rows, want, "face_grads")
    assert not bits(rows[:4]).any() and rows[4].any()


def test_a_permuted_triangle_order_gives_the_same_vertex_sums():
    """The rows move with their triangles bit for bit; a vertex's sum adds the same terms in
    another order: the same bits for a valence of at most 2 (an IEEE add commutes), and within
    (n - 1) u of the sum of the terms' sizes otherwise."""
    width, height = 33, 29
    vertices, triangles = _fan(9)
    _, proj, eye = view(width, height, yaw=0.0, pitch=0.0)
    colors, d_color = ref.grey(vertices, 11), gradient(width, height, 12)
    a = both(vertices, triangles, proj, eye, width, height, colors, d_color)
    order = np.random.default_rng(13).permutation(len(triangles))
    b = both(vertices, triangles[order], proj, eye, width, height, colors, d_color)
    assert_bits(b.face_grads, a.face_grads[order], "rows")
    valence = np.diff(a.starts)
    assert_bits(b.grad[valence <= 2], a.grad[valence <= 2], "valence <= 2")
    assert (valence[1:10] == 2).all() and valence[0] == 9
    # vertex 0: nine terms per sum, eight adds in either order, each at most u of the terms' sizes;
    # then through |J| / w and |P2c|, and four more roundings of the value itself
    terms = np.abs(a.face_grads.astype(np.float64).reshape(-1, 3)[a.order[a.starts[0]:a.starts[1]]])
    slack = 2 * 8 * U * terms.sum(0)
    p = np.asarray(proj, dtype=np.float64).reshape(3, 4)
    homog = p[:, :3] @ vertices[0].astype(np.float64) + p[:, 3]
    for c in range(3):
        jac = np.abs([p[0, c] - homog[0] / homog[2] * p[2, c], p[1, c] - homog[1] / homog[2] * p[2, c]])
        bound = (slack[0] * jac[0] + slack[1] * jac[1]) / homog[2] + slack[2] * abs(p[2, c]) \
            + 8 * U * ((terms.sum(0)[:2] * jac).sum() / homog[2] + terms.sum(0)[2] * abs(p[2, c]))
        assert abs(float(b.grad[0][c]) - float(a.grad[0][c])) <= bound
    assert a.grad[0].all()


# ------------------------------------------------------------------------------- the host functions
def test_geometry_backward_with_interior_is_k34_plus_k35():
    import fourier_feature_nets_amd as ffn
    width, height = 24, 20
    vertices, triangles, colors, _ = ref.scene(402, 14)
    cam, proj, eye = view(width, height)
    rng = np.random.default_rng(21)
    g_color = rng.uniform(-1, 1, (width * height, 3)).astype(np.float32)
    g_alpha = rng.uniform(-1, 1, width * height).astype(np.float32)
    opposite = ffn.edge_opposites(triangles, len(vertices), "cpu").numpy()
    grad34, plain, _, fr, _, _ = A.geometry_backward(vertices, triangles, proj, eye, width, height,
                                                     colors, opposite, g_color, g_alpha)
    want, _ = I.interior_backward(fr["state"], fr["ids"], plain, colors, vertices, triangles, proj,
                                  width, height, grad34)
    without, plain_a = ffn.render_mesh_geometry_backward(vertices, triangles, cam, colors, g_color,
                                                         g_alpha)
    got, plain_b = ffn.render_mesh_geometry_backward(vertices, triangles, cam, colors, g_color,
                                                     g_alpha, interior=True)
    assert_bits(without, grad34, "interior=False is K34's result")
    assert_bits(plain_a, plain, "d_color_plain")
    assert_bits(plain_b, plain, "d_color_plain")
    assert_bits(got, want, "K34 + K35")
    assert (got != without).any()
    # tensors in, a given adjacency and grad with accumulate: the same sums on top of a start
    from fourier_feature_nets_amd import mesh
    v, t = on_gpu(vertices, "float32"), on_gpu(triangles, "int32")
    start = rng.standard_normal(vertices.shape).astype(np.float32)
    held = on_gpu(start, "float32")
    out, _ = ffn.render_mesh_geometry_backward(
        v, t, cam, on_gpu(colors, "float32"), on_gpu(g_color, "float32"), on_gpu(g_alpha, "float32"),
        grad=held, accumulate=True, interior=True, adjacency=mesh.vertex_adjacency(t, len(vertices)))
    assert out is held
    base = A.vertex_grad(*A.backward(fr, A.decisions(fr, opposite), g_color, g_alpha)[2:], vertices,
                         proj, start)
    assert_bits(held.cpu().numpy(), I.interior_backward(
        fr["state"], fr["ids"], plain, colors, vertices, triangles, proj, width, height, base)[0],
        "accumulate")


SIZE, CAMERAS = 32, 4


@pytest.fixture(scope="module")
def torus():
    """The dataset of tests/test_mesh_aa_gpu.py, rebuilt here: ``procedural_torus(16, 8)`` with
    per-vertex colours drawn by K31 from 4 cameras at 32 x 32."""
    import fourier_feature_nets_amd as ffn
    from bench import synthetic_rig
    vertices, triangles, _, _ = ffn.procedural_torus(rings=16, sides=8)
    vertices = ffn.normalize_points(vertices)
    colors = np.random.default_rng(16).uniform(0, 1, (len(vertices), 3)).astype(np.float32)
    intr, poses = synthetic_rig(CAMERAS, SIZE)
    cams = [ffn.CameraInfo.create("c%d" % i, ffn.Resolution(SIZE, SIZE), intr, p)
            for i, p in enumerate(poses)]
    images = np.zeros((CAMERAS, SIZE, SIZE, 4), np.uint8)
    for index, cam in enumerate(cams):
        color, alpha, _ = ffn.render_mesh_image(vertices, triangles, cam, colors=colors,
                                                include_depth=True)
        images[index, ..., :3] = color
        images[index, ..., 3] = np.rint(255 * alpha)
    bounds = np.diag([2, 2, 2, 1]).astype(np.float32)
    with contextlib.redirect_stdout(io.StringIO()):
        dataset = ffn.ImageDataset("torus", images, bounds, cams, 2, True, False)
    centre = vertices.mean(0, keepdims=True)
    start = (centre + 0.9 * (vertices - centre)).astype(np.float32)
    return types.SimpleNamespace(vertices=vertices, triangles=triangles, colors=colors, cams=cams,
                                 dataset=dataset, start=start)


def test_one_step_with_interior_is_the_step_done_by_hand(torus):
    import fourier_feature_nets_amd as ffn
    from fourier_feature_nets_amd import mesh, ops
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    train = torus.dataset
    weight = 0.25
    fit = dict(num_steps=1, learning_rate=1e-3, cameras_per_step=2, seed=5,
               laplacian_weight=weight, verbose=False)
    got, log = ffn.fit_mesh_geometry(torus.start, torus.triangles, torus.colors, train,
                                     interior=True, **fit)
    plain, plain_log = ffn.fit_mesh_geometry(torus.start, torus.triangles, torus.colors, train, **fit)

    v0, t = on_gpu(torus.start, "float32"), on_gpu(torus.triangles, "int32")
    colors = on_gpu(torus.colors, "float32")
    data = v0.clone()
    projections = projection_matrices(torus.cams)
    eyes = eye_positions(torus.cams, (0.0, 0.0, 0.0))
    opposite = mesh.edge_opposites(t, len(torus.start))
    adjacency = mesh.vertex_adjacency(t, len(torus.start))
    starts, neighbors = mesh.vertex_neighbors(t, len(torus.start))
    grads = torch.empty_like(data)
    per = SIZE * SIZE
    pixels = torch.arange(per, dtype=torch.int64, device="cuda")
    chosen = torch.randperm(CAMERAS, generator=torch.Generator().manual_seed(5)).tolist()[:2]
    count = 2 * per
    aw = float(train.alpha_weight)
    for number, camera in enumerate(chosen):
        record, color, alpha, _, ids, _, _, zbuf = mesh._rasterize_z(
            data, t, projections[camera], eyes[camera], SIZE, SIZE, colors)
        smooth = ops.mesh_aa_forward(record, zbuf, ids, opposite, data, projections[camera], color,
                                     alpha, SIZE, SIZE)
        sums, g_color, g_alpha = ops.mse_loss(smooth[0], smooth[1], train.colors, train.alphas,
                                              pixels + camera * per, 1.0 / (3 * count), aw / count)
        d_color, _, entry_vertex, entry_grad = ops.mesh_aa_backward(
            record, zbuf, ids, opposite, data, t, projections[camera], color, alpha, g_color,
            g_alpha, SIZE, SIZE)
        sorted_vertex, order = torch.sort(entry_vertex, stable=True)
        ops.mesh_aa_vertex_grad(sorted_vertex.contiguous(), order.to(torch.int32).contiguous(),
                                entry_grad, data, projections[camera], grads, accumulate=number > 0)
        face_grads = ops.mesh_interp_face_grads(record, ids, d_color, colors, t, SIZE, SIZE)
        ops.mesh_interp_vertex_grad(face_grads, adjacency[0], adjacency[1], data,
                                    projections[camera], grads, accumulate=True)
        total = sums if number == 0 else total + sums
    ops.mesh_laplacian(data - v0, starts, neighbors, weight / len(torus.start), grads,
                       accumulate=True)
    loss = float(ops.loss_value(total, count, aw).item())
    exp_avg, exp_avg_sq = torch.zeros_like(data.view(-1)), torch.zeros_like(data.view(-1))
    ops.clip_adam(data.view(-1), grads.view(-1), exp_avg, exp_avg_sq, 1, 1e-3)
    assert log[0].loss == loss and loss > 0 and plain_log[0].loss == loss
    assert_bits(got, data.cpu().numpy(), "vertices after one step")
    assert (got != plain).any() and (got != torus.start).any()


def test_interior_adds_no_host_synchronisation_to_a_step(torus, monkeypatch):
    """The two extra launches take tensors that are already on the device: between the frame and
    the update no ``.item()``, ``.cpu()`` or ``.tolist()`` is called by the interior path."""
    from fourier_feature_nets_amd import mesh
    calls = []
    real = mesh._interior_backward

    def watched(*args):
        with monkeypatch.context() as patch:
            for name in ("item", "cpu", "tolist", "numpy"):
                patch.setattr(torch.Tensor, name, lambda self, *a, _n=name, **k: calls.append(_n))
            return real(*args)
    monkeypatch.setattr(mesh, "_interior_backward", watched)
    import fourier_feature_nets_amd as ffn
    _, log = ffn.fit_mesh_geometry(torus.start, torus.triangles, torus.colors, torus.dataset,
                                   num_steps=2, cameras_per_step=2, verbose=False, interior=True)
    assert len(log) == 2 and calls == []


# ------------------------------------------------------------------------------- stream order, bounds
NAMES = ["mesh_interp_face_grads", "mesh_interp_vertex_grad"]


@pytest.mark.parametrize("scenario", ["A", "B"])
@pytest.mark.parametrize("name", NAMES)
def test_k35_launches_on_the_callers_stream(name, scenario, monkeypatch):
    """The two cases of tests/stream_order_cases_mesh_interp.py under the harness of
    tests/test_stream_order_gpu.py, run from here as well."""
    from fourier_feature_nets_amd import _lib
    from tests import stream_helpers as sh
    from tests.stream_order_cases import CASES
    case, = [c for c in CASES if c.name == name]
    hook = sh.Hook(_lib.call)
    monkeypatch.setattr(_lib, "call", hook)
    reached = sh.run_case(case, scenario, hook, monkeypatch)
    assert set(case.reaches) <= set(reached)


@pytest.mark.parametrize("name", NAMES)
def test_k35_stays_inside_its_buffers(name, monkeypatch):
    """The same two cases under the guarded placement of tests/memory_helpers.py with both fills,
    by the checks of tests/test_memory_bounds_gpu.py: no red zone changes, every output word is
    written, no input is read outside its extent or written."""
    from tests.stream_order_cases import CASES
    from tests.test_memory_bounds_gpu import _check
    case, = [c for c in CASES if c.name == name]
    guard = _check(case, monkeypatch)
    assert set(case.reaches) <= set(guard.reached)
