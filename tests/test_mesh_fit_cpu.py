"""K32 without a GPU: the numpy restatement (tests/mesh_raster_grad_reference.py) held to the float64
identities a transpose has to satisfy, ``vertex_adjacency`` against closed forms, the refusals of the
new wrappers and the two new entry points of the header.

The budgets are counted from the f32 roundings of the contract (``Rg.adjoint_budget``,
``Rg.weight_budget``, ``Rg.splat_budget`` derive them); the tests print the share of each they use.
"""

import inspect
import types

import numpy as np
import pytest
import torch

from tests import mesh_raster_grad_reference as Rg
from tests import mesh_raster_reference as R
# (the public names this module is about, at module scope: without the feature nothing here runs)
from fourier_feature_nets_amd import (color_mesh_from_images, fit_mesh_colors,  # noqa: F401
                                      render_mesh_backward, vertex_adjacency)
from fourier_feature_nets_amd.ops import (mesh_raster_face_sums_check,  # noqa: F401
                                          mesh_vertex_gather_check)
from tests import stream_order_cases_mesh_fit  # noqa: F401  (adds K32's stream-order cases)

WIDTH, HEIGHT = 48, 40


@pytest.fixture(scope="module")
def world():
    """``scene(3, 40)`` from ``camera(48, 40)``: its K31 state and ids, made once."""
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    vertices, triangles, colors, _ = R.scene(3, 40)
    cam = R.camera(WIDTH, HEIGHT)
    proj, eye = projection_matrices([cam])[0], eye_positions([cam], (0.0, 0.0, 0.0))[0]
    state, ids = Rg.raster_ids(vertices, triangles, proj, WIDTH, HEIGHT)
    order, starts = Rg.adjacency(triangles, len(vertices))
    out = types.SimpleNamespace(vertices=vertices, triangles=triangles, colors=colors, proj=proj,
                                eye=eye, state=state, ids=ids, order=order, starts=starts)
    for value in (vertices, triangles, colors, ids, order, starts):
        value.setflags(write=False)
    return out


def _frame(world, colors):
    return R.raster(world.vertices, world.triangles, world.proj, world.eye, WIDTH, HEIGHT,
                    colors=colors)


def test_the_scene_is_covered_enough(world):
    covered = float((world.ids >= 0).mean())
    print("covered %.1f %% of the pixels, %d triangles drawn, largest box %d pixels"
          % (100 * covered, int((world.state["status"] == R.DRAWN).sum()),
             int(world.state["counts"].max())))
    assert covered >= 0.15
    color, alpha, _, ids, _, _ = _frame(world, world.colors)
    assert np.array_equal(ids, world.ids) and np.array_equal(alpha > 0, ids >= 0)


def test_adjoint_identity_in_float64(world):
    """sum_p color[p] . g[p] over the covered pixels = sum_v c_v . grad_v."""
    g = np.random.default_rng(11).standard_normal((WIDTH * HEIGHT, 3)).astype(np.float32)
    color = _frame(world, world.colors)[0]
    grad, _, _, _ = Rg.backward(world.vertices, world.triangles, world.proj, WIDTH, HEIGHT, g)
    hit = world.ids >= 0
    left = float((color[hit].astype(np.float64) * g[hit].astype(np.float64)).sum())
    right = float((world.colors.astype(np.float64) * grad.astype(np.float64)).sum())
    budget = Rg.adjoint_budget(world.state, world.ids, WIDTH, world.colors, g, world.starts)
    print("adjoint: %.9g against %.9g, difference %.3g, budget %.3g, share %.3f"
          % (left, right, abs(left - right), budget, abs(left - right) / budget))
    assert budget < 1e-4 * abs(left)           # the budget is one that can fail
    assert abs(left - right) <= budget


def test_weights_sum_to_the_covered_pixels(world):
    g = np.zeros((WIDTH * HEIGHT, 3), dtype=np.float32)
    _, weight, _, _ = Rg.backward(world.vertices, world.triangles, world.proj, WIDTH, HEIGHT, g)
    covered = int((world.ids >= 0).sum())
    assert covered >= 0.15 * WIDTH * HEIGHT
    total = float(weight.astype(np.float64).sum())
    budget = Rg.weight_budget(world.state, world.ids, world.starts)
    print("weights: %.10f for %d covered pixels, budget %.3g, share %.3f"
          % (total, covered, budget, abs(total - covered) / budget))
    assert abs(total - covered) <= budget


def test_splat_of_a_constant_frame_returns_the_constant(world):
    constant = np.array([0.3, 0.6, 0.9], dtype=np.float32)
    color = _frame(world, np.tile(constant, (len(world.vertices), 1)))[0]
    grad, weight, _, _ = Rg.backward(world.vertices, world.triangles, world.proj, WIDTH, HEIGHT,
                                     color)
    got = Rg.mean_colors(grad, weight)
    seen = weight > 0
    assert seen.sum() >= 3 and not seen.all()         # both branches of the division
    assert np.array_equal(got[~seen], np.full((int((~seen).sum()), 3), 0.5, dtype=np.float32))
    error = np.abs(got[seen].astype(np.float64) - constant.astype(np.float64))
    budget = Rg.splat_budget(world.state, world.ids, world.starts, constant)
    print("splat: %d seen vertices, worst error %.3g, budget %s, share %.3f"
          % (int(seen.sum()), error.max(), budget, (error / budget).max()))
    assert (error <= budget).all()


def test_unselected_pixels_are_not_read(world):
    g = np.random.default_rng(5).standard_normal((WIDTH * HEIGHT, 3)).astype(np.float32)
    clean = Rg.face_sums(world.state, world.ids, g, WIDTH, HEIGHT)
    dirty = g.copy()
    dirty[world.ids < 0] = [np.nan, np.inf, -np.inf]
    assert np.array_equal(Rg.face_sums(world.state, world.ids, dirty, WIDTH, HEIGHT), clean)
    assert np.isfinite(clean).all()


# ------------------------------------------------------------------------------- adjacency
def _fan(valence):
    """Vertex 0 in ``valence`` triangles (0, k, k + 1), k = 1 .. valence."""
    k = np.arange(1, valence + 1)
    return np.stack([np.zeros_like(k), k, k + 1], 1).astype(np.int32), valence + 2


def _fan_closed_form(valence):
    order = [3 * f for f in range(valence)] + [1]
    starts = [0, valence, valence + 1]
    for k in range(2, valence + 1):
        order += [3 * k - 4, 3 * k - 2]            # third corner of face k - 2, second of face k - 1
        starts.append(starts[-1] + 2)
    order.append(3 * (valence - 1) + 2)
    starts.append(starts[-1] + 1)
    return order, starts


ADJACENCY = {
    "unused_vertex": (np.array([[0, 1, 2], [0, 2, 4]]), 5, [0, 3, 1, 2, 4, 5], [0, 2, 3, 5, 5, 6]),
    "face_twice": (np.array([[0, 1, 2], [0, 1, 2]]), 3, [0, 3, 1, 4, 2, 5], [0, 2, 4, 6]),
    "clamped_single_face": (np.array([[-5, 1, 99]]), 3, [0, 1, 2], [0, 1, 2, 3]),
    "all_clamped_to_one": (np.array([[7, 8, 9]], dtype=np.int64), 1, [0, 1, 2], [0, 3]),
    "fan_130": _fan(130) + _fan_closed_form(130),
}


@pytest.mark.parametrize("name", sorted(ADJACENCY))
def test_vertex_adjacency_closed_forms(name):
    from fourier_feature_nets_amd import vertex_adjacency
    triangles, num_vertices, order, starts = ADJACENCY[name]
    for given in (triangles, torch.from_numpy(triangles)):
        got_order, got_starts = vertex_adjacency(given, num_vertices, device="cpu")
        assert got_order.dtype == torch.int32 and got_starts.dtype == torch.int32
        assert got_order.tolist() == order and got_starts.tolist() == starts
    ref_order, ref_starts = Rg.adjacency(triangles, num_vertices)
    assert ref_order.tolist() == order and ref_starts.tolist() == starts
    if name == "fan_130":
        assert starts[1] - starts[0] == 130


# ------------------------------------------------------------------------------- refusals
@pytest.fixture
def no_device(monkeypatch):
    """A launch, or anything else that wants the library, fails the test."""
    from fourier_feature_nets_amd import ops

    def refuse(*args, **kwargs):
        raise AssertionError("a refusal reached the device")
    monkeypatch.setattr(ops, "_call", refuse)
    monkeypatch.setattr(torch.cuda, "is_available", refuse)


def _raises(name, call, *args, **kwargs):
    with pytest.raises(ValueError) as caught:
        call(*args, **kwargs)
    assert name in str(caught.value), (name, str(caught.value))


def test_ops_checks_refuse_by_name(no_device):
    from fourier_feature_nets_amd import ops
    record = torch.zeros((5, 16), dtype=torch.int32)
    ids = torch.zeros((12,), dtype=torch.int32)
    d_color = torch.zeros((12, 3), dtype=torch.float32)
    check = ops.mesh_raster_face_sums_check
    check(record, ids, d_color, 4, 3)
    _raises("record", check, record[:, :15].contiguous(), ids, d_color, 4, 3)
    _raises("record", check, record.to(torch.int64), ids, d_color, 4, 3)
    _raises("record", check, record[:0], ids, d_color, 4, 3)
    _raises("ids", check, record, ids.to(torch.int64), d_color, 4, 3)
    _raises("ids", check, record, ids[:11], d_color, 4, 3)
    _raises("d_color", check, record, ids, d_color.double(), 4, 3)
    _raises("d_color", check, record, ids, d_color.reshape(3, 12), 4, 3)
    _raises("d_color", check, record, ids, d_color.numpy(), 4, 3)
    _raises("width", check, record, ids, d_color, 0, 3)
    _raises("width", check, record, ids, d_color, 4, 16385)

    sums = torch.zeros((5, 12), dtype=torch.float32)
    order = torch.zeros((15,), dtype=torch.int32)
    starts = torch.zeros((8,), dtype=torch.int32)
    grad, weight = torch.zeros((7, 3)), torch.zeros((7,))
    check = ops.mesh_vertex_gather_check
    assert check(sums, order, starts) == 7 and check(sums, order, starts, grad, weight, True) == 7
    _raises("face_sums", check, sums[:, :11].contiguous(), order, starts)
    _raises("face_sums", check, sums.double(), order, starts)
    _raises("corner_order", check, sums, order.to(torch.int64), starts)
    _raises("corner_order", check, sums, order[:14], starts)
    _raises("vertex_starts", check, sums, order, starts[:1])
    _raises("vertex_starts", check, sums, order, starts.to(torch.int64))
    _raises("grad", check, sums, order, starts, grad[:6], weight)
    _raises("weight", check, sums, order, starts, grad, weight[:6])
    _raises("weight", check, sums, order, starts, grad, None)
    _raises("accumulate", check, sums, order, starts, None, None, True)


def _stand_in(images, cameras):
    return types.SimpleNamespace(images=images, cameras=cameras, color_space="RGB")


def test_mesh_functions_refuse_before_any_device(no_device):
    import fourier_feature_nets_amd as ffn
    vertices, triangles = R.quad_scene()
    colors = R.grey(vertices)
    cam = R.camera(6, 5)
    d_color = np.zeros((30, 3), dtype=np.float32)
    images = np.zeros((2, 5, 6, 4), dtype=np.uint8)
    data = _stand_in(images, [cam, cam])

    back = ffn.render_mesh_backward
    _raises("supersample", back, vertices, triangles, cam, d_color, supersample=2)
    _raises("texture", back, vertices, triangles, cam, d_color, uvs=np.zeros((4, 2), np.float32),
            texture=np.zeros((2, 2, 3), np.uint8))
    _raises("d_color", back, vertices, triangles, cam, d_color[:29])
    _raises("vertices", back, vertices[:, :2], triangles, cam, d_color)
    _raises("triangles", back, vertices, triangles.astype(np.float32), cam, d_color)
    _raises("triangles", back, vertices, triangles + 9, cam, d_color)
    _raises("camera", back, vertices, triangles, "front", d_color)
    _raises("batch_size", back, vertices, triangles, cam, d_color, batch_size=0)
    _raises("accumulate", back, vertices, triangles, cam, d_color, accumulate=True)

    fit = ffn.fit_mesh_colors
    _raises("learning_rate", fit, vertices, triangles, colors, data, learning_rate=0.0)
    _raises("learning_rate", fit, vertices, triangles, colors, data, learning_rate=-1e-2)
    _raises("learning_rate", fit, vertices, triangles, colors, data, learning_rate=float("nan"))
    _raises("colors", fit, vertices, triangles, colors[:3], data)
    _raises("colors", fit, vertices, triangles, None, data)
    _raises("colors", fit, vertices, triangles, (255 * colors).astype(np.uint8), data)
    _raises("cameras_per_step", fit, vertices, triangles, colors, data, cameras_per_step=0)
    _raises("alpha_threshold", fit, vertices, triangles, colors, data, alpha_threshold=1.5)
    _raises("images", fit, vertices, triangles, colors, _stand_in(images.astype(np.float32),
                                                                  [cam, cam]))
    _raises("cameras", fit, vertices, triangles, colors, _stand_in(images, [cam]))
    _raises("val_dataset", fit, vertices, triangles, colors, data,
            _stand_in(images[..., :2], [cam, cam]))
    _raises("alpha", fit, vertices, triangles, colors, _stand_in(images[..., :3], [cam, cam]),
            alpha_threshold=0.5)

    splat = ffn.color_mesh_from_images
    _raises("alpha_threshold", splat, vertices, triangles, data, alpha_threshold=2.0)
    _raises("alpha_threshold", splat, vertices, triangles, data, alpha_threshold=float("nan"))
    _raises("images", splat, vertices, triangles, _stand_in(images[0], [cam]))
    _raises("camera", splat, vertices, triangles, _stand_in(images, [cam, R.camera(7, 5)]))
    _raises("colors", splat, vertices, triangles, data, colors=colors[:, :2])
    _raises("color_space", splat, vertices, triangles,
            types.SimpleNamespace(images=images, cameras=[cam, cam], color_space="YCrCb"))

    adjacency = ffn.vertex_adjacency
    _raises("triangles", adjacency, triangles.reshape(-1), 4, "cpu")
    _raises("triangles", adjacency, triangles.astype(np.float64), 4, "cpu")
    _raises("num_vertices", adjacency, triangles, 0, "cpu")


# ------------------------------------------------------------------------------- the ABI
def test_header_declares_and_ops_binds_the_entry_points():
    from fourier_feature_nets_amd import _lib, ops
    from tests import stream_helpers
    import fourier_feature_nets
    import fourier_feature_nets_amd
    for name, wrapper in (("ffn_mesh_raster_face_sums", ops.mesh_raster_face_sums),
                          ("ffn_mesh_vertex_gather", ops.mesh_vertex_gather)):
        assert name in _lib.declared_symbols()
        assert name in stream_helpers.stream_entry_points()
        assert '"%s"' % name in inspect.getsource(wrapper)
    assert _lib.ABI_VERSION == 3
    for name in ("vertex_adjacency", "render_mesh_backward", "color_mesh_from_images",
                 "fit_mesh_colors"):
        assert name in fourier_feature_nets_amd.__all__
        assert getattr(fourier_feature_nets, name) is getattr(fourier_feature_nets_amd, name)


def test_the_stream_order_table_holds_a_case_for_each_entry_point():
    """tests/stream_order_cases_mesh_fit.py has added its two cases to the table that
    tests/test_stream_order_cpu.py holds to the header, each once."""
    from tests.stream_order_cases import CASES
    reached = [name for c in CASES for name in c.reaches]
    for name in ("ffn_mesh_raster_face_sums", "ffn_mesh_vertex_gather"):
        assert reached.count(name) == 1
    names = [c.name for c in CASES]
    assert names.count("mesh_raster_face_sums") == 1 and names.count("mesh_vertex_gather") == 1
