"""K33 without a GPU: the numpy restatement (tests/mesh_texture_reference.py) held to things it does
not share -- K31c's own textured colour, the float64 identities a matrix and its transpose have to
satisfy, closed forms of the atlas -- and the refusals, the OBJ round trip and the three new entry
points of the header.

The budgets are counted from the f32 roundings of the contract (``Rt.partition_budget``,
``Rt.weight_budget``, ``Rt.adjoint_budget``, ``Rt.splat_budget``, ``Rt.quantisation_budget`` derive
them); the tests print the share of each they use.
"""

import inspect
import types

import numpy as np
import pytest
import torch

from tests import mesh_raster_reference as R
from tests import mesh_texture_reference as Rt
# (the public names this module is about, at module scope: without the feature nothing here runs)
from fourier_feature_nets_amd import (MeshTaps, bake_vertex_colors, fit_mesh_texture,  # noqa: F401
                                      mesh_texture_taps, render_mesh_texture,
                                      render_mesh_texture_backward, texture_mesh_from_images,
                                      texture_to_uint8, unwrap_mesh)
from fourier_feature_nets_amd.ops import (mesh_texture_gather_check,  # noqa: F401
                                          mesh_texture_grad_check, mesh_texture_taps_check)
from tests import stream_order_cases_mesh_fit  # noqa: F401  (the table as the whole suite has it)
from tests import stream_order_cases_mesh_texture  # noqa: F401  (adds K33's stream-order cases)

WIDTH, HEIGHT = 48, 40
TEX_H, TEX_W = 8, 4

# a unit cube the way OcTree.extract_mesh writes a lone cell: six quads (q0, q1, q2), (q0, q2, q3)
CUBE_QUADS = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]


def cube():
    corner = np.arange(8)
    vertices = np.stack([corner & 1, (corner >> 1) & 1, corner >> 2], 1).astype(np.float32) - 0.5
    triangles = np.array([face for q in CUBE_QUADS for face in ((q[0], q[1], q[2]),
                                                                (q[0], q[2], q[3]))], np.int32)
    return vertices, triangles


@pytest.fixture(scope="module")
def world():
    """``scene(3, 40)`` from ``camera(48, 40)`` with its random UVs in [-0.5, 1.5] and a random
    8 x 4 texture: the K31 state, the ids and the taps, made once."""
    from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
    vertices, triangles, _, uvs = R.scene(3, 40)
    cam = R.camera(WIDTH, HEIGHT)
    proj, eye = projection_matrices([cam])[0], eye_positions([cam], (0.0, 0.0, 0.0))[0]
    tap_texel, tap_weight, sorted_texels, order, state, ids = Rt.camera_taps(
        vertices, triangles, uvs, proj, WIDTH, HEIGHT, (TEX_H, TEX_W))
    bytes_ = R.texture(33, TEX_H, TEX_W, 3)
    out = types.SimpleNamespace(vertices=vertices, triangles=triangles, uvs=uvs, proj=proj, eye=eye,
                                state=state, ids=ids, tap_texel=tap_texel, tap_weight=tap_weight,
                                sorted_texels=sorted_texels, order=order, bytes=bytes_,
                                depth=Rt.longest_row(sorted_texels, TEX_H * TEX_W))
    for value in (vertices, triangles, uvs, ids, tap_texel, tap_weight, sorted_texels, order,
                  bytes_):
        value.setflags(write=False)
    return out


def test_the_scene_is_covered_and_uses_both_ends_of_the_texture(world):
    covered = world.tap_texel[:, 0] >= 0
    assert np.array_equal(covered, world.ids >= 0) and covered.mean() >= 0.15
    assert not np.any(world.tap_weight[~covered]) and (world.tap_texel[~covered] == -1).all()
    used = np.unique(world.tap_texel[covered])
    print("covered %.1f %%, %d of %d texels used, longest row %d"
          % (100 * covered.mean(), len(used), TEX_H * TEX_W, world.depth))
    assert used.min() == 0 and used.max() == TEX_H * TEX_W - 1
    # UVs outside [0, 1] clamp: some pixel repeats a tap
    assert (world.tap_texel[covered, 0] == world.tap_texel[covered, 1]).any()


def test_taps_reproduce_k31c_textured_colour_bit_for_bit(world):
    """The colour formed from the taps and the uint8 texture, divided by 255 after the blend, is
    ``mesh_raster_reference.resolve``'s textured colour: K33a is K31c's own lookup."""
    zbuf = R.draw(world.state, WIDTH, HEIGHT)
    want = R.resolve(world.state, zbuf, world.vertices, world.eye, WIDTH, HEIGHT, uvs=world.uvs,
                     texture=world.bytes)[0]
    hit = np.flatnonzero(world.ids >= 0)
    t = world.bytes.reshape(-1, 3).astype(np.float32)[world.tap_texel[hit]]       # (n,4,3)
    w = world.tap_weight[hit][:, :, None]
    got = (((w[:, 0] * t[:, 0] + w[:, 1] * t[:, 1]) + w[:, 2] * t[:, 2])
           + w[:, 3] * t[:, 3]) / np.float32(255.0)
    assert got.dtype == np.float32 and len(hit) > 300
    np.testing.assert_array_equal(got.view(np.uint32), want[hit].view(np.uint32))


def test_the_weights_of_a_pixel_sum_to_one(world):
    hit = world.ids >= 0
    sums = world.tap_weight[hit].astype(np.float64).sum(1)
    budget = Rt.partition_budget()
    print("partition of unity: worst %.3g, budget %.3g, share %.3f"
          % (np.abs(sums - 1).max(), budget, np.abs(sums - 1).max() / budget))
    assert (world.tap_weight[hit] >= 0).all() and (np.abs(sums - 1) <= budget).all()


def test_texel_weights_sum_to_the_covered_pixels(world):
    g = np.zeros((WIDTH * HEIGHT, 3), dtype=np.float32)
    _, weight = Rt.grad(world.sorted_texels, world.order, world.tap_weight, g, TEX_H * TEX_W)
    covered = int((world.ids >= 0).sum())
    total = float(weight.astype(np.float64).sum())
    budget = Rt.weight_budget(covered, world.depth)
    print("weights: %.10f for %d covered pixels, budget %.3g, share %.3f"
          % (total, covered, budget, abs(total - covered) / budget))
    assert abs(total - covered) <= budget


def test_adjoint_identity_in_float64(world):
    """sum_p color[p] . g[p] over the covered pixels = sum_t texture[t] . grad[t]."""
    rng = np.random.default_rng(11)
    g = rng.standard_normal((WIDTH * HEIGHT, 3)).astype(np.float32)
    texture = rng.uniform(0, 1, (TEX_H * TEX_W, 3)).astype(np.float32)
    color, alpha = Rt.gather(world.tap_texel, world.tap_weight, texture)
    grad, _ = Rt.grad(world.sorted_texels, world.order, world.tap_weight, g, TEX_H * TEX_W)
    hit = world.ids >= 0
    assert np.array_equal(alpha > 0, hit)
    left = float((color[hit].astype(np.float64) * g[hit].astype(np.float64)).sum())
    right = float((texture.astype(np.float64) * grad.astype(np.float64)).sum())
    budget = Rt.adjoint_budget(world.tap_texel, world.tap_weight, texture, g, world.depth)
    print("adjoint: %.9g against %.9g, difference %.3g, budget %.3g, share %.3f"
          % (left, right, abs(left - right), budget, abs(left - right) / budget))
    # the budget is one that can fail: one pixel left out of either side would show
    assert budget < 0.1 * np.abs((color[hit].astype(np.float64) * g[hit]).sum(1)).max()
    assert abs(left - right) <= budget


def test_splat_of_constant_images_returns_the_constant(world):
    from fourier_feature_nets_amd.cameras import projection_matrices
    constant = np.array([77, 150, 230], dtype=np.uint8)
    cams = [R.camera(WIDTH, HEIGHT, yaw=yaw) for yaw in (0.3, 1.3)]
    projections = projection_matrices(cams)
    images = np.zeros((2, HEIGHT, WIDTH, 4), dtype=np.uint8)
    images[..., :3], images[..., 3] = constant, 255
    size = (16, 16)
    got, weights = Rt.texture_from_images(world.vertices, world.triangles, world.uvs, projections,
                                          images, size)
    depth = len(cams) + max(Rt.longest_row(Rt.camera_taps(
        world.vertices, world.triangles, world.uvs, proj, WIDTH, HEIGHT, size)[2], 256)
        for proj in projections)
    seen = weights > 0
    assert seen.sum() >= 50 and not seen.all()        # both branches of the division
    assert np.array_equal(got[~seen], np.full((int((~seen).sum()), 3), 0.5, dtype=np.float32))
    c = constant.astype(np.float32) / np.float32(255.0)
    error = np.abs(got[seen].astype(np.float64) - c.astype(np.float64))
    budget = Rt.splat_budget(depth, c)
    print("splat: %d seen texels, depth %d, worst error %.3g, budget %s, share %.3f"
          % (int(seen.sum()), depth, error.max(), budget, (error / budget).max()))
    assert (error <= budget).all()


def test_nan_weights_and_dirty_background_reach_no_texel(world):
    rng = np.random.default_rng(5)
    g = rng.standard_normal((WIDTH * HEIGHT, 3)).astype(np.float32)
    clean = Rt.grad(world.sorted_texels, world.order, world.tap_weight, g, TEX_H * TEX_W)
    dirty = g.copy()
    dirty[world.ids < 0] = [np.nan, np.inf, -np.inf]
    again = Rt.grad(world.sorted_texels, world.order, world.tap_weight, dirty, TEX_H * TEX_W)
    assert np.array_equal(again[0], clean[0]) and np.isfinite(clean[0]).all()
    # a zero, NaN or negative weight over a non-finite d_color is skipped by selection
    weights = world.tap_weight.copy()
    hit = np.flatnonzero(world.ids >= 0)[:5]
    weights[hit] = [0.0, np.nan, -1.0, 0.0]
    dirty[hit] = np.inf
    out = Rt.grad(world.sorted_texels, world.order, weights, dirty, TEX_H * TEX_W)
    assert np.isfinite(out[0]).all() and np.isfinite(out[1]).all()
    assert not np.array_equal(out[1], clean[1])


# ------------------------------------------------------------------------------- the atlas
def _unwrap_both(vertices, triangles, tile):
    """``unwrap_mesh`` against the restatement -> its results and the tile of every triangle."""
    got = unwrap_mesh(vertices, triangles, tile)
    new_triangles, texel, vertex_map, tile_of, size = Rt.unwrap(triangles, tile)
    assert got[4] == size
    np.testing.assert_array_equal(got[1], new_triangles)
    np.testing.assert_array_equal(got[3], vertex_map)
    np.testing.assert_array_equal(got[2].astype(np.float64) * [size[1], size[0]], texel)
    assert got[0].dtype == vertices.dtype and got[1].dtype == np.int32
    assert got[2].dtype == np.float32 and got[3].dtype == np.int32
    # vertex_map reproduces the positions and the original triangles
    np.testing.assert_array_equal(got[0], vertices[got[3]])
    np.testing.assert_array_equal(got[3][got[1]], triangles)
    for side in size:
        assert side >= 1 and side & (side - 1) == 0
    assert size[1] in (size[0], 2 * size[0])
    return got, tile_of


def test_unwrap_a_lone_triangle():
    vertices = np.random.default_rng(0).uniform(-1, 1, (5, 3)).astype(np.float32)
    got, _ = _unwrap_both(vertices, np.array([[4, 0, 2]], np.int32), 4)
    assert got[4] == (4, 4) and got[3].tolist() == [4, 0, 2] and got[1].tolist() == [[0, 1, 2]]
    np.testing.assert_array_equal(got[2] * 4, [[0.5, 0.5], [2.5, 0.5], [0.5, 2.5]])
    got, _ = _unwrap_both(vertices, np.array([[4, 0, 2]], np.int32), 3)
    assert got[4] == (4, 4)
    np.testing.assert_array_equal(got[2] * 4, [[0.5, 0.5], [1.5, 0.5], [0.5, 1.5]])


def test_unwrap_one_quad_puts_the_shared_edge_on_the_diagonal():
    vertices = np.random.default_rng(1).uniform(-1, 1, (4, 3)).astype(np.float32)
    got, tile_of = _unwrap_both(vertices, np.array([[0, 1, 2], [0, 2, 3]], np.int32), 6)
    assert got[4] == (8, 8) and tile_of.tolist() == [0, 0] and len(got[0]) == 4
    assert got[1].tolist() == [[0, 1, 2], [0, 2, 3]] and got[3].tolist() == [0, 1, 2, 3]
    # q1 alone at (0.5, 0.5), q2 and q0 on the diagonal, q3 opposite
    np.testing.assert_array_equal(got[2] * 8, [[0.5, 4.5], [0.5, 0.5], [4.5, 0.5], [4.5, 4.5]])


def test_unwrap_a_lone_cell_mesh():
    """12 triangles, 6 tiles, 24 vertices; 6 tiles of 4 x 4 need 16 x 8."""
    vertices, triangles = cube()
    got, tile_of = _unwrap_both(vertices, triangles, 4)
    assert len(got[0]) == 24 and got[4] == (8, 16) and tile_of.tolist() == sorted(2 * list(range(6)))
    texel = got[2][got[1]] * [16, 8]
    origin = np.floor(texel.min(1) / 4)
    assert np.array_equal(origin[:, 0] + 4 * origin[:, 1], tile_of)
    assert unwrap_mesh(vertices, triangles, 8)[4] == (16, 32)
    assert unwrap_mesh(vertices, triangles, 5)[4] == (16, 16)        # 16 x 8 holds three, 16 x 16 nine


def test_unwrap_an_odd_count_and_triangles_that_share_one_vertex():
    vertices = np.random.default_rng(2).uniform(-1, 1, (9, 3)).astype(np.float32)
    # a quad, two triangles with one vertex in common, a degenerate pair, a last lone triangle
    triangles = np.array([[2, 0, 1], [3, 0, 2], [4, 5, 6], [6, 7, 8], [0, 1, 1], [0, 1, 2],
                          [5, 3, 8]], np.int32)
    got, tile_of = _unwrap_both(vertices, triangles, 4)
    assert tile_of.tolist() == [0, 0, 1, 2, 3, 4, 5]
    assert len(got[0]) == 4 + 5 * 3 and got[4] == (8, 16)
    assert got[1][:2].tolist() == [[0, 1, 2], [3, 1, 0]]
    # triangles 1 and 2 share an edge but are not the pair (2k, 2k + 1): not joined
    shifted = np.array([[4, 5, 6], [2, 0, 1], [3, 0, 2]], np.int32)
    assert _unwrap_both(vertices, shifted, 4)[1].tolist() == [0, 1, 2]


def test_every_tap_stays_inside_the_winning_triangles_tile():
    """The integer statement of the atlas: whatever the roundings of the interpolated UV."""
    from fourier_feature_nets_amd.cameras import projection_matrices
    vertices, triangles = cube()
    total = 0
    for tile in (3, 4, 7):
        got, tile_of = _unwrap_both(vertices, triangles, tile)
        size = got[4]
        per_row = size[1] // tile
        for yaw, distance in ((0.3, 3.0), (2.1, 1.7), (4.0, 6.0)):
            proj = projection_matrices([R.camera(WIDTH, HEIGHT, yaw=yaw, pitch=-0.5,
                                                 distance=distance)])[0]
            tap_texel, tap_weight, _, _, _, ids = Rt.camera_taps(got[0], got[1], got[2], proj, WIDTH,
                                                                 HEIGHT, size)
            hit = np.flatnonzero(ids >= 0)
            number = tile_of[ids[hit]]
            row, col = tap_texel[hit] // size[1], tap_texel[hit] % size[1]
            assert (col // tile == (number % per_row)[:, None]).all()
            assert (row // tile == (number // per_row)[:, None]).all()
            assert len(np.unique(tap_texel[hit], axis=1)) and (tap_weight[hit] >= 0).all()
            # no clamping inside a tile: the four taps of a pixel are four texels
            assert (tap_texel[hit, 1] == tap_texel[hit, 0] + 1).all()
            assert (tap_texel[hit, 2] == tap_texel[hit, 0] + size[1]).all()
            total += len(hit)
    assert total > 2000


def test_bake_vertex_colors():
    vertices, triangles = cube()
    new_vertices, new_triangles, uvs, vertex_map, size = unwrap_mesh(vertices, triangles, 4)
    constant = np.tile(np.array([0.3, 0.6, 0.9], np.float32), (len(new_vertices), 1))
    texture = bake_vertex_colors(constant, new_triangles, uvs, size, 4)
    assert texture.shape == size + (3,) and texture.dtype == np.float32
    np.testing.assert_array_equal(texture, np.broadcast_to(constant[0], texture.shape))
    # colours linear in the position: a texel at a corner's texel coordinate holds its colour
    # within float64's rounding, texels between them the blend
    colors = (vertices[vertex_map] + 0.5).astype(np.float32) * 0.5 + 0.25
    texture = bake_vertex_colors(colors, new_triangles, uvs, size, 4)
    texel = uvs * [size[1], size[0]]
    for face in new_triangles[:2]:
        a, b = texel[face[0]], texel[face[1]]
        mid = 0.5 * (a + b)                                  # (0.5 + 2.5) / 2: between two texels
        lo, hi = np.floor(mid).astype(int), np.ceil(mid).astype(int)
        want = 0.5 * (colors[face[0]].astype(np.float64) + colors[face[1]])
        got = 0.5 * (texture[lo[1], lo[0]].astype(np.float64) + texture[hi[1], hi[0]])
        np.testing.assert_allclose(got, want, atol=1e-6)
    assert texture.min() >= 0 and texture.max() <= 1


def test_texture_to_uint8_and_the_quantisation_of_the_u8_path(world):
    """``texture_to_uint8`` then K31c's uint8 path against K33b on the float texture."""
    rng = np.random.default_rng(8)
    texture = rng.uniform(0, 1, (TEX_H, TEX_W, 3)).astype(np.float32)
    texture[0, 0], texture[0, 1] = 0.0, 1.0
    quantised = texture_to_uint8(texture)
    assert quantised.dtype == np.uint8 and quantised.shape == texture.shape
    want = np.clip(np.floor(texture.astype(np.float64) * 255 + 0.5), 0, 255)[::-1]
    assert np.abs(quantised.astype(np.float64) - want).max() <= 1      # f32 against f64 at a tie
    assert quantised[-1, 0].tolist() == [0, 0, 0] and quantised[-1, 1].tolist() == [255, 255, 255]
    odd = np.array([[[-0.5, 2.0, np.nan]]], np.float32)
    assert texture_to_uint8(odd).tolist() == [[[0, 255, 0]]]
    assert texture_to_uint8(torch.from_numpy(texture)).tolist() == quantised.tolist()

    zbuf = R.draw(world.state, WIDTH, HEIGHT)
    bytes_color = R.resolve(world.state, zbuf, world.vertices, world.eye, WIDTH, HEIGHT,
                            uvs=world.uvs, texture=quantised[::-1])[0]
    float_color, _ = Rt.gather(world.tap_texel, world.tap_weight, texture.reshape(-1, 3))
    hit = world.ids >= 0
    error = np.abs(bytes_color[hit].astype(np.float64) - float_color[hit].astype(np.float64)).max()
    budget = Rt.quantisation_budget()
    print("quantisation: worst %.6g, budget %.6g, share %.3f" % (error, budget, error / budget))
    assert 0 < error <= budget


# ------------------------------------------------------------------------------- OBJ
def test_save_obj_round_trip_with_a_texture(tmp_path):
    from fourier_feature_nets_amd import load_obj, save_obj
    vertices, triangles = cube()
    new_vertices, new_triangles, uvs, vertex_map, size = unwrap_mesh(vertices, triangles, 4)
    rng = np.random.default_rng(4)
    texture = rng.integers(0, 256, size + (3,), dtype=np.uint8)
    normals = rng.standard_normal(new_vertices.shape).astype(np.float32)
    for name, extra in (("plain.obj", None), ("normals.obj", normals)):
        path = str(tmp_path / name)
        save_obj(path, new_vertices, new_triangles, normals=extra, uvs=uvs, texture=texture)
        text = open(path).read()
        assert ("f 1/1/1 2/2/2 3/3/3" if extra is not None else "f 1/1 2/2 3/3") in text
        assert "mtllib %s.mtl" % name[:-4] in text and text.count("\nvt ") == len(uvs)
        assert "map_Kd %s.png" % name[:-4] in open(str(tmp_path / (name[:-4] + ".mtl"))).read()
        got = load_obj(path)
        np.testing.assert_array_equal(got[0].view(np.uint32), new_vertices.view(np.uint32))
        np.testing.assert_array_equal(got[1], new_triangles)
        np.testing.assert_array_equal(got[2].view(np.uint32), uvs.view(np.uint32))
        np.testing.assert_array_equal(got[3], texture)
        assert got[1].dtype == np.int32 and got[2].dtype == np.float32


def test_save_obj_without_the_new_arguments_writes_what_it_wrote(tmp_path):
    from fourier_feature_nets_amd import save_obj
    vertices = np.array([[0, 0.5, 1], [1, 0, 0.25], [0.125, 1, 0]], np.float32)
    triangles = np.array([[0, 1, 2]], np.int32)
    colors = np.array([[1, 0, 0], [0, 0.5, 0], [0, 0, 0.25]], np.float32)
    normals = np.array([[0, 0, 1], [0, 1, 0], [1, 0, 0]], np.float32)
    head = "# 3 vertices, 1 triangles\n"
    cases = {
        "bare": (dict(), head + "v 0 0.5 1\nv 1 0 0.25\nv 0.125 1 0\nf 1 2 3\n"),
        "colors": (dict(colors=colors), head + "v 0 0.5 1 1 0 0\nv 1 0 0.25 0 0.5 0\n"
                   "v 0.125 1 0 0 0 0.25\nf 1 2 3\n"),
        "both": (dict(colors=colors, normals=normals),
                 head + "v 0 0.5 1 1 0 0\nv 1 0 0.25 0 0.5 0\nv 0.125 1 0 0 0 0.25\n"
                 "vn 0 0 1\nvn 0 1 0\nvn 1 0 0\nf 1//1 2//2 3//3\n"),
    }
    for name, (kwargs, want) in cases.items():
        path = tmp_path / (name + ".obj")
        save_obj(str(path), vertices, triangles, **kwargs)
        assert path.read_bytes() == want.encode(), name
    assert sorted(p.name for p in tmp_path.iterdir()) == ["bare.obj", "both.obj", "colors.obj"]


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
    triangles = torch.zeros((5, 3), dtype=torch.int32)
    uvs = torch.zeros((7, 2), dtype=torch.float32)
    check = ops.mesh_texture_taps_check
    check(record, ids, triangles, uvs, 8, 4, 4, 3)
    _raises("record", check, record[:4], ids, triangles, uvs, 8, 4, 4, 3)
    _raises("record", check, record.to(torch.int64), ids, triangles, uvs, 8, 4, 4, 3)
    _raises("ids", check, record, ids[:11], triangles, uvs, 8, 4, 4, 3)
    _raises("ids", check, record, ids.float(), triangles, uvs, 8, 4, 4, 3)
    _raises("triangles", check, record, ids, triangles.to(torch.int64), uvs, 8, 4, 4, 3)
    _raises("triangles", check, record[:0], ids, triangles[:0], uvs, 8, 4, 4, 3)
    _raises("uvs", check, record, ids, triangles, uvs.double(), 8, 4, 4, 3)
    _raises("uvs", check, record, ids, triangles, torch.zeros((7, 3)), 8, 4, 4, 3)
    _raises("uvs", check, record, ids, triangles, uvs.numpy(), 8, 4, 4, 3)
    _raises("texture", check, record, ids, triangles, uvs, 0, 4, 4, 3)
    _raises("texture", check, record, ids, triangles, uvs, 8, (1 << 24) + 1, 4, 3)
    _raises("texture", check, record, ids, triangles, uvs, 1 << 16, 1 << 16, 4, 3)
    _raises("width", check, record, ids, triangles, uvs, 8, 4, 0, 3)
    _raises("width", check, record, ids, triangles, uvs, 8, 4, 4, 16385)

    tap_texel = torch.zeros((12, 4), dtype=torch.int32)
    tap_weight = torch.zeros((12, 4), dtype=torch.float32)
    texture = torch.zeros((32, 3), dtype=torch.float32)
    check = ops.mesh_texture_gather_check
    check(tap_texel, tap_weight, texture, (0, 0, 0))
    _raises("tap_texel", check, tap_texel.to(torch.int64), tap_weight, texture, (0, 0, 0))
    _raises("tap_texel", check, tap_texel[:, :3].contiguous(), tap_weight, texture, (0, 0, 0))
    _raises("tap_texel", check, tap_texel[:0], tap_weight[:0], texture, (0, 0, 0))
    _raises("tap_weight", check, tap_texel, tap_weight[:11], texture, (0, 0, 0))
    _raises("tap_weight", check, tap_texel, tap_weight.double(), texture, (0, 0, 0))
    _raises("texture", check, tap_texel, tap_weight, texture.reshape(8, 4, 3), (0, 0, 0))
    _raises("texture", check, tap_texel, tap_weight, texture.to(torch.uint8), (0, 0, 0))
    _raises("texture", check, tap_texel, tap_weight, texture[:0], (0, 0, 0))
    _raises("background", check, tap_texel, tap_weight, texture, (0, 0))
    _raises("background", check, tap_texel, tap_weight, texture, (0, float("nan"), 0))

    sorted_texels = torch.zeros((48,), dtype=torch.int32)
    order = torch.zeros((48,), dtype=torch.int32)
    d_color = torch.zeros((12, 3), dtype=torch.float32)
    grad, weight = torch.zeros((32, 3)), torch.zeros((32,))
    check = ops.mesh_texture_grad_check
    assert check(sorted_texels, order, tap_weight, d_color, 32) == 12
    assert check(sorted_texels, order, tap_weight, d_color, 32, grad, weight, True) == 12
    _raises("sorted_texels", check, sorted_texels[:47], order, tap_weight, d_color, 32)
    _raises("sorted_texels", check, sorted_texels.to(torch.int64), order, tap_weight, d_color, 32)
    _raises("tap_order", check, sorted_texels, order.to(torch.int64), tap_weight, d_color, 32)
    _raises("tap_order", check, sorted_texels, order[:12], tap_weight, d_color, 32)
    _raises("tap_weight", check, sorted_texels, order, tap_weight.reshape(-1), d_color, 32)
    _raises("d_color", check, sorted_texels, order, tap_weight, d_color[:11], 32)
    _raises("d_color", check, sorted_texels, order, tap_weight, d_color.double(), 32)
    _raises("num_texels", check, sorted_texels, order, tap_weight, d_color, 0)
    _raises("num_texels", check, sorted_texels, order, tap_weight, d_color, 2 ** 31)
    _raises("grad", check, sorted_texels, order, tap_weight, d_color, 32, grad[:31], weight)
    _raises("weight", check, sorted_texels, order, tap_weight, d_color, 32, grad, weight[:31])
    _raises("weight", check, sorted_texels, order, tap_weight, d_color, 32, grad, None)
    _raises("accumulate", check, sorted_texels, order, tap_weight, d_color, 32, None, None, True)


def _stand_in(images, cameras):
    return types.SimpleNamespace(images=images, cameras=cameras, color_space="RGB")


def test_mesh_functions_refuse_before_any_device(no_device, tmp_path):
    import fourier_feature_nets_amd as ffn
    vertices, triangles = R.quad_scene()
    uvs = np.array([[0, 0], [1, 0], [1, 1], [0, 1]], np.float32)
    cam = R.camera(6, 5)
    texture = np.full((4, 4, 3), 0.5, dtype=np.float32)
    images = np.zeros((2, 5, 6, 4), dtype=np.uint8)
    data = _stand_in(images, [cam, cam])

    _raises("vertices", unwrap_mesh, vertices[:, :2], triangles)
    _raises("triangles", unwrap_mesh, vertices, triangles + 9)
    _raises("triangles", unwrap_mesh, vertices, triangles.astype(np.float32))
    _raises("tile", unwrap_mesh, vertices, triangles, 2)
    _raises("tile", unwrap_mesh, vertices, triangles, 4.5)

    colors = R.grey(vertices)
    _raises("colors", bake_vertex_colors, colors[:, :2], triangles, uvs, (4, 4), 4)
    _raises("uvs", bake_vertex_colors, colors, triangles, uvs[:3], (4, 4), 4)
    _raises("tile", bake_vertex_colors, colors, triangles, uvs, (4, 4), 2)
    _raises("size", bake_vertex_colors, colors, triangles, uvs, (2, 4), 4)
    _raises("outside", bake_vertex_colors, colors, triangles, uvs + 2, (4, 4), 4)

    _raises("texture", texture_to_uint8, np.zeros((4, 4, 3), np.uint8))
    _raises("texture", texture_to_uint8, np.zeros((4, 4), np.float32))

    taps = mesh_texture_taps
    _raises("supersample", taps, vertices, triangles, uvs, cam, (4, 4), supersample=2)
    _raises("uvs", taps, vertices, triangles, uvs[:3], cam, (4, 4))
    _raises("uvs", taps, vertices, triangles, None, cam, (4, 4))
    _raises("vertices", taps, vertices[:, :2], triangles, uvs, cam, (4, 4))
    _raises("camera", taps, vertices, triangles, uvs, "front", (4, 4))
    _raises("size", taps, vertices, triangles, uvs, cam, 4)
    _raises("texture", taps, vertices, triangles, uvs, cam, (0, 4))
    _raises("texture", taps, vertices, triangles, uvs, cam, (1 << 16, 1 << 16))
    _raises("batch_size", taps, vertices, triangles, uvs, cam, (4, 4), batch_size=0)
    _raises("triangles", taps, vertices, triangles + 9, uvs, cam, (4, 4))

    made = MeshTaps(torch.full((30, 4), -1, dtype=torch.int32), torch.zeros((30, 4)),
                    torch.full((120,), -1, dtype=torch.int32),
                    torch.arange(120, dtype=torch.int32), 4, 4)
    _raises("taps", render_mesh_texture, (made.tap_texel, made.tap_weight), texture)
    _raises("texture", render_mesh_texture, made, (255 * texture).astype(np.uint8))
    _raises("texture", render_mesh_texture, made, texture[..., :2])
    _raises("texture", render_mesh_texture, made, texture.reshape(-1, 3))
    _raises("texture", render_mesh_texture, made, texture[:3])
    _raises("background", render_mesh_texture, made, texture, (0, 0))
    back = render_mesh_texture_backward
    d_color = np.zeros((30, 3), dtype=np.float32)
    _raises("taps", back, None, d_color)
    _raises("d_color", back, made, d_color[:29])
    _raises("accumulate", back, made, d_color, accumulate=True)
    _raises("grad", back, made, d_color, torch.zeros((4, 4, 3)), None)
    _raises("grad", back, made, d_color, torch.zeros((3, 4, 3)), torch.zeros((4, 4)))

    splat = texture_mesh_from_images
    _raises("alpha_threshold", splat, vertices, triangles, uvs, data, (4, 4), alpha_threshold=2.0)
    _raises("images", splat, vertices, triangles, uvs, _stand_in(images[0], [cam]), (4, 4))
    _raises("camera", splat, vertices, triangles, uvs,
            _stand_in(images, [cam, R.camera(7, 5)]), (4, 4))
    _raises("uvs", splat, vertices, triangles, uvs[:, :1], data, (4, 4))
    _raises("size", splat, vertices, triangles, uvs, data, None)
    _raises("texture", splat, vertices, triangles, uvs, data, (4, 4), texture=texture[:2])
    _raises("texture", splat, vertices, triangles, uvs, data, (4, 4),
            texture=np.zeros((4, 4, 3), np.uint8))

    fit = fit_mesh_texture
    _raises("texture", fit, vertices, triangles, uvs, None, data)
    _raises("texture", fit, vertices, triangles, uvs, np.zeros((4, 4, 3), np.uint8), data)
    _raises("texture", fit, vertices, triangles, uvs, texture[..., 0], data)
    _raises("uvs", fit, vertices, triangles, None, texture, data)
    _raises("learning_rate", fit, vertices, triangles, uvs, texture, data, learning_rate=0.0)
    _raises("learning_rate", fit, vertices, triangles, uvs, texture, data,
            learning_rate=float("nan"))
    _raises("cameras_per_step", fit, vertices, triangles, uvs, texture, data, cameras_per_step=0)
    _raises("alpha_threshold", fit, vertices, triangles, uvs, texture, data, alpha_threshold=1.5)
    _raises("cameras", fit, vertices, triangles, uvs, texture, _stand_in(images, [cam]))
    _raises("val_dataset", fit, vertices, triangles, uvs, texture, data,
            _stand_in(images[..., :2], [cam, cam]))
    _raises("alpha", fit, vertices, triangles, uvs, texture,
            _stand_in(images[..., :3], [cam, cam]), alpha_threshold=0.5)
    _raises("triangles", fit, vertices, triangles + 9, uvs, texture, data)

    path = str(tmp_path / "refused.obj")
    _raises("uvs", ffn.save_obj, path, vertices, triangles, uvs=uvs)
    _raises("uvs", ffn.save_obj, path, vertices, triangles, uvs=uvs[:3],
            texture=np.zeros((4, 4, 3), np.uint8))
    _raises("texture", ffn.save_obj, path, vertices, triangles, uvs=uvs, texture=texture)
    assert not list(tmp_path.iterdir())


# ------------------------------------------------------------------------------- the ABI
def test_header_declares_and_ops_binds_the_entry_points():
    from fourier_feature_nets_amd import _lib, ops
    from tests import stream_helpers
    import fourier_feature_nets
    import fourier_feature_nets_amd
    for name, wrapper in (("ffn_mesh_texture_taps", ops.mesh_texture_taps),
                          ("ffn_mesh_texture_gather", ops.mesh_texture_gather),
                          ("ffn_mesh_texture_grad", ops.mesh_texture_grad)):
        assert name in _lib.declared_symbols()
        assert name in stream_helpers.stream_entry_points()
        assert '"%s"' % name in inspect.getsource(wrapper)
    assert _lib.ABI_VERSION == 3
    for name in ("MeshTaps", "unwrap_mesh", "bake_vertex_colors", "mesh_texture_taps",
                 "render_mesh_texture", "render_mesh_texture_backward",
                 "texture_mesh_from_images", "fit_mesh_texture", "texture_to_uint8"):
        assert name in fourier_feature_nets_amd.__all__
        assert getattr(fourier_feature_nets, name) is getattr(fourier_feature_nets_amd, name)
    assert list(inspect.signature(fourier_feature_nets_amd.save_obj).parameters)[-2:] \
        == ["uvs", "texture"]


def test_the_stream_order_table_holds_a_case_for_each_entry_point():
    """tests/stream_order_cases_mesh_texture.py has added its three cases to the table that
    tests/test_stream_order_cpu.py holds to the header, each once."""
    from tests.stream_order_cases import CASES
    reached = [name for c in CASES for name in c.reaches]
    names = [c.name for c in CASES]
    for name in ("mesh_texture_taps", "mesh_texture_gather", "mesh_texture_grad"):
        assert reached.count("ffn_" + name) == 1 and names.count(name) == 1
