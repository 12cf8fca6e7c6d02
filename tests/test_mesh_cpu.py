"""K22 without a GPU: the numpy restatement (tests/mesh_reference.py) against a property it was not
written from, the host layer of ``fourier_feature_nets_amd/mesh.py`` (normalisation, per-triangle
counts, the OBJ reader) and the argument refusals of ``ops.mesh_sample`` that need no device."""

import numpy as np
import pytest
import torch

from tests import mesh_reference as mref


# ------------------------------------------------------------------------------- restatement
@pytest.mark.parametrize("m", [1, 2, 3, 4, 5])
def test_restatement_one_point_per_subtriangle(m):
    """Basu and Owen's construction puts the first 4^m points one into each of the 4^m congruent
    sub-triangles of side 2^-m; here for the numbers 1 .. 4^m the kernel uses (the sequence
    without its point 0).  A sub-triangle is named by the cell of p.x, of p.y and of p.x + p.y."""
    count = 4 ** m
    p = mref.triangle_points(np.arange(1, count + 1)).astype(np.float64)
    weights = mref.barycentric(p.astype(np.float32))
    assert (weights > 0).all()                       # strictly inside, in float32
    side = 2.0 ** m
    keys = np.stack([np.floor(p[:, 0] * side), np.floor(p[:, 1] * side),
                     np.floor((p[:, 0] + p[:, 1]) * side)], -1).astype(np.int64)
    assert len(np.unique(keys, axis=0)) == count


def test_restatement_numbers_skip_empty_triangles():
    triangle, number = mref.sample_numbers([0, 2, 0, 0, 3, 0])
    assert triangle.tolist() == [1, 1, 4, 4, 4]
    assert number.tolist() == [1, 2, 1, 2, 3]


# ------------------------------------------------------------------------------- normalize
def _cloud(seed=3, n=200):
    rng = np.random.default_rng(seed)
    return rng.normal(size=(n, 3)) * [3.0, 0.5, 1.5] + [10.0, -4.0, 2.0]


def test_normalize_points_extent_and_centre():
    from fourier_feature_nets import normalize_points
    for up in ((0, 1, 0), (0, 0, 1), (1, 2, -0.5)):
        out = normalize_points(_cloud(), up)
        assert out.dtype == np.float32 and out.shape == (200, 3)
        wide = out.astype(np.float64)
        extent = wide.max(0) - wide.min(0)
        # float64 arithmetic, one rounding to float32 per coordinate: 2^-24 relative at |x| <= 0.8
        assert abs(extent.max() - 1.6) <= 2 * 0.8 * 2.0 ** -24
        assert np.abs(wide.max(0) + wide.min(0)).max() <= 2 * 0.8 * 2.0 ** -24


def test_normalize_points_rotates_up_onto_y():
    from fourier_feature_nets import normalize_points
    # a bar along +z with its heavy end up: after up_dir = +z it stands along +y, same end up
    bar = np.array([[0, 0, 0], [0.1, 0, 0], [0, 0.1, 0], [0, 0, 4.0], [0.1, 0, 4.0]])
    out = normalize_points(bar, (0, 0, 1)).astype(np.float64)
    extent = out.max(0) - out.min(0)
    assert extent.argmax() == 1
    assert out[3, 1] > 0.79 and out[0, 1] < -0.79
    np.testing.assert_allclose(out[3] - out[0], [0, 1.6, 0], atol=1e-6)
    # the identity rotation leaves the directions alone, and a scaled up_dir is the same direction
    same = normalize_points(bar, (0, 1, 0)).astype(np.float64)
    np.testing.assert_allclose(same[3] - same[0], [0, 0, 1.6], atol=1e-6)
    np.testing.assert_array_equal(normalize_points(bar, (0, 0, 5)), normalize_points(bar, (0, 0, 1)))


def test_normalize_points_refusals():
    from fourier_feature_nets import normalize_points
    with pytest.raises(ValueError, match="opposite"):
        normalize_points(_cloud(), (0, -1, 0))
    with pytest.raises(ValueError, match="up_dir"):
        normalize_points(_cloud(), (0, 0, 0))
    with pytest.raises(ValueError, match="vertices"):
        normalize_points(np.zeros((4, 2)))
    with pytest.raises(ValueError, match="coincide"):
        normalize_points(np.ones((4, 3)))


# ------------------------------------------------------------------------------- counts
def test_triangle_counts():
    from fourier_feature_nets import triangle_counts
    vertices = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [2, 0, 0], [3, 0, 0], [0, 3, 0]], float)
    #                      area 0.5   a line     a point    area 4.5   a line (last)
    triangles = np.array([[0, 1, 2], [0, 1, 3], [4, 4, 4], [0, 4, 5], [0, 3, 4]])
    counts = triangle_counts(vertices, triangles, 10000, seed=1)
    assert counts.dtype == np.int64 and counts.shape == (5,)
    assert counts.sum() == 10000
    assert counts[1] == 0 and counts[2] == 0 and counts[4] == 0
    # shares 0.1 and 0.9: a binomial with sigma = 30, so 6 sigma either way
    assert abs(int(counts[0]) - 1000) < 180
    np.testing.assert_array_equal(counts, triangle_counts(vertices, triangles, 10000, seed=1))
    assert not np.array_equal(counts, triangle_counts(vertices, triangles, 10000, seed=2))
    assert triangle_counts(vertices, triangles, 0).sum() == 0
    with pytest.raises(ValueError, match="no surface"):
        triangle_counts(vertices, triangles[[1, 2]], 10)
    with pytest.raises(ValueError, match="triangles"):
        triangle_counts(vertices, np.array([[0, 1, 6]]), 10)


def test_procedural_torus():
    from fourier_feature_nets import procedural_torus
    vertices, triangles, uvs, texture = procedural_torus(16, 8, 32)
    assert vertices.shape == (17 * 9, 3) and vertices.dtype == np.float32
    assert triangles.shape == (2 * 16 * 8, 3) and triangles.dtype == np.int32
    assert uvs.shape == (17 * 9, 2) and uvs.dtype == np.float32
    assert texture.shape == (32, 32, 3) and texture.dtype == np.uint8
    assert triangles.min() == 0 and triangles.max() == len(vertices) - 1
    assert uvs.min() == 0.0 and uvs.max() == 1.0
    # every vertex on the torus of radii 1 and 0.4 round +y
    ring = np.hypot(vertices[:, 0], vertices[:, 2]) - 1.0
    np.testing.assert_allclose(np.hypot(ring, vertices[:, 1]), 0.4, atol=1e-6)
    # no triangle crosses the seam: its UVs span one quad
    span = uvs[triangles].max(1) - uvs[triangles].min(1)
    np.testing.assert_allclose(span, np.broadcast_to([1 / 16, 1 / 8], span.shape), atol=1e-6)
    # smooth: neighbouring texels (wrapping round) differ by little
    wide = texture.astype(np.int32)
    for axis in (0, 1):
        assert np.abs(wide - np.roll(wide, 1, axis)).max() <= 48


# ------------------------------------------------------------------------------- load_obj
def _corner_arrays(mesh):
    vertices, triangles, uvs, _ = mesh
    assert vertices.dtype == np.float32 and uvs.dtype == np.float32
    assert triangles.dtype == np.int32 and triangles.ndim == 2 and triangles.shape[1] == 3
    assert len(vertices) == len(uvs)
    return vertices[triangles], uvs[triangles]


def _white(texture):
    return texture.shape == (1, 1, 3) and texture.dtype == np.uint8 and (texture == 255).all()


def _png(path, height=3, width=2, seed=0):
    from PIL import Image
    pixels = np.random.default_rng(seed).integers(0, 256, (height, width, 3), dtype=np.uint8)
    Image.fromarray(pixels).save(path)
    return pixels


QUAD_V = np.float32([[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 2, 0.25]])
QUAD_VT = np.float32([[0, 0], [1, 0], [1, 1], [0, 1], [0.5, 0.75]])


def _write_obj(path, faces, vt=True, header=""):
    lines = [header, "# a comment", "o thing"]
    lines += ["v %r %r %r" % tuple(float(x) for x in v) for v in QUAD_V]
    if vt:
        lines += ["vt %r %r" % tuple(float(x) for x in t) for t in QUAD_VT]
    lines += ["vn 0 0 1", "s off"] + faces
    path.write_text("\n".join(lines) + "\n")


def test_load_obj_quads_and_polygons(tmp_path):
    from fourier_feature_nets import load_obj
    texture = _png(tmp_path / "t.png")
    _write_obj(tmp_path / "m.obj", ["f 1/1 2/2 3/3 4/4", "f 4/4 3/3 5/5"])
    mesh = load_obj(str(tmp_path / "m.obj"), str(tmp_path / "t.png"))
    positions, coords = _corner_arrays(mesh)
    fan = [[0, 1, 2], [0, 2, 3], [3, 2, 4]]
    np.testing.assert_array_equal(positions, QUAD_V[fan])
    np.testing.assert_array_equal(coords, QUAD_VT[fan])
    assert len(mesh[0]) == 5                     # five distinct (v, vt) pairs
    np.testing.assert_array_equal(mesh[3], texture)


def test_load_obj_normals_and_negative_indices(tmp_path):
    from fourier_feature_nets import load_obj
    _png(tmp_path / "t.png")
    # -5 is the first of five vertices / texture coordinates, -1 the last
    _write_obj(tmp_path / "m.obj", ["f -5/-5/1 -4/-4/-1 -3/-3/1", "f 1/-2/1 3//1 -1/5/1"])
    positions, coords = _corner_arrays(load_obj(str(tmp_path / "m.obj"), str(tmp_path / "t.png")))
    np.testing.assert_array_equal(positions, QUAD_V[[[0, 1, 2], [0, 2, 4]]])
    # (the corner without a vt has the UV (0, 0))
    np.testing.assert_array_equal(coords, [QUAD_VT[[0, 1, 2]], [QUAD_VT[3], [0, 0], QUAD_VT[4]]])
    for bad in ("f 1/1 2/2 6/1", "f 1/1 2/2 0/1", "f 1/1 2/2 -6/1", "f 1/1 2/9 3/3"):
        _write_obj(tmp_path / "bad.obj", [bad])
        with pytest.raises(ValueError, match="index"):
            load_obj(str(tmp_path / "bad.obj"))


def test_load_obj_one_vertex_two_texture_coordinates(tmp_path):
    from fourier_feature_nets import load_obj
    _png(tmp_path / "t.png")
    _write_obj(tmp_path / "m.obj", ["f 1/1 2/2 3/3", "f 1/5 3/3 4/4"])
    mesh = load_obj(str(tmp_path / "m.obj"), str(tmp_path / "t.png"))
    positions, coords = _corner_arrays(mesh)
    np.testing.assert_array_equal(positions, QUAD_V[[[0, 1, 2], [0, 2, 3]]])
    np.testing.assert_array_equal(coords, QUAD_VT[[[0, 1, 2], [4, 2, 3]]])
    # vertex 1 twice (two vt), vertex 3 once (the same vt both times): 5 rows
    assert len(mesh[0]) == 5
    assert mesh[1][0, 0] != mesh[1][1, 0] and mesh[1][0, 2] == mesh[1][1, 1]


def test_load_obj_texture_through_mtl(tmp_path):
    from fourier_feature_nets import load_obj
    texture = _png(tmp_path / "skin.png", 4, 5, seed=2)
    (tmp_path / "m.mtl").write_text("# material\nnewmtl skin\nKd 1 1 1\nmap_Kd skin.png\n"
                                    "newmtl other\nmap_Kd missing.png\n")
    _write_obj(tmp_path / "m.obj", ["usemtl skin", "f 1/1 2/2 3/3"], header="mtllib m.mtl")
    mesh = load_obj(str(tmp_path / "m.obj"))
    np.testing.assert_array_equal(mesh[3], texture)
    np.testing.assert_array_equal(_corner_arrays(mesh)[1], QUAD_VT[[[0, 1, 2]]])
    # texture_path wins over the library
    other = _png(tmp_path / "other.png", 2, 2, seed=5)
    np.testing.assert_array_equal(load_obj(str(tmp_path / "m.obj"), str(tmp_path / "other.png"))[3],
                                  other)
    # an RGBA file keeps its four channels (K22 ignores the fourth)
    from PIL import Image
    rgba = np.random.default_rng(7).integers(0, 256, (2, 3, 4), dtype=np.uint8)
    Image.fromarray(rgba).save(tmp_path / "rgba.png")
    np.testing.assert_array_equal(load_obj(str(tmp_path / "m.obj"), str(tmp_path / "rgba.png"))[3],
                                  rgba)


def test_load_obj_without_texture_coordinates(tmp_path):
    from fourier_feature_nets import load_obj
    _write_obj(tmp_path / "m.obj", ["f 1 2 3", "f 1//1 3//1 4//1"], vt=False)
    mesh = load_obj(str(tmp_path / "m.obj"))
    positions, coords = _corner_arrays(mesh)
    np.testing.assert_array_equal(positions, QUAD_V[[[0, 1, 2], [0, 2, 3]]])
    assert (coords == 0).all() and len(mesh[0]) == 4 and _white(mesh[3])
    # texture coordinates but no texture: the same
    _write_obj(tmp_path / "n.obj", ["f 1/1 2/2 3/3", "f 1/5 3/3 4/4"])
    mesh = load_obj(str(tmp_path / "n.obj"))
    assert (mesh[2] == 0).all() and len(mesh[0]) == 4 and _white(mesh[3])
    # a texture but no texture coordinates: the same
    _png(tmp_path / "t.png")
    mesh = load_obj(str(tmp_path / "m.obj"), str(tmp_path / "t.png"))
    assert (mesh[2] == 0).all() and _white(mesh[3])
    _write_obj(tmp_path / "empty.obj", [])
    with pytest.raises(ValueError, match="no faces"):
        load_obj(str(tmp_path / "empty.obj"))


# ------------------------------------------------------------------------------- refusals
def _arguments():
    return dict(vertices=torch.zeros((4, 3)), triangles=torch.tensor([[0, 1, 2], [1, 2, 3]],
                                                                     dtype=torch.int32),
                uvs=torch.zeros((4, 2)), offsets=torch.tensor([0, 3, 5], dtype=torch.int32),
                texture=torch.zeros((2, 2, 3), dtype=torch.uint8))


@pytest.mark.parametrize("name, value, match", [
    ("triangles", torch.tensor([[0, 1, 2], [1, 2, 4]], dtype=torch.int32), "triangles"),
    ("triangles", torch.tensor([[0, -1, 2], [1, 2, 3]], dtype=torch.int32), "triangles"),
    ("triangles", torch.tensor([[0, 1, 2], [1, 2, 3]], dtype=torch.int64), "triangles"),
    ("offsets", torch.tensor([0, 3, 5, 6], dtype=torch.int32), "offsets"),
    ("offsets", torch.tensor([0, 5, 3], dtype=torch.int32), "offsets"),
    ("offsets", torch.tensor([1, 3, 5], dtype=torch.int32), "offsets"),
    ("offsets", torch.tensor([0, 0, 0], dtype=torch.int32), "offsets"),
    ("offsets", torch.tensor([0, 1 << 24, (1 << 24) + 1], dtype=torch.int32), "offsets"),
    ("texture", torch.zeros((2, 2, 2), dtype=torch.uint8), "texture"),
    ("texture", torch.zeros((2, 2), dtype=torch.uint8), "texture"),
    ("texture", torch.zeros((2, 2, 3)), "texture"),
    ("uvs", torch.tensor([[0, 0], [0, float("nan")], [0, 0], [0, 0]]), "uvs"),
    ("uvs", torch.tensor([[0, 0], [float("inf"), 0], [0, 0], [0, 0]]), "uvs"),
    ("uvs", torch.zeros((3, 2)), "uvs"),
    ("vertices", torch.zeros((4, 3), dtype=torch.float64), "vertices"),
    ("vertices", torch.zeros((4, 3, 1)), "vertices"),
])
def test_mesh_sample_refusals(name, value, match):
    """Bad input is a ValueError that names the argument, before any device is asked for (these
    tensors live on the host: a launch would raise a RuntimeError instead)."""
    from fourier_feature_nets_amd import ops
    arguments = _arguments()
    arguments[name] = value
    with pytest.raises(ValueError, match=match):
        ops.mesh_sample(**arguments)


def test_mesh_sample_is_declared():
    from fourier_feature_nets_amd import _lib, ops
    assert "ffn_mesh_sample" in _lib.declared_symbols()
    # good arguments pass the checks and reach the device requirement
    assert ops.mesh_sample_check(**_arguments()) == 5
    with pytest.raises(RuntimeError, match="GPU"):
        ops.mesh_sample(**_arguments())


def test_build_from_triangles_refusals():
    from fourier_feature_nets import OcTree, procedural_torus
    mesh = procedural_torus(4, 3, 2)
    for depth, leaf in ((1, 4), (12, 4), (5, 0)):
        with pytest.raises(ValueError, match="voxel_depth"):
            OcTree.build_from_triangles(*mesh, depth, leaf)
    with pytest.raises(ValueError, match="opposite"):
        OcTree.build_from_triangles(*mesh, 3, 4, up_dir=(0, -1, 0))
    # the path-taking entry stays the stub it was
    with pytest.raises(NotImplementedError, match="build_from_mesh"):
        OcTree.build_from_mesh("no_such_file.obj", 5, 4)
