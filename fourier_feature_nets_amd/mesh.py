"""Textured triangle meshes as a source of octrees: read or make one, normalise it, decide how many
samples every triangle gets and draw them on the GPU (K22, ``csrc/mesh.hip``).

The reference does all of this inside ``OcTree.build_from_mesh`` (octree.py:42-197, 807-853) with
trimesh, numba and numpy on the host.  Here the steps are separate functions and only the hot one,
drawing the samples, is a kernel:

* ``load_obj`` reads a Wavefront OBJ (trimesh is not a dependency); ``procedural_torus`` makes a
  mesh with a smooth texture from nothing.  Both return ``(vertices, triangles, uvs, texture)``:
  (V,3) float32, (F,3) int32, (V,2) float32, (H,W,C) uint8 with row 0 at the TOP of the image, as
  an image file stores it (``OcTree.build_from_triangles`` flips it, as the reference does).
* ``normalize_points`` is the reference's ``_normalize_points`` in float64.
* ``triangle_counts`` draws the per-triangle sample counts, proportional to area, from a seeded
  multinomial: the distribution of the reference's unseeded ``choice`` + ``bincount``
  (octree.py:128-129) in O(F), and the same counts for the same seed.
* ``sample_mesh`` turns the counts into offsets and runs K22; the cloud stays on the GPU.

``OcTree.build_from_triangles`` chains them into a colour octree.  ``save_obj`` is the way back: it
writes what ``OcTree.extract_mesh`` (K30) returns, with per-vertex colours and normals.

``render_mesh`` and ``render_mesh_image`` look at a mesh: a z-buffer rasteriser on the GPU (K31,
``csrc/mesh_raster.hip``) that draws per-vertex colours or a texture from a ``CameraInfo`` and
returns what ``OcTree.render`` and ``OcTree.render_image`` return.  No counterpart in the reference.
"""

import os
from typing import Optional, Tuple

import numpy as np
import torch

from . import ops

Mesh = Tuple[np.ndarray, np.ndarray, np.ndarray, np.ndarray]


def normalize_points(vertices, up_dir=(0, 1, 0)) -> np.ndarray:
    """Rotates ``up_dir`` onto +y, centres the vertices on their mean, scales the longest extent
    of the bounding box to 1.6 and centres the box on the origin (octree.py:155-197), in float64.
    -> (V,3) float32.  ``up_dir`` is normalised first (the reference assumes a unit vector); the
    direction opposite to +y has no such rotation (``1 + cos = 0``) and is a ``ValueError``."""
    points = np.asarray(vertices, dtype=np.float64)
    if points.ndim != 2 or points.shape[1] != 3 or len(points) == 0:
        raise ValueError("normalize_points: vertices must be (V,3) with V >= 1, got %s"
                         % (points.shape,))
    if not np.isfinite(points).all():
        raise ValueError("normalize_points: vertices holds a NaN or an infinity")
    up = np.asarray(up_dir, dtype=np.float64).reshape(-1)
    length = np.linalg.norm(up) if up.shape == (3,) else 0.0
    if not 0.0 < length < np.inf:
        raise ValueError("normalize_points: up_dir must be three finite numbers, not all zero, "
                         "got %r" % (up_dir,))
    up = up / length
    target = np.array([0.0, 1.0, 0.0])
    v = np.cross(up, target)
    cos = float(up @ target)
    if 1.0 + cos <= 1e-12:
        raise ValueError("normalize_points: up_dir %r is opposite to +y; the rotation onto +y is "
                         "not defined (1 + cos = 0)" % (up_dir,))
    vx = np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])
    rotation = np.eye(3) + vx + (1.0 / (1.0 + cos)) * (vx @ vx)
    points = (points - points.mean(0)) @ rotation.T
    extent = (points.max(0) - points.min(0)).max()
    if not extent > 0.0:
        raise ValueError("normalize_points: the vertices all coincide")
    points = points * (1.6 / extent)
    points = points - 0.5 * (points.max(0) + points.min(0))
    return points.astype(np.float32)


def _check_triangles(who: str, triangles, num_vertices: int) -> np.ndarray:
    triangles = np.asarray(triangles)
    if (triangles.ndim != 2 or triangles.shape[1] != 3 or len(triangles) == 0
            or not np.issubdtype(triangles.dtype, np.integer)):
        raise ValueError("%s: triangles must be an integer (F,3) array with F >= 1, got %s %s"
                         % (who, triangles.dtype, triangles.shape))
    if triangles.min() < 0 or triangles.max() >= num_vertices:
        raise ValueError("%s: triangles indexes vertices %d .. %d, outside 0 .. %d"
                         % (who, triangles.min(), triangles.max(), num_vertices - 1))
    return triangles


def triangle_counts(vertices, triangles, num_points: int, seed: int = 0) -> np.ndarray:
    """How many of ``num_points`` samples every triangle gets -> (F,) int64 that sums to
    ``num_points``: one draw of ``np.random.default_rng(seed).multinomial`` with probabilities
    proportional to the float64 areas.  A triangle of area zero gets 0."""
    points = np.asarray(vertices, dtype=np.float64)
    triangles = _check_triangles("triangle_counts", triangles, len(points))
    num_points = int(num_points)
    if num_points < 0:
        raise ValueError("triangle_counts: num_points must be >= 0, got %d" % num_points)
    corners = points[triangles]
    normals = np.cross(corners[:, 2] - corners[:, 0], corners[:, 1] - corners[:, 0])
    area = 0.5 * np.linalg.norm(normals, axis=-1)
    # (only triangles with area take part, so that the remainder numpy gives the last entry
    # cannot land on an empty one)
    solid = np.flatnonzero(area > 0.0)
    if len(solid) == 0 or not np.isfinite(area).all():
        raise ValueError("triangle_counts: the mesh has no surface (every triangle has area zero, "
                         "or a vertex is not finite)")
    share = area[solid] / area[solid].sum()
    counts = np.zeros(len(triangles), dtype=np.int64)
    counts[solid] = np.random.default_rng(seed).multinomial(num_points, share)
    return counts


def sample_mesh(vertices, triangles, uvs, texture, counts, device=None, want_uvs: bool = False):
    """Draws ``counts[f]`` surface samples of every triangle ``f`` (K22) -> ``(positions, colors)``
    [, ``sample_uvs``]: (N,3), (N,3) [, (N,2)] float32 tensors on the GPU, triangle by triangle in
    the order of ``triangles``.  numpy arrays or tensors; ``texture`` (H,W,C) uint8 with the row
    index growing with ``v``.  The prefix sum of the counts is taken here, on the host."""
    device = torch.device("cuda" if device is None else device)
    counts = np.asarray(counts)
    if counts.ndim != 1 or not np.issubdtype(counts.dtype, np.integer) or (counts < 0).any():
        raise ValueError("sample_mesh: counts must be a one-dimensional array of integers >= 0, "
                         "got %s %s" % (counts.dtype, counts.shape))
    offsets = np.zeros(len(counts) + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    if offsets[-1] > ops.octree_max_points():
        raise ValueError("sample_mesh: counts sums to %d samples; at most %d are supported"
                         % (offsets[-1], ops.octree_max_points()))

    def tensor(x, dtype):
        if torch.is_tensor(x):
            return x.to(device=device, dtype=getattr(torch, dtype)).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)

    if not torch.is_tensor(triangles):
        triangles = np.asarray(triangles)
        if (not np.issubdtype(triangles.dtype, np.integer) or triangles.size == 0
                or triangles.min() < 0 or triangles.max() > 2 ** 31 - 1):
            raise ValueError("sample_mesh: triangles must hold integers in 0 .. 2^31 - 1, got %s %s"
                             % (triangles.dtype, triangles.shape))
    return ops.mesh_sample(tensor(vertices, "float32"), tensor(triangles, "int32"),
                           tensor(uvs, "float32"), tensor(offsets, "int32"),
                           tensor(texture, "uint8"), want_uvs)


# ------------------------------------------------------------------------------------ meshes
def procedural_torus(rings: int = 64, sides: int = 32, texture_size: int = 256) -> Mesh:
    """A UV torus (axis +y, radii 1 and 0.4) of ``rings`` x ``sides`` quads, two triangles each,
    with a texture of a few low-frequency sinusoids in ``(u, v)``: large smooth colour regions and
    no seam (whole periods in both directions).  ``u`` runs round the ring, ``v`` round the tube;
    the seam vertices are doubled so that the UVs are continuous over every triangle."""
    rings, sides, size = int(rings), int(sides), int(texture_size)
    if rings < 3 or sides < 3 or size < 1:
        raise ValueError("procedural_torus: rings >= 3, sides >= 3, texture_size >= 1, got %d, "
                         "%d, %d" % (rings, sides, size))
    i, j = np.meshgrid(np.arange(rings + 1), np.arange(sides + 1), indexing="ij")
    u, v = i / rings, j / sides
    theta, phi = 2 * np.pi * u, 2 * np.pi * v
    tube = 1.0 + 0.4 * np.cos(phi)
    vertices = np.stack([tube * np.cos(theta), 0.4 * np.sin(phi), tube * np.sin(theta)], -1)
    uvs = np.stack([u, v], -1)
    corner = (i * (sides + 1) + j)[:-1, :-1].reshape(-1)
    right, up = corner + (sides + 1), corner + 1
    triangles = np.concatenate([np.stack([corner, right, right + 1], -1),
                                np.stack([corner, right + 1, up], -1)])
    centre = (np.arange(size) + 0.5) / size
    tv, tu = np.meshgrid(centre, centre, indexing="ij")       # row <-> v, column <-> u
    two_pi = 2 * np.pi
    red = 0.5 + 0.35 * np.sin(two_pi * tu) + 0.15 * np.sin(two_pi * 2 * tv)
    green = 0.5 + 0.35 * np.cos(two_pi * (tu + tv)) + 0.15 * np.sin(two_pi * 3 * tu)
    blue = 0.5 + 0.35 * np.sin(two_pi * tv + 1.0) + 0.15 * np.cos(two_pi * 2 * (tu - tv))
    texture = np.rint(255 * np.clip(np.stack([red, green, blue], -1), 0, 1)).astype(np.uint8)
    return (vertices.reshape(-1, 3).astype(np.float32), triangles.astype(np.int32),
            uvs.reshape(-1, 2).astype(np.float32), texture)


def _read_image(path: str) -> np.ndarray:
    from PIL import Image      # only a textured OBJ needs it
    with Image.open(path) as image:
        if image.mode not in ("RGB", "RGBA"):
            image = image.convert("RGB")
        return np.ascontiguousarray(np.asarray(image, dtype=np.uint8))


def _diffuse_map(mtl_path: str) -> Optional[str]:
    """The file of the first ``map_Kd`` statement of a material library (one material is read)."""
    if not os.path.exists(mtl_path):
        return None
    with open(mtl_path) as f:
        for line in f:
            words = line.split("#", 1)[0].split()
            if len(words) >= 2 and words[0] == "map_Kd":
                return os.path.join(os.path.dirname(mtl_path), words[-1])
    return None


def save_obj(path: str, vertices, triangles, colors=None, normals=None) -> None:
    """Writes a Wavefront OBJ: ``v x y z`` per vertex (``v x y z r g b`` with ``colors`` (V,3), the
    vertex-colour extension most viewers read), ``vn x y z`` per vertex with ``normals`` (V,3), and
    ``f a b c`` per triangle, 1-based, as ``a//a b//b c//c`` when normals are given.  Floats are
    written with ``%.9g``: a float32 survives the file bit for bit.  Needs no GPU."""
    vertices = np.asarray(vertices)
    if vertices.ndim != 2 or vertices.shape[1] != 3:
        raise ValueError("save_obj: vertices must be (V,3), got %s" % (vertices.shape,))
    triangles = np.asarray(triangles)
    if (triangles.ndim != 2 or triangles.shape[1] != 3
            or not np.issubdtype(triangles.dtype, np.integer)):
        raise ValueError("save_obj: triangles must be an integer (F,3) array, got %s %s"
                         % (triangles.dtype, triangles.shape))
    if len(triangles) and (triangles.min() < 0 or triangles.max() >= len(vertices)):
        raise ValueError("save_obj: triangles indexes vertices %d .. %d, outside 0 .. %d"
                         % (triangles.min(), triangles.max(), len(vertices) - 1))
    columns = [vertices]
    for name, extra in (("colors", colors), ("normals", normals)):
        if extra is not None and np.shape(extra) != vertices.shape:
            raise ValueError("save_obj: %s must be (V,3) = %s, got %s"
                             % (name, vertices.shape, np.shape(extra)))
    if colors is not None:
        columns.append(np.asarray(colors))
    rows = np.concatenate(columns, 1)
    lines = ["# %d vertices, %d triangles" % (len(vertices), len(triangles))]
    lines += ["v " + " ".join("%.9g" % x for x in row) for row in rows.tolist()]
    if normals is not None:
        lines += ["vn " + " ".join("%.9g" % x for x in row)
                  for row in np.asarray(normals).tolist()]
    corner = "%d//%d" if normals is not None else "%d"
    for a, b, c in (triangles.astype(np.int64) + 1).tolist():
        if normals is not None:
            lines.append("f " + " ".join(corner % (i, i) for i in (a, b, c)))
        else:
            lines.append("f %d %d %d" % (a, b, c))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")


def load_obj(path: str, texture_path: Optional[str] = None, return_colors: bool = False):
    """Reads the ``v``, ``vt`` and ``f`` records of a Wavefront OBJ -> ``(vertices, triangles, uvs,
    texture)``.  A face corner is ``v``, ``v/vt``, ``v/vt/vn`` or ``v//vn``, 1-based or negative
    (counted back from the records read so far); polygons become triangle fans; every distinct
    ``(v, vt)`` pair becomes one vertex, in the order the faces first use them.  The texture is
    ``texture_path`` or else the ``map_Kd`` of the ``mtllib`` (read with PIL, row 0 at the top).
    A file with no ``vt``, or with no texture, gives a 1x1 white texture and zero UVs.  Normals,
    groups and all but the first material are ignored, and so are vertex colours unless
    ``return_colors`` is set: then a fifth value follows, (V,3) float32 per-vertex colours when
    every ``v`` record reads ``v x y z r g b`` (what ``save_obj`` writes), ``None`` otherwise."""
    positions, coords, corners, library, tints = [], [], [], None, []

    def resolve(text, count, what, number):
        index = int(text)
        index = index - 1 if index > 0 else count + index
        if index < 0 or index >= count or int(text) == 0:
            raise ValueError("load_obj: %s line %d: %s index %s with %d read so far"
                             % (path, number, what, text, count))
        return index

    with open(path) as f:
        for number, line in enumerate(f, 1):
            words = line.split("#", 1)[0].split()
            if not words:
                continue
            if words[0] == "v":
                if len(words) < 4:
                    raise ValueError("load_obj: %s line %d: a vertex needs three coordinates"
                                     % (path, number))
                positions.append([float(w) for w in words[1:4]])
                if return_colors and len(words) >= 7:
                    tints.append([float(w) for w in words[4:7]])
            elif words[0] == "vt":
                values = [float(w) for w in words[1:3]]
                coords.append((values + [0.0, 0.0])[:2])
            elif words[0] == "f":
                if len(words) < 4:
                    raise ValueError("load_obj: %s line %d: a face needs three corners"
                                     % (path, number))
                face = []
                for word in words[1:]:
                    parts = word.split("/")
                    vertex = resolve(parts[0], len(positions), "vertex", number)
                    coord = -1
                    if len(parts) > 1 and parts[1]:
                        coord = resolve(parts[1], len(coords), "texture coordinate", number)
                    face.append((vertex, coord))
                for k in range(1, len(face) - 1):
                    corners.extend([face[0], face[k], face[k + 1]])
            elif words[0] == "mtllib" and library is None and len(words) > 1:
                library = os.path.join(os.path.dirname(os.path.abspath(path)), words[-1])
    if not corners:
        raise ValueError("load_obj: %s has no faces" % path)
    if texture_path is None and library is not None:
        texture_path = _diffuse_map(library)
    textured = texture_path is not None and any(coord >= 0 for _, coord in corners)
    if not textured:
        corners = [(vertex, -1) for vertex, _ in corners]
    pairs, index = {}, []
    for pair in corners:
        index.append(pairs.setdefault(pair, len(pairs)))
    order = np.array(list(pairs), dtype=np.int64).reshape(-1, 2)
    vertices = np.asarray(positions, dtype=np.float32)[order[:, 0]]
    uvs = np.zeros((len(order), 2), dtype=np.float32)
    if textured:
        has = order[:, 1] >= 0
        uvs[has] = np.asarray(coords, dtype=np.float32).reshape(-1, 2)[order[has, 1]]
        texture = _read_image(texture_path)
        if texture.ndim != 3 or texture.shape[2] < 3:
            raise ValueError("load_obj: texture %s is not an RGB image" % texture_path)
    else:
        texture = np.full((1, 1, 3), 255, dtype=np.uint8)
    triangles = np.asarray(index, dtype=np.int32).reshape(-1, 3)
    if not return_colors:
        return vertices, triangles, uvs, texture
    colors = None
    if tints and len(tints) == len(positions):
        colors = np.asarray(tints, dtype=np.float32)[order[:, 0]]
    return vertices, triangles, uvs, texture, colors


# ------------------------------------------------------------------------------------ K31
def supersample_projection(camera, supersample: int = 1) -> np.ndarray:
    """``cameras.projection_matrices([camera])[0]`` for an image of ``k`` times the width and
    height whose ``k x k`` blocks are centred on the camera's own pixels: ``S @ P`` with ``S``
    mapping ``u -> k u + (k - 1) / 2`` (and ``v`` likewise), formed in float64 and rounded once.
    -> (3,4) float32; ``k = 1`` is the plain matrix, bit for bit."""
    from .cameras import projection_matrices
    k = int(supersample)
    if k == 1:
        return projection_matrices([camera])[0]
    proj = np.eye(4, dtype=np.float64)
    proj[:3, :3] = np.asarray(camera.intrinsics, np.float64)
    proj = (proj @ np.linalg.inv(np.asarray(camera.extrinsics, np.float64)))[:3]
    grow = np.array([[k, 0.0, 0.5 * (k - 1)], [0.0, k, 0.5 * (k - 1)], [0.0, 0.0, 1.0]])
    return (grow @ proj).astype(np.float32)


def supersample_reduce(color: torch.Tensor, alpha: torch.Tensor, depth: torch.Tensor, width: int,
                       height: int, supersample: int):
    """``(k H) x (k W)`` rows of colour, alpha and depth -> ``H x W`` rows: the mean of every
    ``k x k`` block of colour and alpha, and the mean depth of the block's covered sub-pixels (0
    when none is).  Plain torch, on whatever device the tensors lie."""
    k = int(supersample)
    blocks = (height, k, width, k)
    color = color.reshape(blocks + (3,)).mean((1, 3)).reshape(-1, 3)
    hits = alpha.reshape(blocks).sum((1, 3))
    total = (depth * alpha).reshape(blocks).sum((1, 3))
    depth = torch.where(hits > 0, total / hits.clamp(min=1), torch.zeros_like(total))
    return color, (hits / float(k * k)).reshape(-1), depth.reshape(-1)


def rasterize_mesh(vertices: torch.Tensor, triangles: torch.Tensor, proj, eye, width: int,
                   height: int, colors=None, uvs=None, texture=None, background=(0, 0, 0),
                   batch_size: int = 1 << 22):
    """K31 from set-up to resolve on GPU tensors: ``proj`` (3,4) and ``eye`` (3,) on the host,
    ``texture`` with the row index growing with ``v`` -> ``(color, alpha, depth, ids, status,
    box_pixels)``; ``status`` (F,) uint8 indexes ``ops.MESH_RASTER_STATUS``.  One read-back (the
    number of box pixels); the box pixels are drawn ``batch_size`` at a time, and the image does
    not depend on that size."""
    width, height, batch_size = int(width), int(height), int(batch_size)
    if not 1 <= batch_size <= ops.octree_max_points():
        raise ValueError("rasterize_mesh: batch_size must lie in 1 .. %d, got %d"
                         % (ops.octree_max_points(), batch_size))
    record, status, counts = ops.mesh_raster_setup(vertices, triangles, proj, width, height)
    offsets, total = ops.mesh_raster_offsets(counts)
    zbuf = torch.full((width * height,), ops.MESH_RASTER_EMPTY, dtype=torch.int64,
                      device=vertices.device)
    for first in range(0, total, batch_size):
        ops.mesh_raster_draw(record, offsets, first, min(batch_size, total - first), width, height,
                             zbuf)
    return ops.mesh_raster_resolve(zbuf, record, vertices, triangles, colors, uvs, texture, eye,
                                   background, width, height) + (status, total)


_warned_clipped = False


def _render_mesh_check(who, vertices, triangles, camera, colors, uvs, texture, background,
                       supersample, batch_size):
    """The refusals of ``render_mesh`` and ``render_mesh_image``; none needs a device."""
    shape = tuple(vertices.shape) if hasattr(vertices, "shape") else np.shape(vertices)
    if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
        raise ValueError("%s: vertices must be (V,3) with V >= 1, got %s" % (who, shape))
    ids = triangles.cpu().numpy() if torch.is_tensor(triangles) else triangles
    _check_triangles(who, ids, shape[0])
    if not hasattr(camera, "intrinsics") or not hasattr(camera, "extrinsics") \
            or not hasattr(camera, "resolution"):
        raise ValueError("%s: camera must be a CameraInfo, got %s" % (who, type(camera).__name__))
    if colors is not None and (uvs is not None or texture is not None):
        raise ValueError("%s: give either colors, or uvs and texture, not both" % who)
    if colors is None and (uvs is None or texture is None):
        raise ValueError("%s: give colors, or both uvs and texture" % who)
    for name, value, last in (("colors", colors, 3), ("uvs", uvs, 2)):
        if value is not None and tuple(value.shape if hasattr(value, "shape")
                                       else np.shape(value)) != (shape[0], last):
            raise ValueError("%s: %s must be (V,%d) = (%d,%d), got %s"
                             % (who, name, last, shape[0], last, tuple(np.shape(value))))
    if texture is not None:
        tex = tuple(texture.shape) if hasattr(texture, "shape") else np.shape(texture)
        if len(tex) != 3 or tex[2] < 3 or min(tex) < 1:
            raise ValueError("%s: texture must be (H,W,C) with C >= 3, got %s" % (who, tex))
    ground = np.asarray(background, dtype=np.float64).reshape(-1)
    if ground.shape != (3,) or not np.isfinite(ground).all():
        raise ValueError("%s: background must be three finite numbers, got %r"
                         % (who, background))
    k = int(supersample)
    width, height = int(camera.resolution.width), int(camera.resolution.height)
    if k != supersample or k < 1:
        raise ValueError("%s: supersample must be an integer >= 1, got %r" % (who, supersample))
    if not 1 <= k * width <= ops.MESH_RASTER_MAX_SIDE \
            or not 1 <= k * height <= ops.MESH_RASTER_MAX_SIDE:
        raise ValueError("%s: supersample times the camera's resolution must lie in 1 .. %d a "
                         "side, got %d x (%d x %d)"
                         % (who, ops.MESH_RASTER_MAX_SIDE, k, width, height))
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("%s: batch_size must be an integer >= 1, got %r" % (who, batch_size))
    return k, width, height


def render_mesh(vertices, triangles, camera, colors=None, uvs=None, texture=None,
                background=(0, 0, 0), supersample: int = 1, batch_size: int = 1 << 22,
                device=None, return_ids: bool = False):
    """Draws a triangle mesh as ``camera`` (a ``CameraInfo``) sees it, with a z-buffer (K31,
    ``csrc/mesh_raster.hip``) -> ``(RenderResult, report)``: ``color`` (H W,3), ``alpha`` (H W,) 1
    where a triangle covers the pixel's centre and 0 elsewhere, ``depth`` (H W,) the distance of
    the surface from the camera (the ``t`` of ``OcTree.render``; 0 where nothing is), rows in
    pixel order ``py W + px``.  numpy in gives numpy out; tensors stay tensors.  With
    ``return_ids`` -> ``(RenderResult, ids, report)``, ``ids`` (H W,) int32 the triangle drawn in
    every pixel, -1 for none.

    vertices (V,3), triangles (F,3) integers.  Exactly one of ``colors`` (V,3), interpolated
    perspective-correctly, and ``uvs`` (V,2) + ``texture`` (h,w,C) uint8 with row 0 at the top (as
    ``load_obj`` and ``procedural_torus`` return it; it is flipped as
    ``OcTree.build_from_triangles`` flips it for K22, whose bilinear lookup is used).  Both sides
    of a triangle are drawn; a pixel centre exactly on an edge is covered.

    ``report``: how many triangles were ``drawn``, ``behind`` the camera, ``clipped``,
    ``degenerate`` after snapping to 1/256 pixel or ``off_image``, and ``box_pixels``.  There is
    NO near-plane clipping: a triangle with a vertex at or behind the camera plane, or one
    projected beyond 16384 pixels from the origin, is ``clipped`` -- not drawn -- and a warning
    says so once.

    ``supersample=k`` draws ``k W x k H`` sub-pixels, ``k x k`` centred on every pixel, and
    averages colour and alpha over them; the depth is the mean over the covered sub-pixels.
    ``k = 1`` is the plain image.  ``batch_size``: box pixels per launch; the image does not
    depend on it."""
    global _warned_clipped
    who = "render_mesh"
    k, width, height = _render_mesh_check(who, vertices, triangles, camera, colors, uvs, texture,
                                          background, supersample, batch_size)
    if return_ids and k != 1:
        raise ValueError("%s: return_ids needs supersample = 1, got %d" % (who, k))
    from .cameras import eye_positions
    from .utils import RenderResult
    as_numpy = not torch.is_tensor(vertices)
    if device is None:
        device = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else "cuda"
    device = torch.device(device)

    def tensor(x, dtype):
        if x is None:
            return None
        if torch.is_tensor(x):
            return x.to(device=device, dtype=getattr(torch, dtype)).contiguous()
        return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)

    if texture is not None:
        texture = texture.flip(0) if torch.is_tensor(texture) else np.asarray(texture)[::-1]
    color, alpha, depth, ids, status, total = rasterize_mesh(
        tensor(vertices, "float32"), tensor(triangles, "int32"),
        supersample_projection(camera, k), eye_positions([camera], (0.0, 0.0, 0.0))[0],
        k * width, k * height, tensor(colors, "float32"), tensor(uvs, "float32"),
        tensor(texture, "uint8"), background, batch_size)
    if k > 1:
        color, alpha, depth = supersample_reduce(color, alpha, depth, width, height, k)
    tally = torch.bincount(status.to(torch.int64), minlength=len(ops.MESH_RASTER_STATUS))
    report = dict(zip(ops.MESH_RASTER_STATUS, [int(v) for v in tally.cpu().tolist()]))
    report["box_pixels"] = total
    if report["clipped"] > 0 and not _warned_clipped:
        _warned_clipped = True
        import warnings
        warnings.warn("render_mesh: %d of %d triangles reach the camera plane or leave the guard "
                      "band and are not drawn (there is no near-plane clipping)"
                      % (report["clipped"], len(status)))
    out = RenderResult(color, alpha, depth)
    if as_numpy:
        out, ids = out.numpy(), ids.cpu().numpy()
    return (out, ids, report) if return_ids else (out, report)


def render_mesh_image(vertices, triangles, camera, colors=None, uvs=None, texture=None,
                      background=(0, 0, 0), supersample: int = 1, batch_size: int = 1 << 22,
                      device=None, include_depth: bool = False):
    """``render_mesh`` as a frame -> (H,W,3) uint8 numpy (K8's bytes: ``color * 255`` truncated),
    and with ``include_depth`` also the (H,W) float32 alpha and depth maps: the return shape of
    ``OcTree.render_image``."""
    _render_mesh_check("render_mesh_image", vertices, triangles, camera, colors, uvs, texture,
                       background, supersample, batch_size)

    def on_device(x):
        if x is None or torch.is_tensor(x):
            return x
        return torch.from_numpy(np.ascontiguousarray(x))

    out, _ = render_mesh(on_device(np.asarray(vertices, dtype=np.float32)
                                   if not torch.is_tensor(vertices) else vertices),
                         on_device(triangles), camera, on_device(colors), on_device(uvs),
                         on_device(texture), background, supersample, batch_size, device)
    width, height = int(camera.resolution.width), int(camera.resolution.height)
    pixels = torch.arange(width * height, dtype=torch.int64, device=out.color.device)
    image = ops.to_image(out.color.contiguous(), pixels, width, height).cpu().numpy()
    if not include_depth:
        return image
    return (image, out.alpha.reshape(height, width).cpu().numpy(),
            out.depth.reshape(height, width).cpu().numpy())
