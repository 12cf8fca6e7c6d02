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

``render_mesh_backward`` is the transpose of that picture in the per-vertex colours (K32,
``csrc/mesh_raster_grad.hip``); ``color_mesh_from_images`` uses it to give every vertex the mean
colour of the pixels that see it, ``fit_mesh_colors`` to optimise the colours against a dataset's
images, and ``vertex_adjacency`` makes the corner lists both need.  No counterpart either.

``mesh_texture_taps`` writes the textured picture of one camera as a sparse matrix in the texture
(K33, ``csrc/mesh_texture.hip``); ``render_mesh_texture`` and ``render_mesh_texture_backward``
are its two products, ``texture_mesh_from_images`` and ``fit_mesh_texture`` what
``color_mesh_from_images`` and ``fit_mesh_colors`` are for vertices.  ``unwrap_mesh`` makes a
texture atlas for a mesh that has no UVs, ``bake_vertex_colors`` fills it from per-vertex colours,
and ``texture_to_uint8`` + ``save_obj(uvs=, texture=)`` write the result out.

``render_mesh(..., antialias=True)`` blends the silhouette edges analytically (K34,
``csrc/mesh_aa.hip``, nvdiffrast's edge antialiasing), which makes the picture a smooth function of
the vertex positions; ``render_mesh_geometry_backward`` is its transpose in the positions,
``fit_mesh_geometry`` optimises them against a dataset's images, and ``edge_opposites`` and
``vertex_neighbors`` make the edge and neighbour lists they need.  With ``interior=True`` both add
the other half of the geometry gradient, colour through the barycentric weights (K35,
``csrc/mesh_interp_grad.hip``): it moves the vertices that lie on no outline.
"""

import math
import os
from typing import NamedTuple, Optional, Tuple

import numpy as np
import torch

from . import fit_loop, ops

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


def save_obj(path: str, vertices, triangles, colors=None, normals=None, uvs=None,
             texture=None) -> None:
    """Writes a Wavefront OBJ: ``v x y z`` per vertex (``v x y z r g b`` with ``colors`` (V,3), the
    vertex-colour extension most viewers read), ``vn x y z`` per vertex with ``normals`` (V,3), and
    ``f a b c`` per triangle, 1-based, as ``a//a b//b c//c`` when normals are given.  Floats are
    written with ``%.9g``: a float32 survives the file bit for bit.  Needs no GPU.

    With ``uvs`` (V,2) and ``texture`` (H,W,3 or 4) uint8 with row 0 at the top (what ``load_obj``
    returns and ``texture_to_uint8`` makes) -- both or neither -- it also writes ``vt u v`` per
    vertex, the faces as ``a/a b/b c/c`` (``a/a/a`` with normals), the texture as a PNG and a
    material library with its ``map_Kd`` beside the OBJ (``name.png``, ``name.mtl`` for
    ``name.obj``): ``load_obj`` reads the same arrays back when the triangles use the vertices in
    the order of their numbers, as those of ``unwrap_mesh`` do.  Without them the file is byte for
    byte what it was."""
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
    if (uvs is None) != (texture is None):
        raise ValueError("save_obj: give both uvs and texture, or neither")
    if uvs is not None:
        if np.shape(uvs) != (len(vertices), 2):
            raise ValueError("save_obj: uvs must be (V,2) = (%d,2), got %s"
                             % (len(vertices), np.shape(uvs)))
        texture = np.asarray(texture)
        if texture.ndim != 3 or texture.shape[2] not in (3, 4) or texture.dtype != np.uint8 \
                or min(texture.shape) < 1:
            raise ValueError("save_obj: texture must be (H,W,3) or (H,W,4) uint8 with row 0 at the "
                             "top (texture_to_uint8 makes one), got %s %s"
                             % (texture.dtype, texture.shape))
    if colors is not None:
        columns.append(np.asarray(colors))
    rows = np.concatenate(columns, 1)
    lines = ["# %d vertices, %d triangles" % (len(vertices), len(triangles))]
    stem = os.path.splitext(os.path.basename(path))[0]
    if uvs is not None:
        lines.append("mtllib %s.mtl" % stem)
    lines += ["v " + " ".join("%.9g" % x for x in row) for row in rows.tolist()]
    if uvs is not None:
        lines += ["vt " + " ".join("%.9g" % x for x in row) for row in np.asarray(uvs).tolist()]
    if normals is not None:
        lines += ["vn " + " ".join("%.9g" % x for x in row)
                  for row in np.asarray(normals).tolist()]
    if uvs is not None:
        lines.append("usemtl atlas")
        corner = "%d/%d/%d" if normals is not None else "%d/%d"
        copies = 3 if normals is not None else 2
        for face in (triangles.astype(np.int64) + 1).tolist():
            lines.append("f " + " ".join(corner % ((i,) * copies) for i in face))
    else:
        corner = "%d//%d" if normals is not None else "%d"
        for a, b, c in (triangles.astype(np.int64) + 1).tolist():
            if normals is not None:
                lines.append("f " + " ".join(corner % (i, i) for i in (a, b, c)))
            else:
                lines.append("f %d %d %d" % (a, b, c))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
    if uvs is not None:
        from PIL import Image      # only a textured OBJ needs it
        folder = os.path.dirname(os.path.abspath(path))
        Image.fromarray(texture).save(os.path.join(folder, stem + ".png"))
        with open(os.path.join(folder, stem + ".mtl"), "w") as f:
            f.write("newmtl atlas\nKa 1 1 1\nKd 1 1 1\nKs 0 0 0\nmap_Kd %s.png\n" % stem)


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
    return _rasterize(vertices, triangles, proj, eye, width, height, colors, uvs, texture,
                      background, batch_size)[1:]


def _rasterize(vertices, triangles, proj, eye, width, height, colors=None, uvs=None, texture=None,
               background=(0, 0, 0), batch_size=1 << 22):
    """``rasterize_mesh`` with K31a's ``record`` in front of its results (K32a reads it)."""
    return _rasterize_z(vertices, triangles, proj, eye, width, height, colors, uvs, texture,
                        background, batch_size)[:-1]


def _rasterize_z(vertices, triangles, proj, eye, width, height, colors=None, uvs=None,
                 texture=None, background=(0, 0, 0), batch_size=1 << 22):
    """``_rasterize`` with K31b's ``zbuf`` behind its results (K34 reads it)."""
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
    return (record,) + ops.mesh_raster_resolve(zbuf, record, vertices, triangles, colors, uvs,
                                               texture, eye, background, width, height) \
        + (status, total, zbuf)


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
                device=None, return_ids: bool = False, antialias: bool = False):
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
    depend on it.

    ``antialias=True`` puts colour and alpha through K34a (``csrc/mesh_aa.hip``, nvdiffrast's
    analytic edge antialiasing): two neighbouring pixels that a silhouette edge separates are
    blended by how far the edge reaches between their centres, so alpha takes values between 0
    and 1 along the outline, on the vertex-colour and the textured path alike; ``depth`` and
    ``ids`` stay K31's.  With ``supersample > 1`` the pass runs on the sub-pixel image, before the
    reduction.  With False, the default, nothing of K34 is called and the bits are K31's.  The
    limits: only silhouette, fold, boundary and non-manifold edges are blended (an edge between
    two triangles that continue the surface is not); a silhouette that falls between two pixel
    centres of the same id is not seen."""
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
    frame = (tensor(vertices, "float32"), tensor(triangles, "int32"),
             supersample_projection(camera, k), eye_positions([camera], (0.0, 0.0, 0.0))[0],
             k * width, k * height, tensor(colors, "float32"), tensor(uvs, "float32"),
             tensor(texture, "uint8"), background, batch_size)
    if antialias:
        record, color, alpha, depth, ids, status, total, zbuf = _rasterize_z(*frame)
        color, alpha = ops.mesh_aa_forward(
            record, zbuf, ids, edge_opposites(frame[1], frame[0].shape[0], device), frame[0],
            frame[2], color, alpha, k * width, k * height)
    else:
        color, alpha, depth, ids, status, total = rasterize_mesh(*frame)
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
                      device=None, include_depth: bool = False, antialias: bool = False):
    """``render_mesh`` as a frame -> (H,W,3) uint8 numpy (K8's bytes: ``color * 255`` truncated),
    and with ``include_depth`` also the (H,W) float32 alpha and depth maps: the return shape of
    ``OcTree.render_image``.  ``antialias`` is ``render_mesh``'s."""
    _render_mesh_check("render_mesh_image", vertices, triangles, camera, colors, uvs, texture,
                       background, supersample, batch_size)

    def on_device(x):
        if x is None or torch.is_tensor(x):
            return x
        return torch.from_numpy(np.ascontiguousarray(x))

    out, _ = render_mesh(on_device(np.asarray(vertices, dtype=np.float32)
                                   if not torch.is_tensor(vertices) else vertices),
                         on_device(triangles), camera, on_device(colors), on_device(uvs),
                         on_device(texture), background, supersample, batch_size, device,
                         antialias=bool(antialias))
    width, height = int(camera.resolution.width), int(camera.resolution.height)
    pixels = torch.arange(width * height, dtype=torch.int64, device=out.color.device)
    image = ops.to_image(out.color.contiguous(), pixels, width, height).cpu().numpy()
    if not include_depth:
        return image
    return (image, out.alpha.reshape(height, width).cpu().numpy(),
            out.depth.reshape(height, width).cpu().numpy())


# ------------------------------------------------------------------------------------ K32
# ops.clip_adam's defaults, as fit_octree has them
CLIP_VALUE = 0.1
MAX_NORM = 0.1
_MOST = (2 ** 31 - 1) // 3


def _shape_of(x):
    return tuple(x.shape) if hasattr(x, "shape") else np.shape(x)


def _on(x, dtype, device):
    if torch.is_tensor(x):
        return x.to(device=device, dtype=getattr(torch, dtype)).contiguous()
    return torch.from_numpy(np.ascontiguousarray(x, dtype=dtype)).to(device)


def _mesh_on(vertices, triangles, device=None):
    """numpy in, numpy out -> (whether ``vertices`` came as numpy, the device, ``vertices`` float32
    and ``triangles`` int32 as tensors on it).  ``device`` defaults to that of ``vertices`` when
    they are a GPU tensor, else the GPU."""
    if device is None:
        device = vertices.device if torch.is_tensor(vertices) and vertices.is_cuda else "cuda"
    device = torch.device(device)
    return (not torch.is_tensor(vertices), device, _on(vertices, "float32", device),
            _on(triangles, "int32", device))


def vertex_adjacency(triangles, num_vertices: int, device=None):
    """Which corners use every vertex -> ``(corner_order (3F,) int32, vertex_starts (V+1,) int32)``
    tensors on ``device`` (default: the tensor's own, or the GPU for a numpy array):
    ``corner_order`` holds the flat corner indices ``3 f + i`` stably sorted by vertex id -- the
    corners of one vertex in the order of the faces -- and ``vertex_starts`` the CSR rows, so that
    vertex ``v`` owns ``corner_order[vertex_starts[v] : vertex_starts[v + 1]]``.  The ids are
    clamped into ``0 .. V - 1`` as K31 clamps them.  A torch stable sort and a bincount: integer
    plumbing, as the key sort of ``OcTree.extract_mesh``; it depends on the triangles alone and
    can be made once for many calls of ``render_mesh_backward``."""
    who = "vertex_adjacency"
    shape = _shape_of(triangles)
    if torch.is_tensor(triangles):
        integer = not (triangles.dtype.is_floating_point or triangles.dtype.is_complex
                       or triangles.dtype == torch.bool)
    else:
        integer = np.issubdtype(np.asarray(triangles).dtype, np.integer)
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= _MOST or not integer:
        raise ValueError("%s: triangles must be an integer (F,3) array with 1 <= F <= "
                         "(2^31 - 1) / 3, got %s" % (who, shape))
    if int(num_vertices) != num_vertices or not 1 <= int(num_vertices) <= _MOST:
        raise ValueError("%s: num_vertices must be an integer in 1 .. (2^31 - 1) / 3, got %r"
                         % (who, num_vertices))
    num_vertices = int(num_vertices)
    if device is None:
        device = triangles.device if torch.is_tensor(triangles) else "cuda"
    flat = _on(triangles, "int64", torch.device(device)).reshape(-1).clamp(0, num_vertices - 1)
    order = torch.sort(flat, stable=True)[1].to(torch.int32).contiguous()
    starts = torch.zeros((num_vertices + 1,), dtype=torch.int64, device=flat.device)
    torch.cumsum(torch.bincount(flat, minlength=num_vertices), 0, out=starts[1:])
    return order, starts.to(torch.int32)


def _mesh_colors_check(who, vertices, colors=None, uvs=None, texture=None,
                       supersample=1, batch_size=1):
    """What every K32 function refuses of its mesh from shapes and types alone -> V.  The vertex
    ids themselves are looked at last (``_mesh_ids_check``): for a tensor on the GPU that is a
    read-back, and every refusal that needs none comes before it."""
    shape = _shape_of(vertices)
    if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
        raise ValueError("%s: vertices must be (V,3) with V >= 1, got %s" % (who, shape))
    if uvs is not None or texture is not None:
        raise ValueError("%s: uvs and texture are not supported here, only per-vertex colors: the "
                         "textured path's transpose is render_mesh_texture_backward" % who)
    if colors is not None:
        if _shape_of(colors) != (shape[0], 3):
            raise ValueError("%s: colors must be (V,3) = (%d,3), got %s"
                             % (who, shape[0], _shape_of(colors)))
        kind = colors.dtype
        floating = kind.is_floating_point if torch.is_tensor(colors) \
            else np.issubdtype(np.asarray(colors).dtype, np.floating)
        if not floating:
            raise ValueError("%s: colors must be floating point, got %s" % (who, kind))
    if supersample != 1:
        raise ValueError("%s: supersample must be 1 (the backward of the k x k mean is not "
                         "built), got %r" % (who, supersample))
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("%s: batch_size must be an integer >= 1, got %r" % (who, batch_size))
    return shape[0]


def _mesh_ids_check(who, triangles, num_vertices):
    """The shape, type and range of the vertex ids, as ``render_mesh`` checks them: the last of a
    function's refusals."""
    _check_triangles(who, triangles.cpu().numpy() if torch.is_tensor(triangles) else triangles,
                     num_vertices)


def _camera_size(who, camera):
    if not hasattr(camera, "intrinsics") or not hasattr(camera, "extrinsics") \
            or not hasattr(camera, "resolution"):
        raise ValueError("%s: camera must be a CameraInfo, got %s" % (who, type(camera).__name__))
    width, height = int(camera.resolution.width), int(camera.resolution.height)
    if not 1 <= width <= ops.MESH_RASTER_MAX_SIDE or not 1 <= height <= ops.MESH_RASTER_MAX_SIDE:
        raise ValueError("%s: the camera's resolution must lie in 1 .. %d a side, got %d x %d"
                         % (who, ops.MESH_RASTER_MAX_SIDE, width, height))
    return width, height


def _alpha_byte(who, alpha_threshold):
    """K24's threshold byte: ``ceil(alpha_threshold * 255)`` clamped into 1 .. 255."""
    alpha_threshold = float(alpha_threshold)
    if not 0.0 <= alpha_threshold <= 1.0:        # NaN fails too
        raise ValueError("%s: alpha_threshold must lie in [0, 1], got %r" % (who, alpha_threshold))
    return min(max(int(np.ceil(alpha_threshold * 255)), 1), 255)


def _mesh_dataset_check(who, name, dataset):
    """``dataset.images`` (C,H,W,3 or 4) uint8 and ``dataset.cameras`` of that one resolution, RGB
    -> (images, cameras, width, height).  No device."""
    images = np.asarray(getattr(dataset, "images", None))
    if images.ndim != 4 or images.shape[-1] not in (3, 4) or images.dtype != np.uint8:
        raise ValueError("%s: %s.images must be (C,H,W,3) or (C,H,W,4) uint8, got %s %s"
                         % (who, name, images.dtype, images.shape))
    if getattr(dataset, "color_space", "RGB") != "RGB":
        raise ValueError("%s: %s.color_space must be RGB, got %r"
                         % (who, name, dataset.color_space))
    cameras = list(dataset.cameras)
    if len(cameras) != len(images) or not cameras:
        raise ValueError("%s: %s has %d cameras for %d images"
                         % (who, name, len(cameras), len(images)))
    height, width = images.shape[1:3]
    for camera in cameras:
        if _camera_size(who, camera) != (width, height):
            raise ValueError("%s: a camera of %s is %d x %d, its image %d x %d"
                             % ((who, name) + _camera_size(who, camera) + (width, height)))
    return images, cameras, width, height


def _raster_ids(vertices, triangles, proj, width, height, batch_size):
    """K31a-c for the ids alone -> (record, ids).  The resolve needs some colours and an eye: the
    vertices and the origin serve, the image they make is dropped."""
    out = _rasterize(vertices, triangles, proj, (0.0, 0.0, 0.0), width, height, vertices,
                     batch_size=batch_size)
    return out[0], out[4]


def render_mesh_backward(vertices, triangles, camera, d_color, adjacency=None, grad=None,
                         weight=None, accumulate: bool = False, batch_size: int = 1 << 22,
                         supersample: int = 1, uvs=None, texture=None):
    """The transpose of ``render_mesh``'s colours in the per-vertex ``colors`` (K32,
    ``csrc/mesh_raster_grad.hip``) -> ``(grad (V,3), weight (V,))`` float32: with ``d_color``
    (H W,3) the gradient of a loss in the image's colours, ``grad`` is its gradient in the vertex
    colours, ``grad[v] = sum b_i d_color[p]`` over the pixels ``p`` won by a triangle with ``v``
    as its corner ``i``, and ``weight[v] = sum b_i`` over the same pixels; ``b_i`` are K31's
    perspective-correct barycentric weights, the bits the forward used.  It runs K31a-c for the
    camera (the ids of the z-buffer decide which triangle owns a pixel: occlusion is the mesh's
    own), then K32a and K32b: fixed orders, no float atomics, the same bits on every call and for
    every ``batch_size``.  The background has no gradient here; positions get none.

    numpy in gives numpy out; tensors stay tensors.  ``adjacency``: what ``vertex_adjacency``
    returns for these triangles (made here when None).  ``grad`` and ``weight`` (GPU tensors) are
    written in place when given, and added to with ``accumulate``.  ``supersample`` must be 1 and
    ``uvs`` / ``texture`` None: the mean over sub-pixels and the textured path have no
    backward."""
    who = "render_mesh_backward"
    num_vertices = _mesh_colors_check(who, vertices, None, uvs, texture, supersample,
                                      batch_size)
    width, height = _camera_size(who, camera)
    if _shape_of(d_color) != (width * height, 3):
        raise ValueError("%s: d_color must be (H W,3) = (%d,3), got %s"
                         % (who, width * height, _shape_of(d_color)))
    if (grad is None) != (weight is None) or (accumulate and grad is None):
        raise ValueError("%s: give both grad and weight, or neither; accumulate needs them" % who)
    _mesh_ids_check(who, triangles, num_vertices)
    as_numpy, device, vertices, triangles = _mesh_on(vertices, triangles)
    if adjacency is None:
        adjacency = vertex_adjacency(triangles, num_vertices, device)
    record, ids = _raster_ids(vertices, triangles, supersample_projection(camera, 1), width,
                              height, batch_size)
    face_sums = ops.mesh_raster_face_sums(record, ids, _on(d_color, "float32", device), width,
                                          height)
    grad, weight = ops.mesh_vertex_gather(face_sums, adjacency[0], adjacency[1], grad, weight,
                                          accumulate)
    if as_numpy:
        return grad.cpu().numpy(), weight.cpu().numpy()
    return grad, weight


def color_mesh_from_images(vertices, triangles, dataset, colors=None,
                           alpha_threshold: float = 0.5):
    """Gives every vertex the mean colour of the pixels that see it -> ``(colors (V,3), weights
    (V,))`` float32 (numpy in gives numpy out; tensors stay tensors).  Over the cameras of
    ``dataset`` (an ``ImageDataset``: ``images`` (C,H,W,4) uint8 and ``cameras``) in order, K32
    accumulates ``sum b_i rgb[p] / 255`` and ``sum b_i`` per vertex; a pixel whose own alpha byte
    is below ``ceil(alpha_threshold * 255)`` (clamped into 1 .. 255, as
    ``OcTree.color_from_images`` clamps it) is left out of both sums.  A vertex with
    ``weight > 0`` gets ``sum / weight``, one f32 division per channel; any other keeps
    ``colors[v]``, or 0.5 grey when ``colors`` is None.  What K24 does for the leaves of a tree.

    The limits: the weights are the perspective-correct barycentric weights of the pixels, not
    areas, so a camera that sees a triangle large counts for more; a vertex seen only at grazing
    angles still counts, with whatever those few pixels hold; visibility is the mesh's own
    z-buffer, so a hole in the mesh lets the far side be coloured from the front."""
    who = "color_mesh_from_images"
    num_vertices = _mesh_colors_check(who, vertices, colors)
    alpha_u8 = _alpha_byte(who, alpha_threshold)
    images, cameras, width, height = _mesh_dataset_check(who, "dataset", dataset)
    _mesh_ids_check(who, triangles, num_vertices)
    as_numpy, device, vertices, triangles = _mesh_on(vertices, triangles)
    order, starts = vertex_adjacency(triangles, num_vertices, device)

    def splat(camera, hidden, rgb, total, weights, accumulate):
        record, ids = _raster_ids(vertices, triangles, supersample_projection(camera, 1), width,
                                  height, 1 << 22)
        if hidden is not None:
            ids = ids.masked_fill(hidden, -1)
        face_sums = ops.mesh_raster_face_sums(record, ids, rgb, width, height)
        ops.mesh_vertex_gather(face_sums, order, starts, total, weights, accumulate)

    return _mean_from_images(images, cameras, alpha_u8, colors, num_vertices, splat, device,
                             as_numpy)


def _mean_from_images(images, cameras, alpha_u8, given, count, splat, device, as_numpy):
    """What ``color_mesh_from_images`` and ``texture_mesh_from_images`` share -> ``(colors
    (count,3), weights (count,))``.  Over the cameras in order, ``splat(camera, hidden, rgb, total,
    weights, accumulate)`` adds the camera's weighted colours and weights to the two buffers:
    ``hidden`` (H W,) bool marks the pixels whose alpha byte is below ``alpha_u8`` (None for images
    without alpha).  A row nobody saw keeps ``given``'s, or 0.5 grey when ``given`` is None."""
    total = torch.zeros((count, 3), dtype=torch.float32, device=device)
    weights = torch.zeros((count,), dtype=torch.float32, device=device)
    for number, camera in enumerate(cameras):
        frame = images[number]
        hidden = None
        if frame.shape[-1] == 4:
            hidden = torch.from_numpy(frame[..., 3].reshape(-1) < alpha_u8).to(device)
        rgb = (frame[..., :3].astype(np.float32) / 255).reshape(-1, 3)      # as ImageDataset
        splat(camera, hidden, torch.from_numpy(rgb).to(device), total, weights, number > 0)
    out = np.full((count, 3), 0.5, dtype=np.float32) if given is None else \
        np.array(given.detach().cpu().numpy() if torch.is_tensor(given) else given,
                 dtype=np.float32).reshape(-1, 3)
    # (the division on the host: one IEEE f32 division per channel, whatever the device's is)
    sums, weights_host = total.cpu().numpy(), weights.cpu().numpy()
    seen = weights_host > 0
    out[seen] = sums[seen] / weights_host[seen][:, None]
    if as_numpy:
        return out, weights_host
    return torch.from_numpy(out).to(device), weights


def _fit_mesh(who, num_vertices, vertices, triangles, start, setup, train_dataset, val_dataset,
              num_steps, learning_rate, cameras_per_step, report_interval, alpha_threshold,
              clip_value, max_norm, seed, verbose):
    """What ``fit_mesh_colors`` and ``fit_mesh_texture`` do alike, after the refusals of their own
    buffer ``start``: the other refusals (the vertex ids last; none touches the device), then
    ``fit_loop.run`` on a copy of ``start`` as an (n,3) buffer on the dataset's device ->
    ``(data, log)``, with the step their docstrings describe.  ``setup(vertices, triangles, data,
    view, val_view)`` gets the mesh on the device and ``(cameras, width, height)`` of the two
    datasets (``val_view`` None without one) and returns ``(frame, val_frame, transpose)``:
    ``frame(camera) -> (color, alpha, ctx)`` and ``transpose(ctx, d_color, grads, weight,
    accumulate)``, which accumulates from a step's second camera on."""
    fit_loop.check_schedule(who, "num_steps >= 0, cameras_per_step >= 1, report_interval >= 1",
                            cameras_per_step, num_steps, report_interval, learning_rate)
    cameras_per_step = int(cameras_per_step)
    alpha_u8 = None if alpha_threshold is None else _alpha_byte(who, alpha_threshold)
    images, *view = _mesh_dataset_check(who, "train_dataset", train_dataset)
    if alpha_u8 is not None and images.shape[-1] != 4:
        raise ValueError("%s: alpha_threshold needs train_dataset.images with an alpha channel, "
                         "got %s" % (who, images.shape))
    val_view = None if val_dataset is None else \
        _mesh_dataset_check(who, "val_dataset", val_dataset)[1:]
    _mesh_ids_check(who, triangles, num_vertices)
    _, device, vertices, triangles = _mesh_on(vertices, triangles, train_dataset.colors.device)
    data = _on(start, "float32", device).reshape(-1, 3).clone()
    frame, val_frame, transpose = setup(vertices, triangles, data, view, val_view)
    cameras, width, height = view
    per = width * height
    weight = torch.empty((data.shape[0],), dtype=torch.float32, device=device)
    pixels = torch.arange(per, dtype=torch.int64, device=device)
    alphas = train_dataset._gt_alphas()
    kept = {}
    generator = torch.Generator()
    generator.manual_seed(int(seed))

    def epoch():
        deal = torch.randperm(len(cameras), generator=generator).tolist()
        return [deal[first:first + cameras_per_step]
                for first in range(0, len(deal), cameras_per_step)]

    def step(chosen, grads):
        count = len(chosen) * per
        total = None
        for number, camera in enumerate(chosen):
            color, alpha, ctx = frame(camera)
            sums, d_color, _ = ops.mse_loss(color, alpha, train_dataset.colors, alphas,
                                            pixels + camera * per, 1.0 / (3 * count), 0.0)
            if alpha_u8 is not None:
                if camera not in kept:
                    kept[camera] = torch.from_numpy(
                        images[camera][..., 3].reshape(-1, 1) >= alpha_u8).to(device)
                d_color = torch.where(kept[camera], d_color, torch.zeros_like(d_color))
            transpose(ctx, d_color, grads, weight, number > 0)
            total = sums if total is None else total + sums
        return ops.loss_value(total, count, 0.0)

    def validate():
        return fit_loop.camera_psnr(val_frame, len(val_view[0]), val_view[1] * val_view[2],
                                    val_dataset)

    log = fit_loop.run(data, epoch, step, lambda rows: rows.clamp_(0, 1),
                       validate if val_dataset is not None else None, int(num_steps),
                       learning_rate, report_interval, clip_value, max_norm, verbose)
    return data, log


def _color_frames(vertices, triangles, data, cameras, width, height):
    """-> ``frame(number)``: K31's picture of ``cameras[number]`` with the vertex colours ``data`` as
    they are at the call -> (color, alpha, (record, ids)).  One read-back per frame."""
    from .cameras import eye_positions
    projections = [supersample_projection(camera, 1) for camera in cameras]
    eyes = eye_positions(cameras, (0.0, 0.0, 0.0))

    def frame(number):
        record, color, alpha, _, ids, _, _ = _rasterize(
            vertices, triangles, projections[number], eyes[number], width, height, data)
        return color, alpha, (record, ids)
    return frame


def fit_mesh_colors(vertices, triangles, colors, train_dataset, val_dataset=None,
                    num_steps: int = 500, learning_rate: float = 1e-2, cameras_per_step: int = 1,
                    report_interval: int = 100, alpha_threshold=None,
                    clip_value: float = CLIP_VALUE, max_norm: float = MAX_NORM,
                    seed: int = 20080524, verbose: bool = True):
    """Optimises the per-vertex ``colors`` (V,3) of a mesh against the images of ``train_dataset``
    (an ``ImageDataset``) through ``render_mesh`` with a black background -> ``(colors, log)``;
    the geometry is not changed.  numpy in gives numpy out; tensors stay tensors, and the given
    ``colors`` are not modified.  The loop is ``fit_octree``'s on a (V,3) buffer, with whole
    cameras for batches: a seeded permutation of the cameras is dealt ``cameras_per_step`` at a
    time, and one step is, for each of its cameras, the K31 frame, K6 (``ops.mse_loss``) on that
    camera's pixels with ``color_scale = 1 / (3 count)`` (``count`` the pixels of the step) and
    no alpha term, the optional alpha mask, and K32 accumulated over the step's cameras; then K7
    (``ops.clip_adam`` with ``clip_value`` / ``max_norm``, defaults those of ``fit_octree``) and
    ``clamp_(0, 1)``.  With ``alpha_threshold`` the gradient of a pixel whose own alpha byte is
    below ``ceil(alpha_threshold * 255)`` (clamped into 1 .. 255) is set to zero; None, the
    default, masks nothing.  The dataset's colours count as black where its alpha is 0, as in
    every fit here.

    The log holds ``FitLogEntry(step, loss, val_psnr)``: every step's training loss (the mean
    squared colour error of the step's pixels), ``val_psnr`` over all pixels of ``val_dataset``'s
    cameras at steps below 10 and multiples of ``report_interval``, else NaN; report steps are
    printed as ``fit_octree`` prints them.  The only host synchronisation of a step is the
    read-back inside ``ops.mesh_raster_offsets`` (one per camera), as K17b has one; the losses are
    fetched at the end.  ``learning_rate`` has NO tuned default: 1e-2 is ``fit_octree``'s."""
    who = "fit_mesh_colors"
    num_vertices = _mesh_colors_check(who, vertices, colors)
    if colors is None:
        raise ValueError("%s: colors must be (V,3), got None (color_mesh_from_images makes a "
                         "start)" % who)

    def setup(vertices, triangles, data, view, val_view):
        order, starts = vertex_adjacency(triangles, num_vertices, data.device)

        def transpose(ctx, d_color, grads, weight, accumulate):
            face_sums = ops.mesh_raster_face_sums(ctx[0], ctx[1], d_color, view[1], view[2])
            ops.mesh_vertex_gather(face_sums, order, starts, grads, weight, accumulate=accumulate)
        # (validation rasterises anew at each report: the colours have changed)
        val_frame = None if val_view is None else \
            _color_frames(vertices, triangles, data, *val_view)
        return _color_frames(vertices, triangles, data, *view), val_frame, transpose

    data, log = _fit_mesh(who, num_vertices, vertices, triangles, colors, setup, train_dataset,
                          val_dataset, num_steps, learning_rate, cameras_per_step, report_interval,
                          alpha_threshold, clip_value, max_norm, seed, verbose)
    return (data if torch.is_tensor(vertices) else data.cpu().numpy()), log


# ------------------------------------------------------------------------------------ K33
class MeshTaps(NamedTuple("MeshTaps", [("tap_texel", torch.Tensor), ("tap_weight", torch.Tensor),
                                       ("sorted_texels", torch.Tensor),
                                       ("tap_order", torch.Tensor), ("width", int),
                                       ("height", int)])):
    """K31c's textured picture of one camera as a sparse matrix (K33a and a sort): per pixel the
    four texels ``tap_texel`` (P,4) int32 (``row * width + column``, -1 where nothing is drawn) and
    weights ``tap_weight`` (P,4) float32 of the bilinear lookup; ``sorted_texels`` and
    ``tap_order`` (4P,) int32, the tap slots ``4 p + k`` stably sorted by texel, which K33c reads;
    ``width`` and ``height`` of the TEXTURE.  64 bytes per pixel."""

    @property
    def num_texels(self) -> int:
        return self.width * self.height


def _power_of_two(n: int) -> int:
    return 1 << max(int(n) - 1, 0).bit_length()


def _atlas_size(num_tiles: int, tile: int):
    """The smallest powers of two (width, height), width = height or 2 height, whose
    ``(width // tile) * (height // tile)`` tiles hold ``num_tiles``."""
    width = height = _power_of_two(tile)
    while (width // tile) * (height // tile) < num_tiles:
        if width == height:
            width *= 2
        else:
            height *= 2
    return width, height


def unwrap_mesh(vertices, triangles, tile: int = 4):
    """A texture atlas for a mesh without UVs -> ``(vertices', triangles', uvs, vertex_map,
    (height, width))``: one ``tile x tile`` square of texels per quad.  Host-only, integer work.

    Triangles ``2k`` and ``2k + 1`` share a tile when both have three distinct vertex ids and they
    share exactly two of them (``OcTree.extract_mesh`` writes every quad as ``(q0, q1, q2), (q0,
    q2, q3)``); the shared edge lies on the tile's diagonal.  Every other triangle gets a tile of
    its own and uses its lower-left half.  The corners sit at the tile-local texel coordinates 0.5
    and ``tile - 1.5``: a lone triangle's at ``(0.5, 0.5), (tile - 1.5, 0.5), (0.5, tile - 1.5)`` in
    the order of its corners; of a pair the first triangle's unshared corner at ``(0.5, 0.5)``, the
    next two (in its winding) at ``(tile - 1.5, 0.5)`` and ``(0.5, tile - 1.5)``, and the partner's
    unshared corner at ``(tile - 1.5, tile - 1.5)``.  A bilinear lookup at texel coordinate ``x``
    reads the texels ``floor(x)`` and ``floor(x) + 1``, so every tap of every pixel of a triangle
    stays inside its own tile, whatever the roundings of the interpolated ``u``: neighbouring tiles
    never bleed into each other.  ``tile >= 3``.

    The tiles are laid out row-major, in the order of the triangles, in a texture whose ``width``
    and ``height`` are the smallest powers of two that hold them (``width`` = ``height`` or twice
    it): ``u * width`` is exact in float32.  ``v`` grows with the row index, the kernels'
    orientation.  Vertices are duplicated per tile, 4 per pair and 3 per lone triangle, numbered in
    the order the triangles first use them (so ``load_obj`` of a saved atlas returns these arrays);
    ``vertex_map`` (V',) int32 names the original vertex: ``vertices' = vertices[vertex_map]``,
    ``vertex_map[triangles'] = triangles``, and colours and normals follow the same way."""
    who = "unwrap_mesh"
    points = np.asarray(vertices)
    if points.ndim != 2 or points.shape[1] != 3 or len(points) == 0:
        raise ValueError("%s: vertices must be (V,3) with V >= 1, got %s" % (who, points.shape))
    tri = _check_triangles(who, triangles, len(points)).astype(np.int64)
    if int(tile) != tile or tile < 3:
        raise ValueError("%s: tile must be an integer >= 3, got %r" % (who, tile))
    tile = int(tile)
    count = len(tri)
    pairs = count // 2
    first, second = tri[0:2 * pairs:2], tri[1:2 * pairs:2]

    def distinct(t):
        return (t[:, 0] != t[:, 1]) & (t[:, 1] != t[:, 2]) & (t[:, 0] != t[:, 2])

    equal = first[:, :, None] == second[:, None, :]              # [pair, corner of 2k, of 2k+1]
    in_second, in_first = equal.any(2), equal.any(1)
    paired = distinct(first) & distinct(second) & (in_second.sum(1) == 2)
    joined = np.zeros(count, dtype=bool)                          # the second triangle of a pair
    joined[1:2 * pairs:2] = paired
    opens = np.zeros(count, dtype=bool)                           # the first triangle of a pair
    opens[0:2 * pairs:2] = paired
    tile_of = np.cumsum(~joined) - 1
    num_tiles = int(tile_of[-1]) + 1
    width, height = _atlas_size(num_tiles, tile)
    if width * height > ops.MESH_TEXTURE_MAX_TEXELS:
        raise ValueError("%s: %d tiles of %d x %d need a %d x %d texture; at most (2^31 - 1) / 3 "
                         "texels are supported" % (who, num_tiles, tile, tile, width, height))
    # the vertices a tile owns: 3 for its first triangle, one more for a partner
    owned = np.where(joined, 1, 3)
    base = np.cumsum(owned) - owned                               # the first new vertex of a triangle
    new_tri = base[:, None] + np.arange(3)
    lo, hi = 0.5, tile - 1.5
    spots = np.array([[lo, lo], [hi, lo], [lo, hi], [hi, hi]])    # P0 P1 P2 and the partner's P3
    local = np.zeros((count, 3, 2))
    local[:] = spots[:3]
    vertex_map = np.empty(int(owned.sum()), dtype=np.int64)
    vertex_map[new_tri[~joined].reshape(-1)] = tri[~joined].reshape(-1)
    if paired.any():
        a, b = np.flatnonzero(opens), np.flatnonzero(joined)
        alone = np.argmin(in_second[paired], 1)                   # the first's unshared corner
        other = np.argmin(in_first[paired], 1)                    # the partner's unshared corner
        turn = (np.arange(3)[None, :] - alone[:, None]) % 3       # corner -> P0, P1, P2
        local[a] = spots[turn]
        # the partner: its shared corners are the first's, its own gets the tile's fourth vertex
        match = np.argmax(equal[paired], 1)                       # [pair, corner of 2k+1] -> of 2k
        new_tri[b] = np.take_along_axis(new_tri[a], match, 1)
        local[b] = np.take_along_axis(local[a], match[:, :, None], 1)
        new_tri[b, other] = base[b]
        local[b, other] = spots[3]
        vertex_map[base[b]] = tri[b, other]
    tiles_per_row = width // tile
    origin = np.stack([tile_of % tiles_per_row, tile_of // tiles_per_row], 1) * tile
    texel = origin[:, None, :] + local                            # (F,3,2) in texel coordinates
    uvs = np.zeros((len(vertex_map), 2), dtype=np.float64)
    uvs[new_tri.reshape(-1)] = texel.reshape(-1, 2) / np.array([width, height], dtype=np.float64)
    return (points[vertex_map], new_tri.astype(np.int32), uvs.astype(np.float32),
            vertex_map.astype(np.int32), (height, width))


def bake_vertex_colors(colors, triangles, uvs, size, tile: int):
    """Per-vertex colours of an ``unwrap_mesh`` atlas as a texture -> (H,W,3) float32 in the
    kernels' orientation.  Host-only.  Every texel of a tile takes the barycentric blend of its
    triangle's corner colours at the texel's own position (texel ``j`` lies at texel coordinate
    ``j``); in a pair's tile the texels beyond the diagonal take the partner's.  Texels outside the
    corners extrapolate and are clamped to [0, 1]; texels of no tile get the mean colour.  A fit
    that starts here starts from what K30 or K32 produced, and texels that no camera sees keep a
    sensible colour."""
    who = "bake_vertex_colors"
    colors = np.asarray(colors, dtype=np.float64)
    if colors.ndim != 2 or colors.shape[1] != 3 or len(colors) == 0:
        raise ValueError("%s: colors must be (V,3) with V >= 1, got %s" % (who, colors.shape))
    tri = _check_triangles(who, triangles, len(colors)).astype(np.int64)
    if np.shape(uvs) != (len(colors), 2):
        raise ValueError("%s: uvs must be (V,2) = (%d,2), got %s"
                         % (who, len(colors), np.shape(uvs)))
    if int(tile) != tile or tile < 3:
        raise ValueError("%s: tile must be an integer >= 3, got %r" % (who, tile))
    tile = int(tile)
    height, width = (int(s) for s in size)
    if height < tile or width < tile:
        raise ValueError("%s: size must be (height, width) of at least one tile, got %r"
                         % (who, size))
    texture = np.empty((height, width, 3), dtype=np.float64)
    texture[:] = colors.mean(0)
    texel = np.asarray(uvs, dtype=np.float64)[tri] * np.array([width, height], dtype=np.float64)
    origin = np.floor(texel.min(1) / tile).astype(np.int64) * tile          # (F,2) column, row
    if (origin < 0).any() or (origin[:, 0] + tile > width).any() \
            or (origin[:, 1] + tile > height).any():
        raise ValueError("%s: a triangle's uvs lie outside the %d x %d texture" % (who, width,
                                                                                    height))
    local = texel - origin[:, None, :]
    upper = local.sum(2).max(1) > tile - 1 + 0.25           # it owns the corner (tile-1.5, tile-1.5)
    edge1, edge2 = local[:, 1] - local[:, 0], local[:, 2] - local[:, 0]
    det = edge1[:, 0] * edge2[:, 1] - edge1[:, 1] * edge2[:, 0]
    if (det == 0).any():
        raise ValueError("%s: a triangle's uvs are collinear" % who)
    ly, lx = np.meshgrid(np.arange(tile), np.arange(tile), indexing="ij")
    dx = lx[None] - local[:, 0, 0, None, None]
    dy = ly[None] - local[:, 0, 1, None, None]
    w1 = (dx * edge2[:, 1, None, None] - dy * edge2[:, 0, None, None]) / det[:, None, None]
    w2 = (dy * edge1[:, 0, None, None] - dx * edge1[:, 1, None, None]) / det[:, None, None]
    c0, c1, c2 = (colors[tri[:, i]][:, None, None, :] for i in range(3))
    blend = c0 + w1[..., None] * (c1 - c0) + w2[..., None] * (c2 - c0)       # (F,tile,tile,3)
    rows = origin[:, 1, None, None] + ly[None]
    cols = origin[:, 0, None, None] + lx[None]
    beyond = (lx + ly > tile - 1)[None]
    for chosen, mask in ((~upper, np.ones_like(beyond)), (upper, beyond)):
        keep = np.broadcast_to(mask, rows.shape)[chosen]
        texture[rows[chosen][keep], cols[chosen][keep]] = blend[chosen][keep]
    return np.clip(texture, 0.0, 1.0).astype(np.float32)


def texture_to_uint8(texture) -> np.ndarray:
    """A float (H,W,3) texture in the kernels' orientation -> (H,W,3) uint8 with row 0 at the top,
    as ``load_obj`` returns one and ``render_mesh`` and ``save_obj`` take it:
    ``floor(x * 255 + 0.5)`` in float32, clamped into 0 .. 255 (NaN gives 0)."""
    values = texture.detach().cpu().numpy() if torch.is_tensor(texture) else np.asarray(texture)
    if values.ndim != 3 or values.shape[2] != 3 or not np.issubdtype(values.dtype, np.floating):
        raise ValueError("texture_to_uint8: texture must be a float (H,W,3) array, got %s %s"
                         % (values.dtype, values.shape))
    with np.errstate(invalid="ignore"):
        scaled = np.floor(values.astype(np.float32) * np.float32(255.0) + np.float32(0.5))
        scaled = np.fmin(np.fmax(np.nan_to_num(scaled, nan=0.0), 0.0), 255.0)
    return np.ascontiguousarray(scaled.astype(np.uint8)[::-1])


def _texture_check(who, texture):
    """A float (H,W,3) texture within K33's limits -> (height, width).  No device."""
    shape = _shape_of(texture)
    floating = hasattr(texture, "dtype") and (
        texture.dtype.is_floating_point if torch.is_tensor(texture)
        else np.issubdtype(texture.dtype, np.floating))
    if len(shape) != 3 or shape[2] != 3 or min(shape) < 1 or not floating:
        raise ValueError("%s: texture must be a float (H,W,3) array in the kernels' orientation, "
                         "got %s %s" % (who, getattr(texture, "dtype", type(texture).__name__),
                                        shape))
    _texture_size_check(who, shape[:2])
    return int(shape[0]), int(shape[1])


def _texture_size_check(who, size):
    try:
        height, width = (int(s) for s in size)
    except (TypeError, ValueError):
        raise ValueError("%s: size must be (height, width), got %r" % (who, size)) from None
    if (not 1 <= height <= ops.MESH_MAX_TEXTURE_SIDE or not 1 <= width <= ops.MESH_MAX_TEXTURE_SIDE
            or height * width > ops.MESH_TEXTURE_MAX_TEXELS):
        raise ValueError("%s: the texture must be 1 .. 2^24 a side with at most (2^31 - 1) / 3 "
                         "texels, got %r" % (who, tuple(size)))
    return height, width


def _mesh_uvs_check(who, vertices, uvs, supersample=1, batch_size=1) -> int:
    """What every K33 function refuses of its mesh from shapes alone -> V."""
    shape = _shape_of(vertices)
    if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
        raise ValueError("%s: vertices must be (V,3) with V >= 1, got %s" % (who, shape))
    if uvs is None or _shape_of(uvs) != (shape[0], 2):
        raise ValueError("%s: uvs must be (V,2) = (%d,2), got %s (unwrap_mesh makes an atlas)"
                         % (who, shape[0], None if uvs is None else _shape_of(uvs)))
    if supersample != 1:
        raise ValueError("%s: supersample must be 1 (the backward of the k x k mean is not "
                         "built), got %r" % (who, supersample))
    if int(batch_size) != batch_size or batch_size < 1:
        raise ValueError("%s: batch_size must be an integer >= 1, got %r" % (who, batch_size))
    return shape[0]


def _taps(vertices, triangles, uvs, proj, width, height, size, batch_size=1 << 22, hidden=None):
    """K31a-c for the ids, K33a, and the stable sort of the tap slots by texel -> MeshTaps.
    ``hidden`` (H W,) bool marks pixels that count as uncovered."""
    record, ids = _raster_ids(vertices, triangles, proj, width, height, batch_size)
    if hidden is not None:
        ids = ids.masked_fill(hidden, -1)
    tap_texel, tap_weight = ops.mesh_texture_taps(record, ids, triangles, uvs, size[0], size[1],
                                                  width, height)
    # integer plumbing, as the key sort of OcTree.extract_mesh and vertex_adjacency
    sorted_texels, order = torch.sort(tap_texel.reshape(-1), stable=True)
    return MeshTaps(tap_texel, tap_weight, sorted_texels.contiguous(),
                    order.to(torch.int32).contiguous(), int(size[1]), int(size[0]))


def mesh_texture_taps(vertices, triangles, uvs, camera, size, batch_size: int = 1 << 22,
                      supersample: int = 1) -> MeshTaps:
    """The picture ``render_mesh(uvs=, texture=)`` draws from ``camera`` as a sparse matrix in the
    texture -> ``MeshTaps`` of GPU tensors, for a texture of ``size = (height, width)``: K31a-c for
    the ids of the z-buffer, K33a for the four texels and weights of every pixel (the bits K31c
    uses), and a torch stable sort of the tap slots by texel for K33c.  It depends on the geometry,
    the camera and the UVs alone: made once per camera, it serves every step of a fit.  64 bytes
    per pixel.  The read-backs of K31 (one per call) are the only host synchronisation."""
    who = "mesh_texture_taps"
    num_vertices = _mesh_uvs_check(who, vertices, uvs, supersample, batch_size)
    width, height = _camera_size(who, camera)
    size = _texture_size_check(who, size)
    _mesh_ids_check(who, triangles, num_vertices)
    _, device, vertices, triangles = _mesh_on(vertices, triangles)
    return _taps(vertices, triangles, _on(uvs, "float32", device),
                 supersample_projection(camera, 1), width, height, size, int(batch_size))


def _taps_check(who, taps):
    if not isinstance(taps, MeshTaps):
        raise ValueError("%s: taps must be a MeshTaps (mesh_texture_taps makes one), got %s"
                         % (who, type(taps).__name__))


def render_mesh_texture(taps: MeshTaps, texture, background=(0, 0, 0)):
    """K33b: the picture of ``taps`` for a float ``texture`` (H,W,3) in the kernels' orientation
    (the row index growing with ``v``; plain floats, no ``/ 255``) -> ``RenderResult(color (P,3),
    alpha (P,), None)``: the depth is not recomputed here.  A numpy texture gives numpy results.
    With ``texture = uint8 / 255`` the colours are K31c's within a rounding or two (K31c divides
    after the blend)."""
    who = "render_mesh_texture"
    _taps_check(who, taps)
    if _texture_check(who, texture) != (taps.height, taps.width):
        raise ValueError("%s: texture must be (%d,%d,3) as the taps were made for, got %s"
                         % (who, taps.height, taps.width, _shape_of(texture)))
    from .utils import RenderResult
    as_numpy = not torch.is_tensor(texture)
    flat = _on(texture, "float32", taps.tap_texel.device).reshape(-1, 3)
    color, alpha = ops.mesh_texture_gather(taps.tap_texel, taps.tap_weight, flat, background)
    out = RenderResult(color, alpha, None)
    return out.numpy() if as_numpy else out


def render_mesh_texture_backward(taps: MeshTaps, d_color, grad=None, weight=None,
                                 accumulate: bool = False):
    """K33c: the transpose of ``render_mesh_texture`` -> ``(grad (H,W,3), weight (H,W))`` float32
    of the texture: ``grad[t] = sum w d_color[p]`` over the taps of texel ``t`` and ``weight[t] =
    sum w``, in the fixed order of the sorted slots, no float atomics.  ``grad`` and ``weight`` (GPU
    tensors of those shapes, or flat (T,3) and (T,)) are written in place when given, and added to
    with ``accumulate``: how several cameras fold into one buffer.  A numpy ``d_color`` gives numpy
    results."""
    who = "render_mesh_texture_backward"
    _taps_check(who, taps)
    num_pixels = taps.tap_texel.shape[0]
    if _shape_of(d_color) != (num_pixels, 3):
        raise ValueError("%s: d_color must be (H W,3) = (%d,3), got %s"
                         % (who, num_pixels, _shape_of(d_color)))
    if (grad is None) != (weight is None) or (accumulate and grad is None):
        raise ValueError("%s: give both grad and weight, or neither; accumulate needs them" % who)
    as_numpy = not torch.is_tensor(d_color)
    shaped = (taps.height, taps.width)
    if grad is not None:
        if not torch.is_tensor(grad) or not torch.is_tensor(weight) \
                or grad.numel() != 3 * taps.num_texels or weight.numel() != taps.num_texels:
            raise ValueError("%s: grad must be a (%d,%d,3) and weight a (%d,%d) tensor"
                             % ((who,) + shaped + shaped))
    flat_grad = None if grad is None else grad.view(-1, 3)
    flat_weight = None if weight is None else weight.view(-1)
    out_grad, out_weight = ops.mesh_texture_grad(
        taps.sorted_texels, taps.tap_order, taps.tap_weight,
        _on(d_color, "float32", taps.tap_texel.device), taps.num_texels, flat_grad, flat_weight,
        accumulate)
    if grad is None:
        grad, weight = out_grad.view(shaped + (3,)), out_weight.view(shaped)
    if as_numpy:
        return grad.cpu().numpy(), weight.cpu().numpy()
    return grad, weight


def texture_mesh_from_images(vertices, triangles, uvs, dataset, size, texture=None,
                             alpha_threshold: float = 0.5):
    """Gives every texel the weighted mean colour of the pixels that see it -> ``(texture (H,W,3),
    weights (H,W))`` float32 in the kernels' orientation (numpy in gives numpy out; tensors stay
    tensors): ``color_mesh_from_images`` for texels.  Over the cameras of ``dataset`` in order, K33c
    accumulates ``sum w rgb[p] / 255`` and ``sum w`` per texel, ``w`` the bilinear weights of K31c;
    a pixel whose own alpha byte is below ``ceil(alpha_threshold * 255)`` (clamped into 1 .. 255)
    counts as uncovered.  A texel with ``weight > 0`` gets ``sum / weight``, one f32 division per
    channel on the host; any other keeps ``texture[t]``, or 0.5 grey when ``texture`` is None."""
    who = "texture_mesh_from_images"
    num_vertices = _mesh_uvs_check(who, vertices, uvs)
    size = _texture_size_check(who, size)
    if texture is not None and _texture_check(who, texture) != size:
        raise ValueError("%s: texture must be (%d,%d,3), got %s"
                         % (who, size[0], size[1], _shape_of(texture)))
    alpha_u8 = _alpha_byte(who, alpha_threshold)
    images, cameras, width, height = _mesh_dataset_check(who, "dataset", dataset)
    _mesh_ids_check(who, triangles, num_vertices)
    as_numpy, device, vertices, triangles = _mesh_on(vertices, triangles)
    uvs = _on(uvs, "float32", device)
    num_texels = size[0] * size[1]

    def splat(camera, hidden, rgb, total, weights, accumulate):
        taps = _taps(vertices, triangles, uvs, supersample_projection(camera, 1), width, height,
                     size, hidden=hidden)
        ops.mesh_texture_grad(taps.sorted_texels, taps.tap_order, taps.tap_weight, rgb,
                              num_texels, total, weights, accumulate=accumulate)

    out, weights = _mean_from_images(images, cameras, alpha_u8, texture, num_texels, splat,
                                     device, as_numpy)
    return out.reshape(size + (3,)), weights.reshape(size)


def _texture_frames(vertices, triangles, uvs, data, cameras, width, height, size, keep=True):
    """-> ``frame(number)``: K33b's picture of ``cameras[number]`` with the texels ``data`` (T,3) as
    they are at the call -> (color, alpha, taps).  A camera's taps are built when its frame is first
    asked for (K31a-c + K33a + the sort, with K31's read-backs) and, with ``keep``, kept: a later
    frame of that camera has no host synchronisation."""
    projections = [supersample_projection(camera, 1) for camera in cameras]
    cache = {}

    def frame(number):
        taps = cache.get(number)
        if taps is None:
            taps = _taps(vertices, triangles, uvs, projections[number], width, height, size)
            if keep:
                cache[number] = taps
        color, alpha = ops.mesh_texture_gather(taps.tap_texel, taps.tap_weight, data)
        return color, alpha, taps
    return frame


def fit_mesh_texture(vertices, triangles, uvs, texture, train_dataset, val_dataset=None,
                     num_steps: int = 500, learning_rate: float = 1e-2, cameras_per_step: int = 1,
                     report_interval: int = 100, alpha_threshold=None,
                     clip_value: float = CLIP_VALUE, max_norm: float = MAX_NORM,
                     seed: int = 20080524, cache_taps: bool = True, verbose: bool = True):
    """Optimises the float ``texture`` (H,W,3, the kernels' orientation) of a mesh with ``uvs``
    against the images of ``train_dataset`` with a black background -> ``(texture, log)``; the
    geometry and the UVs are not changed.  numpy in gives numpy out; tensors stay tensors, and the
    given ``texture`` is not modified.  ``fit_mesh_colors``' loop on a (T,3) buffer: the same
    seeded deal of the cameras, ``cameras_per_step`` at a time, and one step is, for each of its
    cameras, the taps (from the cache, or K31a-c + K33a + the sort when ``cache_taps`` is off), the
    K33b frame, K6 (``ops.mse_loss``) on that camera's pixels with ``color_scale = 1 / (3 count)``
    and no alpha term, the optional alpha mask (``alpha_threshold``, as in ``fit_mesh_colors``),
    and K33c accumulated over the step's cameras; then K7 (``ops.clip_adam``) and ``clamp_(0, 1)``.

    The log holds ``FitLogEntry(step, loss, val_psnr)`` as ``fit_mesh_colors``' does, and report
    steps are printed the same way.  With the cache (64 bytes per pixel and camera) a step has no
    host synchronisation at all: the only ones are the read-backs of K31 when a camera's taps are
    first built; without it every camera of every step pays them.  The bits do not depend on
    ``cache_taps``.  ``learning_rate`` has NO tuned default: 1e-2 is ``fit_octree``'s."""
    who = "fit_mesh_texture"
    num_vertices = _mesh_uvs_check(who, vertices, uvs)
    if texture is None:
        raise ValueError("%s: texture must be a float (H,W,3) array, got None "
                         "(texture_mesh_from_images or bake_vertex_colors makes a start)" % who)
    size = _texture_check(who, texture)

    def setup(vertices, triangles, data, view, val_view):
        mesh = (vertices, triangles, _on(uvs, "float32", data.device), data)

        def transpose(taps, d_color, grads, weight, accumulate):
            ops.mesh_texture_grad(taps.sorted_texels, taps.tap_order, taps.tap_weight, d_color,
                                  data.shape[0], grads, weight, accumulate=accumulate)
        # (the validation taps are built once, at the first report)
        val_frame = None if val_view is None else _texture_frames(*mesh, *val_view, size)
        return _texture_frames(*mesh, *view, size, keep=cache_taps), val_frame, transpose

    data, log = _fit_mesh(who, num_vertices, vertices, triangles, texture, setup, train_dataset,
                          val_dataset, num_steps, learning_rate, cameras_per_step, report_interval,
                          alpha_threshold, clip_value, max_norm, seed, verbose)
    data = data.view(size + (3,))
    return (data if torch.is_tensor(texture) else data.cpu().numpy()), log


# ------------------------------------------------------------------------------------ K34
def _triangle_ids(who, triangles, num_vertices) -> np.ndarray:
    """(F,3) int64 on the host, clamped into ``0 .. V - 1`` as K31 clamps them."""
    shape = _shape_of(triangles)
    if torch.is_tensor(triangles):
        integer = not (triangles.dtype.is_floating_point or triangles.dtype.is_complex
                       or triangles.dtype == torch.bool)
    else:
        integer = np.issubdtype(np.asarray(triangles).dtype, np.integer)
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= _MOST or not integer:
        raise ValueError("%s: triangles must be an integer (F,3) array with 1 <= F <= "
                         "(2^31 - 1) / 3, got %s" % (who, shape))
    if int(num_vertices) != num_vertices or not 1 <= int(num_vertices) <= _MOST:
        raise ValueError("%s: num_vertices must be an integer in 1 .. (2^31 - 1) / 3, got %r"
                         % (who, num_vertices))
    ids = triangles.cpu().numpy() if torch.is_tensor(triangles) else np.asarray(triangles)
    return np.clip(ids.astype(np.int64), 0, int(num_vertices) - 1)


def _plumbing_device(triangles, device):
    if device is None:
        device = triangles.device if torch.is_tensor(triangles) else "cuda"
    return torch.device(device)


def edge_opposites(triangles, num_vertices: int, device=None) -> torch.Tensor:
    """Which vertex lies across every edge -> ``opposite`` (3F,) int32 on ``device`` (default: the
    tensor's own, or the GPU for a numpy array), what K34 takes.  Edge ``i`` of triangle ``f`` joins
    its corners ``i + 1`` and ``i + 2`` (mod 3), K31b's numbering.  ``opposite[3 f + i]`` is the
    vertex of the neighbouring triangle that is not on the edge when the undirected edge is used
    by exactly two corners of two different triangles, and -1 otherwise: a boundary edge, an edge
    shared by three or more triangles, an edge a degenerate triangle uses twice.  The ids are
    clamped into ``0 .. V - 1`` as K31 clamps them.  A numpy sort on the host, integer plumbing
    as ``vertex_adjacency``; it depends on the triangles alone and is made once per mesh."""
    ids = _triangle_ids("edge_opposites", triangles, num_vertices)
    j, k = ids[:, [1, 2, 0]].reshape(-1), ids[:, [2, 0, 1]].reshape(-1)      # corner 3 f + i
    keys = np.minimum(j, k) * int(num_vertices) + np.maximum(j, k)
    order = np.argsort(keys, kind="stable")
    ranked = keys[order]
    first = np.ones(len(ranked), dtype=bool)
    first[1:] = ranked[1:] != ranked[:-1]
    starts = np.flatnonzero(first)
    sizes = np.diff(np.append(starts, len(ranked)))
    opposite = np.full(len(keys), -1, dtype=np.int32)
    two = starts[sizes == 2]
    a, b = order[two], order[two + 1]
    apart = a // 3 != b // 3
    a, b = a[apart], b[apart]
    flat = ids.reshape(-1)
    opposite[a], opposite[b] = flat[b], flat[a]
    return torch.from_numpy(opposite).to(_plumbing_device(triangles, device))


def vertex_neighbors(triangles, num_vertices: int, device=None):
    """The vertices every vertex shares an edge with -> ``(starts (V+1,) int32, neighbors int32)``
    on ``device``, the CSR K34d takes: ``neighbors[starts[v] : starts[v + 1]]`` in ascending
    order, every undirected edge once per end, an edge from a vertex to itself left out.  The ids
    are clamped as K31 clamps them.  Integer plumbing on the host, made once per mesh."""
    ids = _triangle_ids("vertex_neighbors", triangles, num_vertices)
    num_vertices = int(num_vertices)
    j, k = ids[:, [1, 2, 0]].reshape(-1), ids[:, [2, 0, 1]].reshape(-1)
    keep = j != k
    keys = np.unique(np.concatenate([j[keep] * num_vertices + k[keep],
                                     k[keep] * num_vertices + j[keep]]))
    if len(keys) >= 2 ** 31:
        raise ValueError("vertex_neighbors: %d neighbour ids; fewer than 2^31 are supported"
                         % len(keys))
    starts = np.zeros(num_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(keys // num_vertices, minlength=num_vertices), out=starts[1:])
    device = _plumbing_device(triangles, device)
    return (torch.from_numpy(starts.astype(np.int32)).to(device),
            torch.from_numpy((keys % num_vertices).astype(np.int32)).to(device))


def _geometry_backward(frame, opposites, vertices, triangles, proj, width, height, g_color,
                       g_alpha, grad, accumulate):
    """K34b, the stable sort of its entries and K34c on one K31 frame ``(record, color, alpha,
    ids, zbuf)`` -> (grad, d_color, d_alpha).  No read-back."""
    record, color, alpha, ids, zbuf = frame
    d_color, d_alpha, entry_vertex, entry_grad = ops.mesh_aa_backward(
        record, zbuf, ids, opposites, vertices, triangles, proj, color, alpha, g_color, g_alpha,
        width, height)
    sorted_vertex, order = torch.sort(entry_vertex, stable=True)
    grad = ops.mesh_aa_vertex_grad(sorted_vertex.contiguous(), order.to(torch.int32).contiguous(),
                                   entry_grad, vertices, proj, grad, accumulate)
    return grad, d_color, d_alpha


def _interior_backward(frame, adjacency, vertices, triangles, colors, proj, width, height,
                       d_color, grad):
    """K35a on K34b's ``d_color`` (the gradient in K31's plain colour) and K35b added into ``grad``,
    which already holds K34c's result for this frame.  No read-back."""
    record, _, _, ids, _ = frame
    face_grads = ops.mesh_interp_face_grads(record, ids, d_color, colors, triangles, width, height)
    return ops.mesh_interp_vertex_grad(face_grads, adjacency[0], adjacency[1], vertices, proj,
                                       grad, accumulate=True)


def render_mesh_geometry_backward(vertices, triangles, camera, colors, d_color, d_alpha,
                                  opposites=None, grad=None, accumulate: bool = False,
                                  background=(0, 0, 0), batch_size: int = 1 << 22,
                                  interior: bool = False, adjacency=None):
    """The transpose of ``render_mesh(..., colors=colors, antialias=True)`` in the vertex
    POSITIONS (K34, ``csrc/mesh_aa.hip``) -> ``(grad (V,3), d_color_plain (H W,3))`` float32.
    ``d_color`` (H W,3) and ``d_alpha`` (H W,) are the gradient of a loss in the antialiased colour
    and alpha; ``grad`` is its gradient in the positions, and ``d_color_plain`` the gradient in
    K31's own colours, which is what ``render_mesh_backward`` (K32) takes: colours and geometry
    can share one backward.  It runs K31 for the camera, then K34b, a stable sort of its vertex
    entries and K34c: fixed orders, no float atomics, the same bits on every call and for every
    ``batch_size``.

    numpy in gives numpy out; tensors stay tensors.  ``opposites``: what ``edge_opposites``
    returns for these triangles (made here when None).  ``grad`` (a GPU tensor) is written in
    place when given, and added to with ``accumulate``.

    ``interior=True`` adds the other half of the gradient (K35, ``csrc/mesh_interp_grad.hip``):
    colour through the barycentric weights.  After K34b, the sort and K34c it runs K35a on K34b's
    ``d_color_plain`` and K35b with ``accumulate`` into the same ``grad``, so a vertex that lies
    on no outline is moved by the colours sliding over its triangles.  ``adjacency``: what
    ``vertex_adjacency`` returns for these triangles (made here when None; not used without
    ``interior``).  With the default ``False`` none of K35 is reached and the result is
    unchanged bit for bit.

    The limits: without ``interior`` only silhouette and fold edges (and boundary and
    non-manifold ones) carry a gradient.  With it: which triangle wins a pixel is held fixed (a
    change of visibility is seen at silhouettes only, by K34); the snap to 1/256 pixel is passed
    straight through; the topology never changes; a silhouette that falls between two pixel
    centres of the same id is not seen; self-intersections are not prevented.  The interior term
    has no textured path (the derivative of the bilinear lookup in the UVs is not built), and a
    screen-filling triangle is one wavefront's loop, as in K32a."""
    who = "render_mesh_geometry_backward"
    num_vertices = _mesh_colors_check(who, vertices, colors, batch_size=batch_size)
    if colors is None:
        raise ValueError("%s: colors must be (V,3), got None" % who)
    width, height = _camera_size(who, camera)
    if _shape_of(d_color) != (width * height, 3):
        raise ValueError("%s: d_color must be (H W,3) = (%d,3), got %s"
                         % (who, width * height, _shape_of(d_color)))
    if _shape_of(d_alpha) != (width * height,):
        raise ValueError("%s: d_alpha must be (H W,) = (%d,), got %s"
                         % (who, width * height, _shape_of(d_alpha)))
    if accumulate and grad is None:
        raise ValueError("%s: accumulate needs grad to add to" % who)
    ground = np.asarray(background, dtype=np.float64).reshape(-1)
    if ground.shape != (3,) or not np.isfinite(ground).all():
        raise ValueError("%s: background must be three finite numbers, got %r"
                         % (who, background))
    _mesh_ids_check(who, triangles, num_vertices)
    from .cameras import eye_positions
    as_numpy, device, vertices, triangles = _mesh_on(vertices, triangles)
    if opposites is None:
        opposites = edge_opposites(triangles, num_vertices, device)
    if interior and adjacency is None:
        adjacency = vertex_adjacency(triangles, num_vertices, device)
    proj = supersample_projection(camera, 1)
    colors = _on(colors, "float32", device)
    record, color, alpha, _, ids, _, _, zbuf = _rasterize_z(
        vertices, triangles, proj, eye_positions([camera], (0.0, 0.0, 0.0))[0], width, height,
        colors, background=background, batch_size=batch_size)
    frame = (record, color, alpha, ids, zbuf)
    grad, plain, _ = _geometry_backward(
        frame, opposites, vertices, triangles, proj, width, height,
        _on(d_color, "float32", device), _on(d_alpha, "float32", device), grad, accumulate)
    if interior:
        _interior_backward(frame, adjacency, vertices, triangles, colors, proj, width, height,
                           plain, grad)
    if as_numpy:
        return grad.cpu().numpy(), plain.cpu().numpy()
    return grad, plain


def fit_mesh_geometry(vertices, triangles, colors, train_dataset, val_dataset=None,
                      num_steps: int = 500, learning_rate: float = 1e-3,
                      cameras_per_step: int = 1, report_interval: int = 100, alpha_weight=None,
                      laplacian_weight: float = 0.0, max_displacement=None,
                      clip_value: float = CLIP_VALUE, max_norm: float = MAX_NORM,
                      seed: int = 20080524, verbose: bool = True, interior: bool = False):
    """Optimises the vertex POSITIONS (V,3) of a mesh against the images of ``train_dataset`` (an
    ``ImageDataset``) through ``render_mesh(..., antialias=True)`` with a black background ->
    ``(vertices, log)``; the per-vertex ``colors`` and the triangles are held fixed.  numpy in gives
    numpy out; tensors stay tensors, and the given ``vertices`` are not modified.  The loop is
    ``fit_mesh_colors``' (``fit_loop.run``) on the (V,3) positions: a seeded permutation of the
    cameras is dealt ``cameras_per_step`` at a time, and one step is, for each of its cameras, the
    K31 frame, K34a, K6 (``ops.mse_loss``) on colour and alpha with ``color_scale = 1 / (3 count)``
    and ``alpha_scale = alpha_weight / count`` (``count`` the pixels of the step; ``alpha_weight``
    None takes the dataset's, as ``fit_octree`` does, and 0 for a dataset without alpha), K34b, the
    stable sort of its entries and K34c accumulated over the step's cameras; with ``interior``
    (default off) two more launches per camera, K35a on K34b's gradient in the plain colour and
    K35b accumulated into the same buffer (``csrc/mesh_interp_grad.hip``: colour through the
    barycentric weights; the adjacency is made once, a step gains no host synchronisation, and
    without it none of K35 is reached: results and logs are unchanged bit for bit).  Then, with
    ``laplacian_weight > 0``, K34d on the displacement ``d = v - v0`` adds the gradient of
    ``laplacian_weight * (1 / V) * 1/2 sum_edges |d_i - d_j|^2`` (report lines gain ``lap:``, the
    value of that term; with 0 the kernel is not entered); then K7 (``ops.clip_adam``) and, with
    ``max_displacement``, every component of ``v`` is clamped into ``v0 -+ max_displacement``.

    The log holds ``FitLogEntry(step, loss, val_psnr)`` as ``fit_mesh_colors``' does -- the loss is
    K6's, colour plus ``alpha_weight`` times alpha, without the smoothness term; ``val_psnr`` is
    the colour PSNR of the antialiased pictures of ``val_dataset``'s cameras -- and report steps
    are printed the same way.  The only host synchronisation of a step is K31's one read-back per
    camera.  ``learning_rate``, ``laplacian_weight`` and ``max_displacement`` have NO tuned
    defaults: 1e-3 is a guess in scene units per step, 0 and None switch the two off.

    The limits: without ``interior`` only silhouette and fold edges (and boundary and
    non-manifold ones) carry a gradient, so a vertex that no camera sees on an outline does not
    move.  With it every vertex of a triangle that wins a pixel does, and may slide along the
    surface: thin triangles can fold when nothing smooths them.  In both: which triangle wins a
    pixel is held fixed away from silhouettes; the topology never changes; the snap to 1/256
    pixel is passed straight through; a silhouette that falls between two pixel centres of the
    same id is not seen; self-intersections are not prevented.  The interior term has no textured
    path (``fit_mesh_texture`` does not move geometry), there is no joint colour-and-geometry
    step, and a screen-filling triangle is one wavefront's loop, as in K32a."""
    who = "fit_mesh_geometry"
    num_vertices = _mesh_colors_check(who, vertices, colors)
    if colors is None:
        raise ValueError("%s: colors must be (V,3), got None (color_mesh_from_images makes them)"
                         % who)
    fit_loop.check_schedule(who, "num_steps >= 0, cameras_per_step >= 1, report_interval >= 1",
                            cameras_per_step, num_steps, report_interval, learning_rate)
    cameras_per_step = int(cameras_per_step)
    if alpha_weight is not None and not float(alpha_weight) >= 0:
        raise ValueError("%s: alpha_weight must be None or >= 0, got %r" % (who, alpha_weight))
    laplacian_weight = float(laplacian_weight)
    if not 0 <= laplacian_weight < float("inf"):
        raise ValueError("%s: laplacian_weight must be finite and >= 0, got %r"
                         % (who, laplacian_weight))
    if max_displacement is not None and not float(max_displacement) > 0:
        raise ValueError("%s: max_displacement must be None or positive, got %r"
                         % (who, max_displacement))
    _, cameras, width, height = _mesh_dataset_check(who, "train_dataset", train_dataset)
    val_view = None if val_dataset is None else \
        _mesh_dataset_check(who, "val_dataset", val_dataset)[1:]
    _mesh_ids_check(who, triangles, num_vertices)
    from .cameras import eye_positions
    _, device, start, triangles = _mesh_on(vertices, triangles, train_dataset.colors.device)
    colors = _on(colors, "float32", device)
    data = start.clone()
    opposites = edge_opposites(triangles, num_vertices, device)
    adjacency = vertex_adjacency(triangles, num_vertices, device) if interior else None
    per = width * height
    pixels = torch.arange(per, dtype=torch.int64, device=device)
    alphas = train_dataset._gt_alphas()
    if alphas is None:
        aw = 0.0
    else:
        aw = float(train_dataset.alpha_weight if alpha_weight is None else alpha_weight)
    displacement = neighbor_starts = neighbors = None
    if laplacian_weight > 0:
        neighbor_starts, neighbors = vertex_neighbors(triangles, num_vertices, device)
        displacement = torch.empty_like(data)
    if max_displacement is not None:
        low, high = start - float(max_displacement), start + float(max_displacement)

    def frames(view_cameras, width, height):
        projections = [supersample_projection(camera, 1) for camera in view_cameras]
        eyes = eye_positions(view_cameras, (0.0, 0.0, 0.0))

        def frame(number):
            record, color, alpha, _, ids, _, _, zbuf = _rasterize_z(
                data, triangles, projections[number], eyes[number], width, height, colors)
            smooth = ops.mesh_aa_forward(record, zbuf, ids, opposites, data, projections[number],
                                         color, alpha, width, height)
            return smooth + ((record, color, alpha, ids, zbuf), projections[number])
        return frame

    frame = frames(cameras, width, height)
    val_frame = None if val_view is None else frames(*val_view)
    generator = torch.Generator()
    generator.manual_seed(int(seed))

    def epoch():
        deal = torch.randperm(len(cameras), generator=generator).tolist()
        return [deal[first:first + cameras_per_step]
                for first in range(0, len(deal), cameras_per_step)]

    def step(chosen, grads):
        count = len(chosen) * per
        total = None
        for number, camera in enumerate(chosen):
            color, alpha, plain, proj = frame(camera)
            sums, g_color, g_alpha = ops.mse_loss(color, alpha, train_dataset.colors, alphas,
                                                  pixels + camera * per, 1.0 / (3 * count),
                                                  aw / count)
            _, d_plain, _ = _geometry_backward(plain, opposites, data, triangles, proj, width,
                                               height, g_color, g_alpha, grads, number > 0)
            if interior:
                _interior_backward(plain, adjacency, data, triangles, colors, proj, width, height,
                                   d_plain, grads)
            total = sums if total is None else total + sums
        if laplacian_weight > 0:
            torch.sub(data, start, out=displacement)
            ops.mesh_laplacian(displacement, neighbor_starts, neighbors,
                               laplacian_weight / num_vertices, grads, accumulate=True)
        return ops.loss_value(total, count, aw)

    def project(rows):
        if max_displacement is not None:
            torch.minimum(rows, high, out=rows)
            torch.maximum(rows, low, out=rows)

    def fields():
        if not laplacian_weight > 0:
            return []
        moved = data - start
        rows = torch.repeat_interleave(
            torch.arange(num_vertices, device=device),
            (neighbor_starts[1:] - neighbor_starts[:-1]).to(torch.int64))
        # (every edge is listed once per end: a quarter of the sum over the ends)
        term = 0.25 * ((moved[rows] - moved[neighbors.to(torch.int64)]) ** 2).sum()
        return [("lap", float(term.item()) * laplacian_weight / num_vertices)]

    def validate():
        return fit_loop.camera_psnr(val_frame, len(val_view[0]), val_view[1] * val_view[2],
                                    val_dataset)

    log = fit_loop.run(data, epoch, step, project,
                       validate if val_dataset is not None else None, int(num_steps),
                       learning_rate, report_interval, clip_value, max_norm, verbose, fields)
    return (data if torch.is_tensor(vertices) else data.cpu().numpy()), log


# ------------------------------------------------------------------------------------ K36
class MeshBVH(NamedTuple("MeshBVH", [("nodes", torch.Tensor), ("boxes", torch.Tensor),
                                     ("order", torch.Tensor), ("vertices", torch.Tensor),
                                     ("triangles", torch.Tensor), ("levels", int),
                                     ("leaf_size", int), ("pad", float)])):
    """The tree K36 casts rays through (``build_mesh_bvh``): ``nodes`` (2^levels - 1, 6) f32, the
    boxes of a complete binary tree stored level by level; ``boxes`` (F,6) f32, the padded box of
    every triangle; ``order`` (F,) int32, the triangles in Morton order, ``leaf_size`` to a leaf;
    and the ``vertices`` (V,3) f32 and ``triangles`` (F,3) int32 it was built from, on the device.
    It is a snapshot: after the vertices move, build another."""

    @property
    def num_triangles(self) -> int:
        return int(self.triangles.shape[0])


MeshHit = NamedTuple("MeshHit", [("triangles", torch.Tensor), ("t", torch.Tensor),
                                 ("u", torch.Tensor), ("v", torch.Tensor)])


def _finite_extent(vertices: torch.Tensor):
    """(lowest corner (3,), longest side, largest |coordinate|) of the finite vertices, on the
    host; one read-back."""
    finite = torch.isfinite(vertices).all(1, keepdim=True)
    high = torch.where(finite, vertices, torch.full_like(vertices, -math.inf)).amax(0)
    low = torch.where(finite, vertices, torch.full_like(vertices, math.inf)).amin(0)
    largest = torch.where(torch.isfinite(vertices), vertices.abs(),
                          torch.zeros_like(vertices)).amax().reshape(1)
    found = torch.cat([low, high, largest]).cpu().numpy()
    return found[0:3], found[3:6], found[6]


def build_mesh_bvh(vertices, triangles, leaf_size: int = 4, pad=None, device=None) -> MeshBVH:
    """The tree over a mesh that ``cast_rays``, ``mesh_spans``, ``render_mesh_rays`` and
    ``RaySampler.clip_to_mesh`` walk (K36a/b, ``csrc/mesh_cast.hip``): the triangles sorted by the
    30-bit Morton code of their box centres (``torch.sort``: plumbing), ``leaf_size`` (1 .. 64) to a
    leaf of an implicit balanced binary tree.  vertices (V,3), triangles (F,3) integers (ids are
    clamped into the vertices, as K22 and K31 do), numpy or tensors.

    ``pad`` >= 0 widens every triangle's box on all sides; None, the default, takes ``2^-16`` times
    the largest finite |coordinate|.  A hit has to lie inside its triangle's padded box, which
    makes the tree exact (a culled node never hides a hit) and discards the garbage ``t`` of
    grazing rays; ``pad`` only has to cover the rounding of ``t`` against the box planes.  A
    triangle with a non-finite coordinate is never hit.

    The result does not depend on the order of the sort or on ``leaf_size``, only the time does.
    Not done: a refit when the vertices move (build again), a surface-area or LBVH build."""
    who = "build_mesh_bvh"
    shape = _shape_of(vertices)
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= _MOST:
        raise ValueError("%s: vertices must be (V,3) with 1 <= V <= (2^31 - 1) / 3, got %s"
                         % (who, shape))
    shape = _shape_of(triangles)
    if len(shape) != 2 or shape[1] != 3 or not 1 <= shape[0] <= _MOST:
        raise ValueError("%s: triangles must be (F,3) with 1 <= F <= (2^31 - 1) / 3, got %s"
                         % (who, shape))
    if isinstance(leaf_size, bool) or int(leaf_size) != leaf_size \
            or not 1 <= leaf_size <= ops.MESH_CAST_MAX_LEAF:
        raise ValueError("%s: leaf_size must be an integer in 1 .. %d, got %r"
                         % (who, ops.MESH_CAST_MAX_LEAF, leaf_size))
    leaf_size = int(leaf_size)
    if pad is not None and not (float(pad) >= 0.0 and math.isfinite(float(pad))):
        raise ValueError("%s: pad must be a finite number >= 0, got %r" % (who, pad))
    _, device, vertices, triangles = _mesh_on(vertices, triangles, device)
    low, high, largest = _finite_extent(vertices)
    if pad is None:
        pad = np.float32(2.0 ** -16) * np.float32(largest)
    pad = float(np.float32(pad))
    extent = np.float32((high - low).max()) if np.isfinite(high - low).all() else np.float32(0.0)
    with np.errstate(all="ignore"):
        scale = np.float32(1024.0) / extent if extent > 0 else np.float32(0.0)
    if not np.isfinite(scale):
        scale = np.float32(0.0)
    corner = low if np.isfinite(low).all() else np.zeros(3, dtype=np.float32)
    boxes, keys = ops.mesh_cast_boxes(vertices, triangles, pad, corner, float(scale))
    number = torch.arange(keys.shape[0], dtype=torch.int64, device=device)
    order = torch.sort((keys.to(torch.int64) << 32) | number).values.bitwise_and_(0xFFFFFFFF) \
        .to(torch.int32)
    nodes = ops.mesh_cast_tree(boxes, order, leaf_size)
    return MeshBVH(nodes, boxes, order, vertices, triangles,
                   ops.mesh_cast_levels(triangles.shape[0], leaf_size), leaf_size, pad)


def _cast_rays_on(who, bvh, starts, directions):
    """-> (whether the rays came as numpy, starts, directions (R,3) f32 on the tree's device)."""
    if not isinstance(bvh, MeshBVH):
        raise ValueError("%s: bvh must be a MeshBVH (build_mesh_bvh), got %s"
                         % (who, type(bvh).__name__))
    for name, value in (("starts", starts), ("directions", directions)):
        shape = _shape_of(value)
        if len(shape) != 2 or shape[1] != 3 or shape[0] < 1:
            raise ValueError("%s: %s must be (R,3) with R >= 1, got %s" % (who, name, shape))
    if _shape_of(starts) != _shape_of(directions):
        raise ValueError("%s: starts %s and directions %s must have one shape"
                         % (who, _shape_of(starts), _shape_of(directions)))
    device = bvh.nodes.device
    return (not torch.is_tensor(starts), _on(starts, "float32", device),
            _on(directions, "float32", device))


def _cast(bvh, starts, directions, t_min, farthest):
    return ops.mesh_cast(bvh.nodes, bvh.boxes, bvh.order, bvh.vertices, bvh.triangles, starts,
                         directions, bvh.leaf_size, float(t_min), farthest)


def cast_rays(bvh: MeshBVH, starts, directions, t_min: float = 0.0,
              which: str = "nearest") -> MeshHit:
    """Per ray ``o + t d`` the triangle of the mesh it hits first after ``t_min`` (K36c), or with
    ``which="farthest"`` last: the mesh counterpart of ``OcTree.first_hit``.  starts, directions
    (R,3), numpy or tensors (numpy in gives numpy out); the directions need not be unit vectors,
    ``t`` is in their units.  -> ``MeshHit``: ``triangles`` (R,) int32, -1 for a miss; ``t`` and the
    barycentric ``u``, ``v`` (R,) float32 of the hit (the point is ``(1 - u - v) a + u b + v c``), 0
    on a miss.  Both sides of a triangle are hit; a ray in a triangle's plane misses it; of two
    triangles hit at the same ``t`` (a shared edge or vertex) the lower id is returned; a NaN or
    infinite ray misses.  The answer is bit for bit that of testing every triangle.  No gradient
    flows through the cast."""
    who = "cast_rays"
    if which not in ("nearest", "farthest"):
        raise ValueError("%s: which must be 'nearest' or 'farthest', got %r" % (who, which))
    as_numpy, starts, directions = _cast_rays_on(who, bvh, starts, directions)
    hit = MeshHit(*_cast(bvh, starts, directions, t_min, which == "farthest"))
    return MeshHit(*[x.cpu().numpy() for x in hit]) if as_numpy else hit


def mesh_spans(bvh: MeshBVH, starts, directions, t_min: float = 0.0, margin: float = 0.0):
    """Per ray the span ``[t_in, t_out]`` between its first and its last hit of the mesh after
    ``t_min`` (two casts of K36c), widened by ``margin`` (in units of ``t``) at both ends but not
    below ``t_min``, and ``hit``: whether it meets the mesh at all.  -> ``(t_in, t_out`` float32,
    ``hit`` bool), each (R,); 0, 0, False for a miss.  The mesh counterpart of ``OcTree.spans``."""
    who = "mesh_spans"
    if not (float(margin) >= 0.0 and math.isfinite(float(margin))):
        raise ValueError("%s: margin must be a finite number >= 0, got %r" % (who, margin))
    as_numpy, starts, directions = _cast_rays_on(who, bvh, starts, directions)
    near, t_near, _, _ = _cast(bvh, starts, directions, t_min, False)
    _, t_far, _, _ = _cast(bvh, starts, directions, t_min, True)
    hit = near >= 0
    zero = torch.zeros_like(t_near)
    t_in = torch.where(hit, torch.clamp_min(t_near - float(margin), float(t_min)), zero)
    t_out = torch.where(hit, t_far + float(margin), zero)
    if as_numpy:
        return t_in.cpu().numpy(), t_out.cpu().numpy(), hit.cpu().numpy()
    return t_in, t_out, hit


def render_mesh_rays(bvh: MeshBVH, starts, directions, colors=None, uvs=None, texture=None,
                     background=(0, 0, 0), t_min: float = 0.0):
    """The mesh as a batch of rays sees it (K36c and K36d) -> ``RenderResult``: ``color`` (R,3) of
    the first hit, ``alpha`` (R,) 1 on a hit and 0 on a miss, ``depth`` (R,) the hit's ``t`` (the
    distance for unit directions).  Exactly one of ``colors`` (V,3), interpolated with the hit's
    barycentric weights, and ``uvs`` (V,2) + ``texture`` (h,w,C) uint8 with row 0 at the top (as
    ``render_mesh`` takes it).  A miss gets ``background``.  numpy in gives numpy out.  There is no
    camera plane: the rays may start inside the mesh or next to it, where ``render_mesh`` reports
    triangles ``clipped``."""
    who = "render_mesh_rays"
    from .utils import RenderResult
    as_numpy, starts, directions = _cast_rays_on(who, bvh, starts, directions)
    if colors is not None and (uvs is not None or texture is not None):
        raise ValueError("%s: give either colors, or uvs and texture, not both" % who)
    if colors is None and (uvs is None or texture is None):
        raise ValueError("%s: give colors, or both uvs and texture" % who)
    num_vertices = bvh.vertices.shape[0]
    for name, value, last in (("colors", colors, 3), ("uvs", uvs, 2)):
        if value is not None and _shape_of(value) != (num_vertices, last):
            raise ValueError("%s: %s must be (V,%d) = (%d,%d), got %s"
                             % (who, name, last, num_vertices, last, _shape_of(value)))
    if texture is not None:
        tex = _shape_of(texture)
        if len(tex) != 3 or tex[2] < 3 or min(tex) < 1:
            raise ValueError("%s: texture must be (H,W,C) with C >= 3, got %s" % (who, tex))
        texture = texture.flip(0) if torch.is_tensor(texture) else np.asarray(texture)[::-1]
    ground = np.asarray(background, dtype=np.float64).reshape(-1)
    if ground.shape != (3,) or not np.isfinite(ground).all():
        raise ValueError("%s: background must be three finite numbers, got %r"
                         % (who, background))
    device = bvh.nodes.device
    hit, t, u, v = _cast(bvh, starts, directions, t_min, False)
    out = RenderResult(*ops.mesh_cast_shade(
        hit, t, u, v, bvh.triangles,
        None if colors is None else _on(colors, "float32", device),
        None if uvs is None else _on(uvs, "float32", device),
        None if texture is None else _on(texture, "uint8", device), ground))
    return out.numpy() if as_numpy else out
