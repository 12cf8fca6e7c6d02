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


def load_obj(path: str, texture_path: Optional[str] = None) -> Mesh:
    """Reads the ``v``, ``vt`` and ``f`` records of a Wavefront OBJ -> ``(vertices, triangles, uvs,
    texture)``.  A face corner is ``v``, ``v/vt``, ``v/vt/vn`` or ``v//vn``, 1-based or negative
    (counted back from the records read so far); polygons become triangle fans; every distinct
    ``(v, vt)`` pair becomes one vertex, in the order the faces first use them.  The texture is
    ``texture_path`` or else the ``map_Kd`` of the ``mtllib`` (read with PIL, row 0 at the top).
    A file with no ``vt``, or with no texture, gives a 1x1 white texture and zero UVs.  Normals,
    vertex colours, groups and all but the first material are ignored."""
    positions, coords, corners, library = [], [], [], None

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
    return vertices, np.asarray(index, dtype=np.int32).reshape(-1, 3), uvs, texture
