"""numpy-f32 restatement of K22 (csrc/mesh.hip), written from the arithmetic the kernel's header
comment spells out: every line below is one rounded float32 operation on whole arrays, in the
kernel's order.  The tests compare the kernel against it bit for bit."""

import numpy as np

F32 = np.float32
ROUNDS = 16


def sample_numbers(counts):
    """Per sample: its triangle ``f`` and its number ``n = k + 1`` inside it (int64 arrays)."""
    counts = np.asarray(counts, dtype=np.int64)
    triangle = np.repeat(np.arange(len(counts)), counts)
    first = np.concatenate([[0], np.cumsum(counts)])[:-1]
    number = np.arange(counts.sum()) - first[triangle] + 1
    return triangle, number


def triangle_points(number):
    """Basu-Owen points of the sample numbers -> (N,2) float32 ``p = ((A + B) + C) / 3``."""
    number = np.asarray(number, dtype=np.int64)
    a = np.zeros((len(number), 2), F32)
    b = np.zeros_like(a)
    c = np.zeros_like(a)
    a[:, 0] = 1
    b[:, 1] = 1
    half = F32(0.5)
    for i in range(ROUNDS):
        d = ((number >> (2 * i)) & 3)[:, None]
        ab, ac, bc = (a + b) * half, (a + c) * half, (b + c) * half
        a, b, c = (np.select([d == 0, d == 1, d == 2], [bc, a, ab], ac),
                   np.select([d == 0, d == 1, d == 2], [ac, ab, b], bc),
                   np.select([d == 0, d == 1, d == 2], [ab, ac, bc], c))
    p = ((a + b) + c) / F32(3)
    assert p.dtype == F32
    return p


def barycentric(p):
    """(N,3) float32 weights ``(p.x, p.y, 1 - (p.x + p.y))``."""
    return np.stack([p[:, 0], p[:, 1], F32(1) - (p[:, 0] + p[:, 1])], -1)


def interpolate(values, corners, weights):
    """``(x0 b0 + x1 b1) + x2 b2`` per component; values (V,D) f32, corners (N,3) vertex ids."""
    x0, x1, x2 = values[corners[:, 0]], values[corners[:, 1]], values[corners[:, 2]]
    b0, b1, b2 = weights[:, 0:1], weights[:, 1:2], weights[:, 2:3]
    out = (x0 * b0 + x1 * b1) + x2 * b2
    assert out.dtype == F32
    return out


def bilinear_colors(texture, sample_uvs):
    """Texture colours of (N,2) float32 UVs, channels 0..2, over 255."""
    height, width = texture.shape[:2]
    col = sample_uvs[:, 0] * F32(width)
    row = sample_uvs[:, 1] * F32(height)
    fj, fi = np.floor(col), np.floor(row)
    dj, di = (col - fj)[:, None], (row - fi)[:, None]

    def clamp(index, last):           # clamped as f32, then converted: NaN -> 0
        with np.errstate(invalid="ignore"):
            index = np.where(np.isnan(index), F32(0), index)
            return np.minimum(np.maximum(index, F32(0)), F32(last)).astype(np.int64)

    j0, j1 = clamp(fj, width - 1), clamp(fj + F32(1), width - 1)
    i0, i1 = clamp(fi, height - 1), clamp(fi + F32(1), height - 1)
    one = F32(1)
    texels = texture[..., :3].astype(F32)
    v00 = ((one - di) * (one - dj)) * texels[i0, j0]
    v01 = ((one - di) * dj) * texels[i0, j1]
    v10 = (di * (one - dj)) * texels[i1, j0]
    v11 = (di * dj) * texels[i1, j1]
    out = (((v00 + v01) + v10) + v11) / F32(255)
    assert out.dtype == F32
    return out


def mesh_sample(vertices, triangles, uvs, counts, texture):
    """-> positions (N,3), colors (N,3), sample_uvs (N,2), float32: what K22 writes for these
    vertices (V,3) f32, triangles (F,3), uvs (V,2) f32, per-triangle counts (F,) and texture
    (H,W,C) uint8 (row index growing with v)."""
    vertices = np.ascontiguousarray(vertices, dtype=F32)
    uvs = np.ascontiguousarray(uvs, dtype=F32)
    triangles = np.asarray(triangles, dtype=np.int64)
    triangle, number = sample_numbers(counts)
    weights = barycentric(triangle_points(number))
    corners = triangles[triangle]
    positions = interpolate(vertices, corners, weights)
    sample_uvs = interpolate(uvs, corners, weights)
    return positions, bilinear_colors(np.asarray(texture), sample_uvs), sample_uvs
