"""Two independent statements of what K31 (csrc/mesh_raster.hip) draws.

``raster`` restates the contract of include/ffn_hip.h operation by operation: every float value is a
numpy float32 and every operation one rounded f32 operation in the header's order, the edge
functions and the pixel boxes are int64.  It has to give the kernel's ids, colours and depths bit
for bit.

``raycast64`` is the truth the restatement itself is held to: Moeller-Trumbore in float64 over all
triangles for every pixel's ray, straight from the camera's intrinsics and pose.  It shares no code
with ``raster`` -- no projection matrix, no fixed point, no boxes.  ``undecided`` says where the
two may differ for a reason: a pixel centre within 1/128 pixel of a float64-projected edge (the
snap to 1/256 pixel may move the edge across it), or two nearest hits within 1e-4 relative depth.

``scene`` and ``camera`` make the seeded test scenes.  Nothing here needs a GPU.
"""

import numpy as np

F32 = np.float32
EMPTY = np.uint64(0xFFFFFFFFFFFFFFFF)
DRAWN, BEHIND, CLIPPED, DEGENERATE, OFF_IMAGE = range(5)
GUARD = F32(16384.0)


# ------------------------------------------------------------------------------- restatement
def project(proj, points):
    """K23's projection of (N,3) f32 points -> x, y, w (N,) f32, every product and sum rounded."""
    p = np.asarray(proj, dtype=F32).reshape(3, 4)
    v = np.asarray(points, dtype=F32)

    def row(r):
        return ((p[r, 0] * v[:, 0] + p[r, 1] * v[:, 1]) + p[r, 2] * v[:, 2]) + p[r, 3]

    return row(0), row(1), row(2)


def setup(vertices, triangles, proj, width, height):
    """K31a -> dict of X, Y (F,3) int64, w (F,3) f32, box (F,4) int64 [x0, y0, x1, y1], status (F,)
    uint8 and counts (F,) int64."""
    vertices = np.asarray(vertices, dtype=F32)
    ids = np.clip(np.asarray(triangles, dtype=np.int64), 0, len(vertices) - 1)
    with np.errstate(all="ignore"):
        x, y, w = project(proj, vertices[ids.reshape(-1)])
        sx, sy = x / w, y / w
        behind = (w <= 0).reshape(-1, 3).all(1)
        bad = (~(w > 0)) | ~(np.abs(sx) <= GUARD) | ~(np.abs(sy) <= GUARD)
        clipped = bad.reshape(-1, 3).any(1)
        safe = ~np.repeat(behind | clipped, 3)
        fx = np.zeros(len(sx), dtype=np.int64)
        fy = np.zeros(len(sx), dtype=np.int64)
        fx[safe] = np.rint(sx[safe] * F32(256.0)).astype(np.int64)
        fy[safe] = np.rint(sy[safe] * F32(256.0)).astype(np.int64)
    fx, fy, w = fx.reshape(-1, 3), fy.reshape(-1, 3), w.reshape(-1, 3)
    area = (fx[:, 1] - fx[:, 0]) * (fy[:, 2] - fy[:, 0]) - (fy[:, 1] - fy[:, 0]) * (fx[:, 2] - fx[:, 0])
    # numpy's // and >> on int64 are floor divisions
    x0 = np.maximum(0, -((-fx.min(1)) // 256))
    x1 = np.minimum(width - 1, fx.max(1) // 256)
    y0 = np.maximum(0, -((-fy.min(1)) // 256))
    y1 = np.minimum(height - 1, fy.max(1) // 256)
    status = np.full(len(ids), DRAWN, dtype=np.uint8)
    empty = (x1 < x0) | (y1 < y0)
    status[empty] = OFF_IMAGE
    status[area == 0] = DEGENERATE
    status[clipped] = CLIPPED
    status[behind] = BEHIND
    drawn = status == DRAWN
    box = np.where(drawn[:, None], np.stack([x0, y0, x1, y1], 1), np.array([0, 0, -1, -1]))
    counts = (box[:, 2] - box[:, 0] + 1) * (box[:, 3] - box[:, 1] + 1)
    return dict(X=fx, Y=fy, w=w, box=box, status=status, counts=counts, ids=ids)


def terms(fx, fy, w, px, py):
    """The header's E_i, l_i, q_i and depth_w for triangles (.., 3) and pixels (..) that broadcast
    -> covered, q (3 arrays), depth_w."""
    px, py = np.asarray(px, dtype=np.int64), np.asarray(py, dtype=np.int64)
    qx, qy = 256 * px, 256 * py
    area = ((fx[..., 1] - fx[..., 0]) * (fy[..., 2] - fy[..., 0])
            - (fy[..., 1] - fy[..., 0]) * (fx[..., 2] - fx[..., 0]))
    sign = np.where(area < 0, -1, 1)
    edges = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        edges.append(sign * ((fx[..., k] - fx[..., j]) * (qy - fy[..., j])
                             - (fy[..., k] - fy[..., j]) * (qx - fx[..., j])))
    covered = (edges[0] >= 0) & (edges[1] >= 0) & (edges[2] >= 0)
    with np.errstate(all="ignore"):
        size = np.abs(area).astype(F32)
        q = [(edges[i].astype(F32) / size) / w[..., i] for i in range(3)]
        inv_w = (q[0] + q[1]) + q[2]
        depth_w = F32(1.0) / inv_w
    return covered, q, depth_w


def draw(state, width, height):
    """K31b over every drawn triangle -> zbuf (H W,) uint64, all ones where nothing was drawn."""
    zbuf = np.full(width * height, EMPTY, dtype=np.uint64)
    for f in np.flatnonzero(state["status"] == DRAWN):
        x0, y0, x1, y1 = state["box"][f]
        py, px = np.meshgrid(np.arange(y0, y1 + 1), np.arange(x0, x1 + 1), indexing="ij")
        covered, _, depth_w = terms(state["X"][f], state["Y"][f], state["w"][f], px, py)
        keep = covered & np.isfinite(depth_w) & (depth_w > 0)
        keys = (depth_w.view(np.uint32).astype(np.uint64) << np.uint64(32)) | np.uint64(f)
        pixels = (py * width + px)[keep]
        zbuf[pixels] = np.minimum(zbuf[pixels], keys[keep])
    return zbuf


def texture_lookup(u, v, texture):
    """K22's bilinear lookup (f32, the weights formed before the indices are clamped), / 255."""
    height, width = texture.shape[:2]
    with np.errstate(all="ignore"):
        col, row = u * F32(width), v * F32(height)
        fj, fi = np.floor(col), np.floor(row)
        dj, di = col - fj, row - fi

        def clamp(index, last):
            return np.fmin(np.fmax(index, F32(0.0)), F32(last)).astype(np.int64)

        j0, j1 = clamp(fj, width - 1), clamp(fj + F32(1.0), width - 1)
        i0, i1 = clamp(fi, height - 1), clamp(fi + F32(1.0), height - 1)
        one = F32(1.0)
        w00, w01, w10, w11 = (one - di) * (one - dj), (one - di) * dj, di * (one - dj), di * dj
        out = np.empty(u.shape + (3,), dtype=F32)
        for ch in range(3):
            t = texture[..., ch].astype(F32)
            out[..., ch] = (((w00 * t[i0, j0] + w01 * t[i0, j1]) + w10 * t[i1, j0])
                            + w11 * t[i1, j1]) / F32(255.0)
    return out


def resolve(state, zbuf, vertices, eye, width, height, colors=None, uvs=None, texture=None,
            background=(0, 0, 0)):
    """K31c -> color (H W,3), alpha, depth (H W,) f32, ids (H W,) int32."""
    vertices = np.asarray(vertices, dtype=F32)
    eye = np.asarray(eye, dtype=F32)
    n = width * height
    color = np.tile(np.asarray(background, dtype=F32), (n, 1))
    alpha, depth = np.zeros(n, dtype=F32), np.zeros(n, dtype=F32)
    ids = np.full(n, -1, dtype=np.int32)
    hit = np.flatnonzero(zbuf != EMPTY)
    if len(hit) == 0:
        return color, alpha, depth, ids
    f = (zbuf[hit] & np.uint64(0xFFFFFFFF)).astype(np.int64)
    _, q, depth_w = terms(state["X"][f], state["Y"][f], state["w"][f], hit % width, hit // width)
    b = [q[i] * depth_w for i in range(3)]
    corner = state["ids"][f]

    def blend(values):
        values = np.asarray(values, dtype=F32)
        return np.stack([(values[corner[:, 0], j] * b[0] + values[corner[:, 1], j] * b[1])
                         + values[corner[:, 2], j] * b[2] for j in range(values.shape[1])], -1)

    with np.errstate(all="ignore"):
        d = blend(vertices) - eye
        depth[hit] = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        if colors is not None:
            color[hit] = blend(colors)
        else:
            uv = blend(uvs)
            color[hit] = texture_lookup(uv[:, 0], uv[:, 1], np.asarray(texture))
    alpha[hit] = 1.0
    ids[hit] = f
    return color, alpha, depth, ids


def raster(vertices, triangles, proj, eye, width, height, colors=None, uvs=None, texture=None,
           background=(0, 0, 0)):
    """K31a-c -> (color, alpha, depth, ids, status, counts).  ``texture`` with the row index growing
    with v, as the kernel takes it."""
    state = setup(vertices, triangles, proj, width, height)
    zbuf = draw(state, width, height)
    return resolve(state, zbuf, vertices, eye, width, height, colors, uvs, texture,
                   background) + (state["status"], state["counts"])


# ------------------------------------------------------------------------------- float64 truth
def raycast64(vertices, triangles, intrinsics, extrinsics, width, height):
    """Moeller-Trumbore in float64, every triangle against every pixel's ray, both sides ->
    (winner (H W,) int64 or -1, nearest (H W,), second (H W,)): the depths along the camera's axis of
    the two nearest hits, inf where there is none."""
    v = np.asarray(vertices, dtype=np.float64)
    tri = np.asarray(triangles, dtype=np.int64)
    k_inv = np.linalg.inv(np.asarray(intrinsics, dtype=np.float64)[:3, :3])
    pose = np.asarray(extrinsics, dtype=np.float64)
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    pixel = np.stack([px.reshape(-1), py.reshape(-1), np.ones(width * height)], 0).astype(np.float64)
    direction = (pose[:3, :3] @ (k_inv @ pixel)).T              # camera-axis component is 1
    origin = pose[:3, 3]
    hits = np.full((width * height, len(tri)), np.inf)
    for f, (a, b, c) in enumerate(v[tri]):
        e1, e2 = b - a, c - a
        p = np.cross(direction, e2)
        det = p @ e1
        with np.errstate(all="ignore"):
            inv = 1.0 / det
            s = origin - a
            bu = (p @ s) * inv
            qv = np.cross(s, e1)
            bv = (direction @ qv) * inv
            t = (qv @ e2) * inv
        inside = (det != 0) & (bu >= 0) & (bv >= 0) & (bu + bv <= 1) & (t > 0)
        hits[inside, f] = t[inside]
    order = np.argsort(hits, axis=1, kind="stable")
    rows = np.arange(len(hits))
    nearest = hits[rows, order[:, 0]]
    second = hits[rows, order[:, 1]] if len(tri) > 1 else np.full(len(hits), np.inf)
    winner = np.where(np.isfinite(nearest), order[:, 0], -1)
    return winner, nearest, second


def plane_distance64(vertices, triangles, winner, intrinsics, extrinsics, px, py):
    """The distance from the eye at which the ray through the screen point (px, py) -- any real
    numbers -- meets the PLANE of triangle ``winner`` (arrays of one length), in float64."""
    v = np.asarray(vertices, dtype=np.float64)[np.asarray(triangles, dtype=np.int64)[winner]]
    pose = np.asarray(extrinsics, dtype=np.float64)
    k_inv = np.linalg.inv(np.asarray(intrinsics, dtype=np.float64)[:3, :3])
    pixel = np.stack([px, py, np.ones_like(px)], 0).astype(np.float64)
    direction = (pose[:3, :3] @ (k_inv @ pixel)).T
    normal = np.cross(v[:, 1] - v[:, 0], v[:, 2] - v[:, 0])
    t = ((v[:, 0] - pose[:3, 3]) * normal).sum(1) / (direction * normal).sum(1)
    return t * np.linalg.norm(direction, axis=1)


def edge_distance64(vertices, triangles, intrinsics, extrinsics, width, height):
    """The distance, in pixels, from every pixel centre to the nearest float64-projected triangle
    edge (a segment) -> (H W,)."""
    v = np.asarray(vertices, dtype=np.float64)
    tri = np.asarray(triangles, dtype=np.int64)
    pose = np.asarray(extrinsics, dtype=np.float64)
    cam = (v - pose[:3, 3]) @ pose[:3, :3]                       # R^T (v - c)
    homog = cam @ np.asarray(intrinsics, dtype=np.float64)[:3, :3].T
    screen = homog[:, :2] / homog[:, 2:3]
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    centre = np.stack([px.reshape(-1), py.reshape(-1)], -1).astype(np.float64)
    best = np.full(len(centre), np.inf)
    for corners in tri:
        for i in range(3):
            a, b = screen[corners[i]], screen[corners[(i + 1) % 3]]
            ab = b - a
            length = ab @ ab
            along = np.clip(((centre - a) @ ab) / length, 0, 1) if length > 0 else np.zeros(len(centre))
            best = np.minimum(best, np.linalg.norm(centre - (a + along[:, None] * ab), axis=1))
    return best


def undecided(vertices, triangles, intrinsics, extrinsics, width, height, nearest, second):
    """Where the restatement and the truth may differ for a reason (see the module docstring)."""
    near_edge = edge_distance64(vertices, triangles, intrinsics, extrinsics, width, height) < 1 / 128
    with np.errstate(all="ignore"):
        tied = np.isfinite(second) & (second - nearest <= 1e-4 * nearest)
    return near_edge | tied


# ------------------------------------------------------------------------------- scenes
def camera(width, height, distance=3.0, fov_y_degrees=40.0, yaw=0.3, pitch=-0.2, focal=None):
    """A pinhole ``CameraInfo`` looking at the origin from ``distance`` away; the principal point
    is the image's centre in the project's convention, ((W-1)/2, (H-1)/2).  ``focal`` in pixels
    replaces the one ``fov_y_degrees`` gives."""
    from fourier_feature_nets_amd.cameras import CameraInfo, Resolution
    if focal is None:
        focal = 0.5 * height / np.tan(np.radians(0.5 * fov_y_degrees))
    intrinsics = np.array([[focal, 0, 0.5 * (width - 1)], [0, focal, 0.5 * (height - 1)], [0, 0, 1]],
                          dtype=np.float32)
    cy, sy, cp, sp = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch)
    rotation = (np.array([[cy, 0, sy], [0, 1, 0], [-sy, 0, cy]])
                @ np.array([[1, 0, 0], [0, cp, -sp], [0, sp, cp]]))
    pose = np.eye(4)
    pose[:3, :3] = rotation
    pose[:3, 3] = rotation @ np.array([0.0, 0.0, -distance])
    return CameraInfo.create("test", Resolution(width, height), intrinsics, pose.astype(np.float32))


def scene(seed, count, half_extent=0.5, spread=0.6):
    """``count`` random triangles: centres uniform in +-spread, corners within +-half_extent of
    them -> (vertices (3F,3) f32, triangles (F,3) int32, colors (3F,3) f32, uvs (3F,2) f32)."""
    rng = np.random.default_rng(seed)
    centres = rng.uniform(-spread, spread, (count, 1, 3))
    vertices = (centres + rng.uniform(-half_extent, half_extent, (count, 3, 3))).reshape(-1, 3)
    triangles = np.arange(3 * count, dtype=np.int32).reshape(-1, 3)
    colors = rng.uniform(0, 1, (3 * count, 3))
    uvs = rng.uniform(-0.5, 1.5, (3 * count, 2))
    return (vertices.astype(np.float32), triangles, colors.astype(np.float32),
            uvs.astype(np.float32))


def texture(seed, height, width, channels):
    return np.random.default_rng(seed).integers(0, 256, (height, width, channels), dtype=np.uint8)


# sx = x / z, sy = y / z, w = z: at z = 1 a vertex (x, y, 1) lies at the pixel coordinates (x, y),
# exactly whenever 256 x and 256 y are integers
PIXEL_PROJ = np.array([[1, 0, 0, 0], [0, 1, 0, 0], [0, 0, 1, 0]], dtype=np.float32)
ORIGIN = np.zeros(3, dtype=np.float32)


def flat(points, z=1.0):
    """Screen points [(x, y), ...] -> (N,3) f32 vertices that PIXEL_PROJ puts there, at depth z."""
    points = np.asarray(points, dtype=np.float64)
    return np.concatenate([points * z, np.full((len(points), 1), z)], 1).astype(np.float32)


def grey(vertices, seed=0):
    """Per-vertex colours for a scene that has none of its own."""
    return np.random.default_rng(seed).uniform(0, 1, (len(vertices), 3)).astype(np.float32)


def quad_scene():
    """The rectangle [2, 10] x [3, 9] as two triangles that share the diagonal (2,3)-(10,9)."""
    return flat([(2, 3), (10, 3), (10, 9), (2, 9)]), np.array([[0, 1, 2], [0, 2, 3]], np.int32)


# a sliver along y - x in [8.1, 8.25]: its box holds 4 x 5 pixels and it contains no centre
SLIVER = flat([(14.25, 22.5), (18.75, 27.0), (18.85, 26.95)])


def placement_scene(width, height):
    """One triangle per placement the contract names -> (vertices, triangles, expected status).
    Under PIXEL_PROJ; the image is ``width`` x ``height``."""
    w, h = float(width - 1), float(height - 1)
    groups = [
        (flat([(-6.25, 4.5), (5.5, 2.25), (3.0, 9.75)]), DRAWN),                  # left border
        (flat([(w - 4.5, 3.25), (w + 7.75, 5.0), (w - 2.0, 11.5)]), DRAWN),       # right border
        (flat([(8.5, -5.5), (15.25, 3.75), (11.0, 4.0)], 2.0), DRAWN),            # top border
        (flat([(20.5, h - 3.0), (27.0, h - 1.5), (24.25, h + 9.0)], 0.5), DRAWN),  # bottom border
        (flat([(-30, -30), (-20, -30), (-25, -12)]), OFF_IMAGE),                  # wholly off
        (flat([(w + 1.5, 2), (w + 9, 2), (w + 4, 7)]), OFF_IMAGE),
        (flat([(3, 3), (9, 4), (5, 8)], -1.0), BEHIND),                           # all w < 0
        (np.array([[1, 1, 1], [5, 2, 1], [3, 6, -0.5]], np.float32), CLIPPED),    # straddles w = 0
        (np.array([[1, 1, 1], [5, 2, 0], [3, 6, 1]], np.float32), CLIPPED),       # a vertex on w = 0
        (flat([(3, 3), (20000, 4), (5, 8)]), CLIPPED),                            # outside the band
        (np.array([[np.nan, 1, 1], [5, 2, 1], [3, 6, 1]], np.float32), CLIPPED),
        (flat([(12.001, 7.001), (12.0015, 7.0012), (12.0005, 7.0018)]), DEGENERATE),  # snaps to a point
        (flat([(4, 4), (8, 8), (12, 12)]), DEGENERATE),                           # collinear
        (flat([(30, 10), (38.5, 12.25), (33.75, 17)]), DRAWN),                    # a vertex on a centre
        (flat([(40.5, 20.5), (48.5, 20.5), (48.5, 28.5)], 3.0), DRAWN),           # tied depths: the
        (flat([(40.5, 20.5), (48.5, 20.5), (48.5, 28.5)], 3.0), DRAWN),           # same triangle twice
        (SLIVER, DRAWN),
    ]
    vertices = np.concatenate([g for g, _ in groups])
    triangles = np.arange(len(vertices), dtype=np.int32).reshape(-1, 3)
    return vertices, triangles, np.array([s for _, s in groups], dtype=np.uint8)
