"""K36 (csrc/mesh_cast.hip) restated in numpy: the contract of include/ffn_hip.h operation by
operation, every float value a numpy float32 and every operation one rounded f32 operation in the
header's order.  It has to give the kernels' boxes, keys, nodes, hits and colours bit for bit.

``brute`` tests every triangle against every ray; ``cast`` walks the tree as K36c does (all rays at
once, each with its own ``(level, index)``) and counts the nodes visited and triangles tested.  The
contract makes the two equal bit for bit, whatever ``order`` and ``leaf_size``; the CPU tests hold
them to that, and ``brute`` to the float64 ``raycast64`` of tests/mesh_raster_reference.py.

Nothing here needs a GPU.
"""

import numpy as np

from tests.mesh_raster_reference import texture_lookup

F32 = np.float32
INF = F32(np.inf)
EMPTY_KEY = 1 << 30
PAD_SCALE = F32(2.0 ** -16)


def _f32(x):
    return np.ascontiguousarray(np.asarray(x, dtype=F32))


def dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]


def cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1],
                     a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1)


def corners(vertices, triangles):
    """(F,3,3) f32: the vertices of every triangle, ids clamped into the vertices."""
    vertices = _f32(vertices)
    ids = np.clip(np.asarray(triangles, dtype=np.int64), 0, len(vertices) - 1)
    return vertices[ids]


# ------------------------------------------------------------------------------- the host's part
def default_pad(vertices):
    """2^-16 times the largest finite |coordinate|, in f32 (0 when there is none)."""
    v = np.abs(_f32(vertices))
    v = v[np.isfinite(v)]
    return F32(0.0) if v.size == 0 else F32(PAD_SCALE * v.max())


def grid_of(vertices):
    """-> (grid_lo (3,) f32, grid_scale f32): the corner of the finite vertices' box and 1024 over
    its longest side (0 for a box without extent)."""
    v = _f32(vertices)
    v = v[np.isfinite(v).all(1)]
    if len(v) == 0:
        return np.zeros(3, dtype=F32), F32(0.0)
    lo, hi = v.min(0), v.max(0)
    extent = F32((hi - lo).max())
    with np.errstate(all="ignore"):
        scale = F32(1024.0) / extent if extent > 0 else F32(0.0)
    return lo, (scale if np.isfinite(scale) else F32(0.0))


def levels_of(num_triangles, leaf_size):
    levels = 1
    while (leaf_size << (levels - 1)) < num_triangles:
        levels += 1
    return levels


def order_of(keys):
    """The sort of key << 32 | f -> (F,) int32."""
    keys = np.asarray(keys, dtype=np.int64)
    return np.argsort((keys << 32) | np.arange(len(keys), dtype=np.int64),
                      kind="stable").astype(np.int32)


# ------------------------------------------------------------------------------- K36a
def _spread10(x):
    x = x.astype(np.uint32)
    x = (x | (x << np.uint32(16))) & np.uint32(0x030000FF)
    x = (x | (x << np.uint32(8))) & np.uint32(0x0300F00F)
    x = (x | (x << np.uint32(4))) & np.uint32(0x030C30C3)
    x = (x | (x << np.uint32(2))) & np.uint32(0x09249249)
    return x


def boxes_keys(vertices, triangles, pad, grid_lo, grid_scale):
    """K36a -> (boxes (F,6) f32, keys (F,) int32)."""
    tri = corners(vertices, triangles)
    pad, grid_lo, grid_scale = F32(pad), _f32(grid_lo), F32(grid_scale)
    finite = np.isfinite(tri).all((1, 2))
    with np.errstate(all="ignore"):
        lo = np.fmin(np.fmin(tri[:, 0], tri[:, 1]), tri[:, 2]) - pad
        hi = np.fmax(np.fmax(tri[:, 0], tri[:, 1]), tri[:, 2]) + pad
        lo[~finite], hi[~finite] = INF, -INF
        centre = (lo + hi) * F32(0.5)
        cell = (centre - grid_lo) * grid_scale
        q = np.fmin(np.fmax(cell, F32(0.0)), F32(1023.0)).astype(np.int64)
    key = _spread10(q[:, 0]) | (_spread10(q[:, 1]) << np.uint32(1)) | (_spread10(q[:, 2]) << np.uint32(2))
    keys = np.where(finite, key.astype(np.int64), EMPTY_KEY).astype(np.int32)
    return np.concatenate([lo, hi], 1).astype(F32), keys


# ------------------------------------------------------------------------------- K36b
def tree(boxes, order, leaf_size):
    """K36b -> (nodes (2^levels - 1, 6) f32, levels)."""
    boxes = _f32(boxes)
    num = len(boxes)
    order = np.clip(np.asarray(order, dtype=np.int64), 0, num - 1)
    levels = levels_of(num, leaf_size)
    nodes = np.empty(((1 << levels) - 1, 6), dtype=F32)
    leaves = 1 << (levels - 1)
    lo = np.full((leaves, 3), INF, dtype=F32)
    hi = np.full((leaves, 3), -INF, dtype=F32)
    for slot in range(leaf_size):
        p = np.arange(leaves, dtype=np.int64) * leaf_size + slot
        live = p < num
        f = order[p[live]]
        lo[live] = np.fmin(lo[live], boxes[f, :3])
        hi[live] = np.fmax(hi[live], boxes[f, 3:])
    for level in range(levels - 1, -1, -1):
        first = (1 << level) - 1
        nodes[first:first + (1 << level)] = np.concatenate([lo, hi], 1)
        lo, hi = np.fmin(lo[0::2], lo[1::2]), np.fmax(hi[0::2], hi[1::2])
    return nodes, levels


def build(vertices, triangles, leaf_size=4, pad=None, order=None):
    """What ``mesh.build_mesh_bvh`` makes -> dict(nodes, boxes, order, keys, levels, leaf_size,
    pad).  ``order`` replaces the Morton order (any permutation gives the same hits)."""
    pad = default_pad(vertices) if pad is None else F32(pad)
    grid_lo, grid_scale = grid_of(vertices)
    boxes, keys = boxes_keys(vertices, triangles, pad, grid_lo, grid_scale)
    order = order_of(keys) if order is None else np.asarray(order, dtype=np.int32)
    nodes, levels = tree(boxes, order, leaf_size)
    return dict(nodes=nodes, boxes=boxes, order=order, keys=keys, levels=levels,
                leaf_size=leaf_size, pad=pad, grid_lo=grid_lo, grid_scale=grid_scale)


# ------------------------------------------------------------------------------- the two tests
def slab(box, o, d):
    """The slab test of boxes (..,6) and rays (..,3) that broadcast -> (tn, tf, the box is not empty
    and tn <= tf)."""
    with np.errstate(all="ignore"):
        inv = F32(1.0) / d
        t0 = (box[..., :3] - o) * inv
        t1 = (box[..., 3:] - o) * inv
        near, far = np.fmin(t0, t1), np.fmax(t0, t1)
        tn = np.fmax(np.fmax(near[..., 0], near[..., 1]), near[..., 2])
        tf = np.fmin(np.fmin(far[..., 0], far[..., 1]), far[..., 2])
        return tn, tf, (box[..., 0] <= box[..., 3]) & (tn <= tf)


def moller_trumbore(tri, o, d):
    """Triangles (..,3,3) and rays (..,3) that broadcast -> det, u, v, t."""
    with np.errstate(all="ignore"):
        a = tri[..., 0, :]
        e1, e2 = tri[..., 1, :] - a, tri[..., 2, :] - a
        p = cross(d, e2)
        det = dot(p, e1)
        k = F32(1.0) / det
        s = o - a
        u = dot(p, s) * k
        q = cross(s, e1)
        v = dot(d, q) * k
        t = dot(q, e2) * k
    return det, u, v, t


def hits(tri, box, o, d, t_min, with_box=True):
    """The hit predicate of the contract -> (hit, t, u, v); ``with_box=False`` leaves the padded-box
    clause out (the CPU tests count what it rejects)."""
    det, u, v, t = moller_trumbore(tri, o, d)
    with np.errstate(all="ignore"):
        inside = ((det != 0) & (u >= 0) & (v >= 0) & (u + v <= F32(1.0)) & np.isfinite(t)
                  & (t > F32(t_min)))
        if with_box:
            tn, tf, ok = slab(box, o, d)
            inside &= ok & (tn <= t) & (t <= tf)
    return inside, t, u, v


def _result(num):
    return (np.full(num, -1, dtype=np.int32), np.zeros(num, dtype=F32), np.zeros(num, dtype=F32),
            np.zeros(num, dtype=F32))


def _better(t, f, best_t, best_f, farthest):
    return ((t > best_t) if farthest else (t < best_t)) | ((t == best_t) & (f < best_f))


def brute(vertices, triangles, pad, starts, directions, t_min=0.0, farthest=False, with_box=True):
    """Every triangle against every ray -> (hit (R,) int32, t, u, v (R,) f32)."""
    tri = corners(vertices, triangles)
    grid_lo, grid_scale = grid_of(vertices)
    box, _ = boxes_keys(vertices, triangles, pad, grid_lo, grid_scale)
    o, d = _f32(starts), _f32(directions)
    best_f, best_t, best_u, best_v = _result(len(o))
    best_t[:] = -INF if farthest else INF
    for f in range(len(tri)):
        inside, t, u, v = hits(tri[f], box[f], o, d, t_min, with_box)
        take = inside & _better(t, f, best_t, best_f, farthest)
        best_f[take], best_t[take], best_u[take], best_v[take] = f, t[take], u[take], v[take]
    best_t[best_f < 0] = 0
    return best_f, best_t, best_u, best_v


def cast(bvh, vertices, triangles, starts, directions, t_min=0.0, farthest=False, counts=False):
    """K36c's walk for all rays at once -> (hit, t, u, v), with ``counts`` also the nodes visited
    and the triangles tested per ray (a triangle whose own box fails the slab test counts)."""
    tri = corners(vertices, triangles)
    nodes, box, leaf_size, levels = bvh["nodes"], bvh["boxes"], bvh["leaf_size"], bvh["levels"]
    num = len(tri)
    order = np.clip(np.asarray(bvh["order"], dtype=np.int64), 0, num - 1)
    o, d = _f32(starts), _f32(directions)
    rays = len(o)
    best_f, best_t, best_u, best_v = _result(rays)
    best_t[:] = -INF if farthest else INF
    level = np.zeros(rays, dtype=np.int64)
    index = np.zeros(rays, dtype=np.int64)
    visits = np.zeros(rays, dtype=np.int64)
    tests = np.zeros(rays, dtype=np.int64)
    live = np.arange(rays)
    t_min = F32(t_min)
    for _ in range((1 << levels) - 1):
        if len(live) == 0:
            break
        lv, ix = level[live], index[live]
        visits[live] += 1
        tn, tf, ok = slab(nodes[(1 << lv) - 1 + ix], o[live], d[live])
        with np.errstate(all="ignore"):
            enter = ok & (tf > t_min) & ((tf >= best_t[live]) if farthest else (tn <= best_t[live]))
        down = enter & (lv < levels - 1)
        at_leaf = live[enter & ~down]
        for slot in range(leaf_size):
            p = index[at_leaf] * leaf_size + slot
            rows = at_leaf[p < num]
            f = order[p[p < num]]
            tests[rows] += 1
            inside, t, u, v = hits(tri[f], box[f], o[rows], d[rows], t_min)
            take = inside & _better(t, f, best_t[rows], best_f[rows], farthest)
            rows, f = rows[take], f[take]
            best_f[rows], best_t[rows], best_u[rows], best_v[rows] = f, t[take], u[take], v[take]
        level[live[down]] += 1
        index[live[down]] <<= 1
        move = live[~down]
        index[move] += 1
        done = index[move] == (1 << level[move])
        move = move[~done]
        while len(move):            # strip the trailing zero bits, one level up per bit
            even = (index[move] & 1) == 0
            move = move[even]
            index[move] >>= 1
            level[move] -= 1
        gone = np.zeros(rays, dtype=bool)
        gone[live[~down][done]] = True
        live = live[~gone[live]]
    assert len(live) == 0, "the walk did not end within its trip bound"
    best_t[best_f < 0] = 0
    out = (best_f, best_t, best_u, best_v)
    return out + (visits, tests) if counts else out


# ------------------------------------------------------------------------------- K36d
def shade(hit, t, u, v, triangles, colors=None, uvs=None, texture=None, background=(0, 0, 0)):
    """K36d -> (color (R,3), alpha (R,), depth (R,)) f32; ``texture`` with the row index growing
    with v, as the kernel takes it."""
    triangles = np.asarray(triangles, dtype=np.int64)
    values = _f32(colors if colors is not None else uvs)
    ids = np.clip(triangles, 0, len(values) - 1)
    hit = np.asarray(hit, dtype=np.int64)
    num = len(hit)
    color = np.tile(np.asarray(background, dtype=F32), (num, 1))
    alpha, depth = np.zeros(num, dtype=F32), np.zeros(num, dtype=F32)
    rows = np.flatnonzero((hit >= 0) & (hit < len(triangles)))
    if len(rows) == 0:
        return color, alpha, depth
    corner = ids[hit[rows]]
    with np.errstate(all="ignore"):
        b1, b2 = _f32(u)[rows], _f32(v)[rows]
        b0 = (F32(1.0) - b1) - b2
        blend = np.stack([(values[corner[:, 0], j] * b0 + values[corner[:, 1], j] * b1)
                          + values[corner[:, 2], j] * b2 for j in range(values.shape[1])], -1)
        color[rows] = blend if colors is not None else texture_lookup(blend[:, 0], blend[:, 1],
                                                                      np.asarray(texture))
    alpha[rows] = 1.0
    depth[rows] = _f32(t)[rows]
    return color, alpha, depth


# ------------------------------------------------------------------------------- rays and scenes
def camera_rays(camera):
    """The ray of every pixel of a ``CameraInfo`` in float64, unnormalised as ``raycast64`` has
    them (the component along the camera's axis is 1) -> (starts, directions) (H W,3) f32."""
    width, height = int(camera.resolution.width), int(camera.resolution.height)
    k_inv = np.linalg.inv(np.asarray(camera.intrinsics, dtype=np.float64)[:3, :3])
    pose = np.asarray(camera.extrinsics, dtype=np.float64)
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    pixel = np.stack([px.reshape(-1), py.reshape(-1), np.ones(width * height)], 0)
    directions = (pose[:3, :3] @ (k_inv @ pixel)).T
    starts = np.tile(pose[:3, 3], (width * height, 1))
    return starts.astype(F32), directions.astype(F32)


def random_rays(seed, count, spread=2.0):
    """Rays from around the scenes of ``mesh_raster_reference.scene`` towards points inside them."""
    rng = np.random.default_rng(seed)
    starts = rng.uniform(-spread, spread, (count, 3))
    targets = rng.uniform(-0.6, 0.6, (count, 3))
    return starts.astype(F32), (targets - starts).astype(F32)


def box_mesh(half=1.0):
    """A closed axis-aligned cube of 12 triangles, two per face in the order -x +x -y +y -z +z ->
    (vertices (8,3) f32, triangles (12,3) int32)."""
    vertices = np.array([[x, y, z] for x in (-half, half) for y in (-half, half)
                         for z in (-half, half)], dtype=F32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    triangles = np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], dtype=np.int32)
    return vertices, triangles
