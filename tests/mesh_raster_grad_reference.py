"""The numpy restatement of K32 (csrc/mesh_raster_grad.hip), on top of tests/mesh_raster_reference.py.

``face_sums`` and ``vertex_gather`` follow the contract of include/ffn_hip.h operation for
operation: every value a numpy float32, every product and add one rounded f32 operation, a segment
of 64 box pixels folded by halves (``a[:h] + a[h:2h]``, h = 32 .. 1: the xor butterfly, an IEEE add
being commutative bit for bit), the segments added in order from 0.0f, the corners of a vertex added
in CSR order from 0.0f.  They have to give the kernels' bits.  ``adjacency`` is the stable argsort
``mesh.vertex_adjacency`` makes; ``mean_colors`` and ``color_mesh`` restate
``color_mesh_from_images``.

``gamma`` and the three ``*_budget`` functions are the error budgets of the float64 identities the
tests hold K32 to, counted from the f32 roundings of the contract (derived where they stand).

Nothing here needs a GPU.
"""

import numpy as np

from tests import mesh_raster_reference as R

F32 = np.float32
U = 2.0 ** -24                      # the unit roundoff of f32
FOLD_DEPTH = 6                      # adds a lane value passes in the butterfly of 64
MAX_BOX = 1 << 28


def ids_of(zbuf):
    """The ids K31c writes: the low word of a drawn z-buffer entry, -1 where nothing was drawn."""
    low = (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.where(zbuf == R.EMPTY, -1, low).astype(np.int32)


def raster_ids(vertices, triangles, proj, width, height):
    """K31a + K31b -> (state, ids (H W,) int32)."""
    state = R.setup(vertices, triangles, proj, width, height)
    return state, ids_of(R.draw(state, width, height))


def fold64(values):
    """(64, ...) f32 -> (...): the fold by halves."""
    h = 32
    while h >= 1:
        values = values[:h] + values[h:2 * h]
        h //= 2
    return values[0]


def face_sums(state, ids, d_color, width, height):
    """K32a -> (F,12) f32.  ``state`` from ``R.setup``; ``d_color`` (H W,3) f32 is read at the
    selected pixels only."""
    d_color = np.asarray(d_color, dtype=F32)
    out = np.zeros((len(state["box"]), 12), dtype=F32)
    for f, (x0, y0, x1, y1) in enumerate(state["box"]):
        if x0 < 0 or y0 < 0 or x1 >= width or y1 >= height or x1 < x0 or y1 < y0:
            continue
        bw = int(x1 - x0 + 1)
        n = bw * int(y1 - y0 + 1)
        if n > MAX_BOX:
            continue
        k = np.arange(n, dtype=np.int64)
        px, py = x0 + k % bw, y0 + k // bw
        pixel = py * width + px
        chosen = np.flatnonzero(ids[pixel] == f)
        t = np.zeros((64 * ((n + 63) // 64), 12), dtype=F32)
        if len(chosen):
            _, q, depth_w = R.terms(state["X"][f], state["Y"][f], state["w"][f], px[chosen],
                                    py[chosen])
            g = d_color[pixel[chosen]]
            with np.errstate(all="ignore"):
                for i in range(3):
                    b = q[i] * depth_w
                    for j in range(3):
                        t[chosen, 3 * i + j] = b * g[:, j]
                    t[chosen, 9 + i] = b
        acc = np.zeros(12, dtype=F32)
        with np.errstate(all="ignore"):
            for s in range(len(t) // 64):
                acc = acc + fold64(t[64 * s:64 * s + 64])
        out[f] = acc
    return out


def adjacency(triangles, num_vertices):
    """-> (corner_order (3F,) int32, vertex_starts (V+1,) int32), ids clamped as K31 clamps."""
    flat = np.clip(np.asarray(triangles, dtype=np.int64).reshape(-1), 0, num_vertices - 1)
    order = np.argsort(flat, kind="stable").astype(np.int32)
    starts = np.zeros(num_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=num_vertices), out=starts[1:])
    return order, starts.astype(np.int32)


def vertex_gather(sums, corner_order, vertex_starts, grad=None, weight=None, accumulate=False):
    """K32b -> (grad (V,3), weight (V,)) f32; with ``accumulate`` ``out = out + value``."""
    num_vertices, num_corners = len(vertex_starts) - 1, 3 * len(sums)
    g = np.zeros((num_vertices, 3), dtype=F32)
    w = np.zeros(num_vertices, dtype=F32)
    with np.errstate(all="ignore"):
        for v in range(num_vertices):
            begin, end = max(int(vertex_starts[v]), 0), min(int(vertex_starts[v + 1]), num_corners)
            for corner in corner_order[begin:end]:
                if not 0 <= corner < num_corners:
                    continue
                f, i = divmod(int(corner), 3)
                g[v] = g[v] + sums[f, 3 * i:3 * i + 3]
                w[v] = w[v] + sums[f, 9 + i]
        if accumulate:
            return grad + g, weight + w
    return g, w


def backward(vertices, triangles, proj, width, height, d_color, ids=None):
    """``render_mesh_backward`` -> (grad, weight, state, ids)."""
    state, own = raster_ids(vertices, triangles, proj, width, height)
    ids = own if ids is None else ids
    order, starts = adjacency(triangles, len(vertices))
    grad, weight = vertex_gather(face_sums(state, ids, d_color, width, height), order, starts)
    return grad, weight, state, ids


def mean_colors(sums, weights, colors=None):
    """``color_mesh_from_images``' last step: ``sums / weights`` where ``weights > 0``, one f32
    division per channel; ``colors`` (0.5 grey when None) elsewhere."""
    out = np.full(sums.shape, 0.5, dtype=F32) if colors is None else np.array(colors, dtype=F32)
    seen = weights > 0
    out[seen] = sums[seen] / weights[seen][:, None]
    return out


def color_mesh(vertices, triangles, projections, images, colors=None, alpha_threshold=0.5):
    """``color_mesh_from_images`` on (C,H,W,4) uint8 images and their (3,4) projections."""
    height, width = images.shape[1:3]
    alpha_u8 = min(max(int(np.ceil(float(alpha_threshold) * 255)), 1), 255)
    order, starts = adjacency(triangles, len(vertices))
    total, weights = None, None
    for proj, frame in zip(projections, images):
        state, ids = raster_ids(vertices, triangles, proj, width, height)
        ids = np.where(frame[..., 3].reshape(-1) < alpha_u8, -1, ids).astype(np.int32)
        rgb = (frame[..., :3].astype(F32) / 255).reshape(-1, 3)
        total, weights = vertex_gather(face_sums(state, ids, rgb, width, height), order, starts,
                                       total, weights, accumulate=total is not None)
    return mean_colors(total, weights, colors), weights


# ------------------------------------------------------------------------------- budgets
def gamma(n):
    """Higham's gamma_n = n u / (1 - n u): the relative error n f32 roundings leave at most."""
    return n * U / (1.0 - n * U)


def sum_depth(state, ids, vertex_starts):
    """The most f32 adds one term passes on its way into a vertex's sum: the fold (6), one add per
    segment of the largest box that wins a pixel, one per corner of the fullest vertex."""
    boxes = state["box"][np.unique(ids[ids >= 0])]
    pixels = (boxes[:, 2] - boxes[:, 0] + 1) * (boxes[:, 3] - boxes[:, 1] + 1)
    segments = int((pixels.max() + 63) // 64) if len(pixels) else 0
    valence = int(np.diff(vertex_starts).max())
    return FOLD_DEPTH + segments + valence


def weights_of(state, ids, width):
    """The f32 b_i K31c and K32a use at every covered pixel -> (pixels, triangle, b (3, n))."""
    hit = np.flatnonzero(ids >= 0)
    f = ids[hit].astype(np.int64)
    _, q, depth_w = R.terms(state["X"][f], state["Y"][f], state["w"][f], hit % width, hit // width)
    return hit, f, np.stack([q[i] * depth_w for i in range(3)])


def adjoint_budget(state, ids, width, colors, g, vertex_starts):
    """|sum_p color[p] . g[p] - sum_v c_v . grad_v| is at most this.  Both sides are sums of the
    reals c_{v_i} b_i g[p][j] with the same f32 b_i.  On the left K31c rounds three products and two
    adds per channel: gamma_3 of the term's size.  On the right K32 rounds the product b_i g once and
    every add the term passes after it (``sum_depth``); adding a +0 is exact.  So the two differ by
    at most (gamma_3 + gamma_{1 + depth}) A <= gamma_{4 + depth} A, A = sum |c b g| in float64; the
    float64 sums themselves add 1e-13 A."""
    hit, f, b = weights_of(state, ids, width)
    corner = state["ids"][f]
    size = 0.0
    for i in range(3):
        c = np.abs(np.asarray(colors, dtype=np.float64)[corner[:, i]])
        size += float((c * b[i].astype(np.float64)[:, None]
                       * np.abs(np.asarray(g, dtype=np.float64)[hit])).sum())
    return (gamma(4 + sum_depth(state, ids, vertex_starts)) + 1e-13) * size


def weight_budget(state, ids, vertex_starts):
    """|sum_v weight_v - covered pixels| is at most this.  At a covered pixel every q_i >= 0, so
    inv_w = (q0 + q1) + q2 is within gamma_2 of their sum, depth_w = 1 / inv_w adds one rounding and
    b_i = q_i depth_w one more: sum_i b_i is within gamma_4 of 1.  The b_i are then added in f32,
    ``sum_depth`` adds each: gamma_{4 + depth} per pixel in all."""
    covered = int((ids >= 0).sum())
    return (gamma(4 + sum_depth(state, ids, vertex_starts)) + 1e-13) * covered


def splat_budget(state, ids, vertex_starts, constant):
    """|sum_v / weight_v - c| per channel for a frame rendered from the one colour c > 0.  The
    frame's colour is c sum_i b_i within gamma_3 (three products, two adds, all terms >= 0), and
    sum_i b_i within gamma_4 of 1 (``weight_budget``): c within gamma_7.  The numerator adds
    b_i color[p] with one product and ``depth`` adds, the denominator b_i with ``depth`` adds, all
    terms >= 0, and the quotient rounds once: gamma_{7 + 1 + depth + depth + 1} of c."""
    depth = sum_depth(state, ids, vertex_starts)
    return gamma(9 + 2 * depth) * np.abs(np.asarray(constant, dtype=np.float64))
