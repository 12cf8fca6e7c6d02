"""Two independent statements of what K35 (csrc/mesh_interp_grad.hip) computes, on top of
tests/mesh_raster_reference.py.

The RESTATEMENT follows the contract of include/ffn_hip.h operation by operation: the edge functions
are int64, every float value is a numpy float32 and every operation one rounded f32 operation in
the header's order; a segment of 64 box pixels is folded by halves and the segments are added in
order from 0.0f (K32a's sums), the corners of a vertex in CSR order.  ``face_grads`` is K35a,
``vertex_grad`` K35b.  They have to give the kernels' outputs bit for bit.

The MODEL is what the restatement itself is held to.  It is float64 and shares no code with the
restatement: for fixed ids it gives the colour of every covered pixel as a smooth function of the
vertex positions -- the float64 projection, the snap (and the f32 rounding of ``w``) entered as a
constant offset frozen at the starting positions, so that "passed straight through" is exact in the
model, barycentric coordinates as ratios of cross products of real-valued screen points, and the
perspective-correct blend sum(c l / w) / sum(l / w).  Its derivatives are central differences.

Nothing here needs a GPU.
"""

import numpy as np

from tests import mesh_raster_reference as R

F32 = np.float32
MAX_BOX = 1 << 28


# ------------------------------------------------------------------------------- restatement
def _fold64(values):
    h = 32
    while h >= 1:
        values = values[:h] + values[h:2 * h]
        h //= 2
    return values[0]


def _edges(x, y, qx, qy):
    """E_0 .. E_2 of K31b (int64, sgn(A) applied) at the points Q -> (list of arrays, A)."""
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    sign = -1 if area < 0 else 1
    out = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        out.append(sign * ((x[k] - x[j]) * (qy - y[j]) - (y[k] - y[j]) * (qx - x[j])))
    return out, area


def pixel_terms(state, f, colors, px, py, g):
    """The nine terms of K35a for triangle ``f`` at the pixels (px, py) with the gradients ``g``
    (n,3) -> (n,9) f32."""
    x = [np.int64(v) for v in state["X"][f]]
    y = [np.int64(v) for v in state["Y"][f]]
    w = [F32(v) for v in state["w"][f]]
    corner = np.asarray(colors, dtype=F32)[state["ids"][f]]                 # (3,3)
    qx, qy = 256 * np.asarray(px, dtype=np.int64), 256 * np.asarray(py, dtype=np.int64)
    e, area = _edges(x, y, qx, qy)
    sign = -1 if area < 0 else 1
    g = np.asarray(g, dtype=F32)
    out = np.zeros((len(qx), 9), dtype=F32)
    with np.errstate(all="ignore"):
        size = F32(float(abs(int(area))))
        nx, ny = [], []
        for i in range(3):
            j, k = (i + 1) % 3, (i + 2) % 3
            dx, dy = sign * -(int(y[k]) - int(y[j])), sign * (int(x[k]) - int(x[j]))
            nx.append((F32(256.0) * F32(float(dx))) / size)
            ny.append((F32(256.0) * F32(float(dy))) / size)
        lam = [e[i].astype(F32) / size for i in range(3)]
        q = [lam[i] / w[i] for i in range(3)]
        depth_w = F32(1.0) / ((q[0] + q[1]) + q[2])
        b = [q[i] * depth_w for i in range(3)]
        mixed = [(corner[0][ch] * b[0] + corner[1][ch] * b[1]) + corner[2][ch] * b[2]
                 for ch in range(3)]
        r = []
        for i in range(3):
            a = (g[:, 0] * (corner[i][0] - mixed[0]) + g[:, 1] * (corner[i][1] - mixed[1])) \
                + g[:, 2] * (corner[i][2] - mixed[2])
            r.append((a * depth_w) / w[i])
        gx = (r[0] * nx[0] + r[1] * nx[1]) + r[2] * nx[2]
        gy = (r[0] * ny[0] + r[1] * ny[1]) + r[2] * ny[2]
        for j in range(3):
            out[:, 3 * j + 0] = -(lam[j] * gx)
            out[:, 3 * j + 1] = -(lam[j] * gy)
            out[:, 3 * j + 2] = -(r[j] * q[j])
    return out


def selected(state, f, ids, width, height):
    """The box pixels of triangle ``f`` that ``ids`` gives it -> (n box pixels, chosen k, px, py,
    pixel), or None for a box that contributes nothing."""
    x0, y0, x1, y1 = [int(v) for v in state["box"][f]]
    if x0 < 0 or y0 < 0 or x1 >= width or y1 >= height or x1 < x0 or y1 < y0:
        return None
    bw = x1 - x0 + 1
    n = bw * (y1 - y0 + 1)
    if n > MAX_BOX:
        return None
    k = np.arange(n, dtype=np.int64)
    px, py = x0 + k % bw, y0 + k // bw
    pixel = py * width + px
    chosen = np.flatnonzero(np.asarray(ids)[pixel] == f)
    return n, chosen, px[chosen], py[chosen], pixel[chosen]


def face_grads(state, ids, d_color, colors, width, height):
    """K35a -> (F,9) f32.  ``state`` from ``R.setup``; ``d_color`` (H W,3) f32 is read at the
    selected pixels only."""
    d_color = np.asarray(d_color, dtype=F32)
    out = np.zeros((len(state["box"]), 9), dtype=F32)
    for f in range(len(state["box"])):
        found = selected(state, f, ids, width, height)
        if found is None:
            continue
        n, chosen, px, py, pixel = found
        t = np.zeros((64 * ((n + 63) // 64), 9), dtype=F32)
        if len(chosen):
            t[chosen] = pixel_terms(state, f, colors, px, py, d_color[pixel])
        acc = np.zeros(9, dtype=F32)
        with np.errstate(all="ignore"):
            for s in range(len(t) // 64):
                acc = acc + _fold64(t[64 * s:64 * s + 64])
        out[f] = acc
    return out


def vertex_grad(grads, corner_order, vertex_starts, vertices, proj, grad=None):
    """K35b -> (V,3) f32; added to ``grad`` when given (accumulate)."""
    vertices = np.asarray(vertices, dtype=F32)
    p = np.asarray(proj, dtype=F32).reshape(3, 4)
    num_vertices, num_corners = len(vertices), 3 * len(grads)
    flat = np.asarray(grads, dtype=F32).reshape(-1, 3)
    out = np.zeros((num_vertices, 3), dtype=F32)
    with np.errstate(all="ignore"):
        x, y, w = R.project(p, vertices)
        sx, sy = x / w, y / w
        for v in range(num_vertices):
            begin = max(int(vertex_starts[v]), 0)
            end = min(int(vertex_starts[v + 1]), num_corners)
            gx = gy = gw = F32(0.0)
            for corner in corner_order[begin:end]:
                if not 0 <= corner < num_corners:
                    continue
                gx = gx + flat[corner][0]
                gy = gy + flat[corner][1]
                gw = gw + flat[corner][2]
            if not w[v] > 0:
                continue
            for c in range(3):
                out[v][c] = ((gx * (p[0, c] - sx[v] * p[2, c]))
                             + (gy * (p[1, c] - sy[v] * p[2, c]))) / w[v] + gw * p[2, c]
        if grad is not None:
            out = np.asarray(grad, dtype=F32) + out
    return out


def adjacency(triangles, num_vertices):
    """``mesh.vertex_adjacency`` -> (corner_order (3F,) int32, vertex_starts (V+1,) int32)."""
    flat = np.clip(np.asarray(triangles, dtype=np.int64).reshape(-1), 0, num_vertices - 1)
    order = np.argsort(flat, kind="stable").astype(np.int32)
    starts = np.zeros(num_vertices + 1, dtype=np.int64)
    np.cumsum(np.bincount(flat, minlength=num_vertices), out=starts[1:])
    return order, starts.astype(np.int32)


def interior_backward(state, ids, d_color, colors, vertices, triangles, proj, width, height,
                      grad=None):
    """K35a and K35b on one frame -> (grad (V,3), face_grads (F,9))."""
    grads = face_grads(state, ids, d_color, colors, width, height)
    order, starts = adjacency(triangles, len(vertices))
    return vertex_grad(grads, order, starts, vertices, proj, grad), grads


# ------------------------------------------------------------------------------- float64 model
def blend64(screen, w, corner_colors, points):
    """The perspective-correct colour at the screen ``points`` (n,2) of the triangle with the screen
    corners ``screen`` (3,2), their ``w`` (3,) and colours (3,3), all float64 -> (n,3)."""
    s = np.asarray(screen, dtype=np.float64)
    pts = np.asarray(points, dtype=np.float64)

    def cross(a, b):
        return a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]

    whole = cross(s[1] - s[0], s[2] - s[0])
    weights = np.stack([cross(s[(i + 1) % 3] - pts, s[(i + 2) % 3] - pts) / whole
                        for i in range(3)], -1)                             # (n,3), sum to 1
    over_w = weights / np.asarray(w, dtype=np.float64)
    return (over_w @ np.asarray(corner_colors, dtype=np.float64)) / over_w.sum(-1, keepdims=True)


def triangle_loss64(screen, w, corner_colors, points, g):
    """sum_p g[p] . colour(p) over one triangle's pixels, float64."""
    return float((blend64(screen, w, corner_colors, points) * np.asarray(g, np.float64)).sum())


class Model64:
    """The image's covered pixels as a function of the (V,3) positions, ids frozen."""

    def __init__(self, state, ids, vertices, proj, colors, width, g):
        self.proj = np.asarray(proj, dtype=np.float64).reshape(3, 4)
        self.colors = np.asarray(colors, dtype=np.float64)
        self.corners = state["ids"]
        ids = np.asarray(ids)
        hit = np.flatnonzero(ids >= 0)
        self.rows = []
        for f in np.unique(ids[hit]):
            pixels = hit[ids[hit] == f]
            points = np.stack([pixels % width, pixels // width], -1).astype(np.float64)
            self.rows.append((int(f), points, np.asarray(g, dtype=np.float64)[pixels]))
        start = np.asarray(vertices, dtype=np.float64)
        own = self.project(start)
        # the snap and the f32 rounding of w, frozen: what the record holds minus the float64
        # projection of the starting positions
        self.offset = np.zeros((len(start), 3))
        drawn = state["status"] == R.DRAWN
        held = np.stack([state["X"][drawn] / 256.0, state["Y"][drawn] / 256.0,
                         state["w"][drawn].astype(np.float64)], -1).reshape(-1, 3)
        users = state["ids"][drawn].reshape(-1)
        self.offset[users] = held - own[users]

    def project(self, positions):
        homog = np.asarray(positions, dtype=np.float64) @ self.proj[:, :3].T + self.proj[:, 3]
        return np.stack([homog[:, 0] / homog[:, 2], homog[:, 1] / homog[:, 2], homog[:, 2]], -1)

    def loss(self, positions, only=None):
        """sum over the covered pixels of g . colour; ``only``: the triangles to sum over."""
        placed = self.project(positions) + self.offset
        total = 0.0
        for f, points, g in self.rows:
            if only is not None and f not in only:
                continue
            c = self.corners[f]
            total += triangle_loss64(placed[c, :2], placed[c, 2], self.colors[c], points, g)
        return total


# ------------------------------------------------------------------------------- scenes
def tetrahedron_with_a_face_vertex():
    """A closed convex mesh: a tetrahedron whose face towards -z is split into three triangles by a
    vertex at its centroid -> (vertices (5,3) f32, triangles (6,3) int32, the centroid's id).  Seen
    from -z (``R.camera(..., yaw=0, pitch=0)``) the centroid lies on a face, is visible and lies on
    no outline."""
    a, b, c = [-0.9, -0.7, -0.3], [0.95, -0.6, -0.3], [0.05, 0.9, -0.3]
    apex = [0.0, 0.0, 0.8]
    centre = [(a[i] + b[i] + c[i]) / 3 for i in range(3)]
    vertices = np.array([a, b, c, apex, centre], dtype=np.float32)
    triangles = np.array([[0, 1, 4], [1, 2, 4], [2, 0, 4], [1, 0, 3], [2, 1, 3], [0, 2, 3]],
                         dtype=np.int32)
    return vertices, triangles, 4
