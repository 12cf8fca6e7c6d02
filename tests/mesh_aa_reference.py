"""Two independent statements of what K34 (csrc/mesh_aa.hip) computes, on top of
tests/mesh_raster_reference.py.

The RESTATEMENT follows the contract of include/ffn_hip.h operation by operation: every decision is
made on Python integers (exact, as the kernel's int64), every float value is a numpy float32 and every
operation one rounded f32 operation in the header's order.  ``decide`` is the pair decision,
``forward`` K34a, ``backward`` K34b, ``vertex_grad`` the stable sort and K34c, ``laplacian`` K34d.
They have to give the kernels' outputs bit for bit.

The MODEL is what the restatement itself is held to.  It is float64 and shares no arithmetic with
the restatement: given the restatement's frozen decisions per pair (active, f, i*, a, b, target) it
evaluates the antialiased image as a smooth function of real-valued screen coordinates -- the
crossing of the segment between two pixel centres with the line through two screen points, as a ratio
of two cross products -- and the projection x / w as a function of the 3-D positions.  Its
derivatives are central differences.  ``forward64`` / ``transpose64`` state the blend and its
transpose in float64 for the adjoint identity.

Nothing here needs a GPU.
"""

import numpy as np

from tests import mesh_raster_reference as R

F32 = np.float32
HALF = F32(0.5)
S256 = F32(256.0)


def f32(value):
    """(float)int64: exact to float64 below 2^53, then one rounding -- the kernel's conversion."""
    return F32(float(int(value)))


# ------------------------------------------------------------------------------- restatement
def frame(vertices, triangles, proj, eye, width, height, colors=None, uvs=None, texture=None,
          background=(0, 0, 0)):
    """K31a-c -> dict(state, zbuf, color, alpha, ids, width, height, ...): what K34 reads."""
    state = R.setup(vertices, triangles, proj, width, height)
    zbuf = R.draw(state, width, height)
    color, alpha, depth, ids = R.resolve(state, zbuf, vertices, eye, width, height, colors, uvs,
                                         texture, background)
    return dict(state=state, zbuf=zbuf, color=color, alpha=alpha, depth=depth, ids=ids,
                width=width, height=height, vertices=np.asarray(vertices, dtype=F32),
                triangles=np.asarray(triangles), proj=np.asarray(proj, dtype=F32).reshape(3, 4))


def edges(state, f, qx, qy):
    """E_0 .. E_2 of K31b at Q with sgn(A) applied, as Python ints -> (list, A)."""
    x = [int(v) for v in state["X"][f]]
    y = [int(v) for v in state["Y"][f]]
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    sign = -1 if area < 0 else 1
    out = []
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        out.append(sign * ((x[k] - x[j]) * (qy - y[j]) - (y[k] - y[j]) * (qx - x[j])))
    return out, area


def attempt(fr, opposite, a, b):
    """attempt(a -> b) -> dict(f, edge, alpha, d, sign, a, b) or None."""
    state, width = fr["state"], fr["width"]
    f = int(fr["ids"][a])
    if not 0 <= f < len(state["X"]):
        return None
    ea, area = edges(state, f, 256 * (a % width), 256 * (a // width))
    eb, _ = edges(state, f, 256 * (b % width), 256 * (b // width))
    if area == 0 or min(ea) < 0:
        return None
    best, best_alpha = -1, None
    for i in range(3):
        if eb[i] >= 0:
            continue
        alpha = f32(ea[i]) / f32(ea[i] - eb[i])
        if best < 0 or alpha < best_alpha:
            best, best_alpha = i, alpha
    if best < 0:
        return None
    sign = -1 if area < 0 else 1
    o = int(opposite[3 * f + best])
    if o >= 0:
        o = min(o, len(fr["vertices"]) - 1)
        with np.errstate(all="ignore"):
            x, y, w = R.project(fr["proj"], fr["vertices"][o:o + 1])
            sx, sy = x / w, y / w
            if not w[0] > 0 or not abs(sx[0]) <= R.GUARD or not abs(sy[0]) <= R.GUARD:
                return None
            ox, oy = int(np.rint(sx[0] * S256)), int(np.rint(sy[0] * S256))
        j, k = (best + 1) % 3, (best + 2) % 3
        xs, ys = state["X"][f], state["Y"][f]
        side = sign * ((int(xs[k]) - int(xs[j])) * (oy - int(ys[j]))
                       - (int(ys[k]) - int(ys[j])) * (ox - int(xs[j])))
        if side < 0:
            return None
    return dict(f=f, edge=best, alpha=best_alpha, d=ea[best] - eb[best], sign=sign, a=a, b=b)


def decide(fr, opposite, p, q):
    """The pair decision of (p, q) -> the attempt's dict with s, m, target, source; or None."""
    ids, zbuf = fr["ids"], fr["zbuf"]
    if ids[p] == ids[q]:
        return None
    near, far = (q, p) if int(zbuf[q]) < int(zbuf[p]) else (p, q)
    found = attempt(fr, opposite, near, far)
    if found is None and ids[far] >= 0:
        found = attempt(fr, opposite, far, near)
    if found is None:
        return None
    s = found["alpha"] - HALF
    forward = bool(s >= 0)
    found.update(s=s, m=np.abs(s), target=found["b"] if forward else found["a"],
                 source=found["a"] if forward else found["b"])
    return found


def decisions(fr, opposite):
    """Every slot's decision -> list of 2 H W entries, slot (p, axis) at 2 p + axis; None for an
    inactive or non-existent slot."""
    width, height = fr["width"], fr["height"]
    out = [None] * (2 * width * height)
    for p in range(width * height):
        if p % width + 1 < width:
            out[2 * p] = decide(fr, opposite, p, p + 1)
        if p // width + 1 < height:
            out[2 * p + 1] = decide(fr, opposite, p, p + width)
    return out


def pairs_of(p, width, height):
    """The slots of pixel p's pairs in the order left, right, up, down, those that exist."""
    px, py = p % width, p // width
    slots = []
    if px > 0:
        slots.append(2 * (p - 1))
    if px + 1 < width:
        slots.append(2 * p)
    if py > 0:
        slots.append(2 * (p - width) + 1)
    if py + 1 < height:
        slots.append(2 * p + 1)
    return slots


def channels(color, alpha):
    return np.concatenate([np.asarray(color, dtype=F32).reshape(-1, 3),
                           np.asarray(alpha, dtype=F32).reshape(-1, 1)], 1)


def forward(fr, made, color=None, alpha=None):
    """K34a -> (out_color (H W,3), out_alpha (H W,)) f32."""
    width, height = fr["width"], fr["height"]
    values = channels(fr["color"] if color is None else color,
                      fr["alpha"] if alpha is None else alpha)
    out = values.copy()
    with np.errstate(all="ignore"):
        for p in range(width * height):
            for slot in pairs_of(p, width, height):
                pair = made[slot]
                if pair is None or pair["target"] != p:
                    continue
                out[p] = out[p] + pair["m"] * (values[pair["source"]] - values[p])
    return out[:, :3].copy(), out[:, 3].copy()


def backward(fr, made, g_color, g_alpha):
    """K34b -> (d_color, d_alpha, entry_vertex (4 H W,) int32, entry_grad (4 H W,2) f32)."""
    width, height = fr["width"], fr["height"]
    state = fr["state"]
    num_vertices = len(fr["vertices"])
    values = channels(fr["color"], fr["alpha"])
    g = channels(g_color, g_alpha)
    d = g.copy()
    entry_vertex = np.full(4 * width * height, num_vertices, dtype=np.int32)
    entry_grad = np.zeros((4 * width * height, 2), dtype=F32)
    with np.errstate(all="ignore"):
        for p in range(width * height):
            for slot in pairs_of(p, width, height):
                pair = made[slot]
                if pair is None:
                    continue
                if pair["target"] == p:
                    d[p] = d[p] - pair["m"] * g[p]
                else:
                    d[p] = d[p] + pair["m"] * g[pair["target"]]
        for slot, pair in enumerate(made):
            if pair is None:
                continue
            f, t = pair["f"], pair["target"]
            delta = values[pair["source"]] - values[t]
            total = ((g[t][0] * delta[0] + g[t][1] * delta[1]) + g[t][2] * delta[2]) \
                + g[t][3] * delta[3]
            d_alpha_pair = total if pair["s"] >= 0 else -total
            j, k = (pair["edge"] + 1) % 3, (pair["edge"] + 2) % 3
            ax, ay = pair["a"] % width, pair["a"] // width
            bx, by = pair["b"] % width, pair["b"] // width
            cx = f32(256 * ax) + pair["alpha"] * f32(256 * (bx - ax))
            cy = f32(256 * ay) + pair["alpha"] * f32(256 * (by - ay))
            cjx, cjy = cx - f32(state["X"][f][j]), cy - f32(state["Y"][f][j])
            ckx, cky = cx - f32(state["X"][f][k]), cy - f32(state["Y"][f][k])
            signed = d_alpha_pair if pair["sign"] > 0 else -d_alpha_pair
            r256 = S256 * (signed / f32(pair["d"]))
            e = 2 * slot                       # 4 p + 2 axis
            entry_vertex[e] = state["ids"][f][k]
            entry_vertex[e + 1] = state["ids"][f][j]
            entry_grad[e] = (r256 * cjy, -(r256 * cjx))
            entry_grad[e + 1] = (-(r256 * cky), r256 * ckx)
    return d[:, :3].copy(), d[:, 3].copy(), entry_vertex, entry_grad


def sort_entries(entry_vertex):
    """The caller's stable sort -> (sorted_vertex, order) int32."""
    order = np.argsort(entry_vertex, kind="stable").astype(np.int32)
    return entry_vertex[order].astype(np.int32), order


def vertex_grad(entry_vertex, entry_grad, vertices, proj, grad=None):
    """The stable sort and K34c -> grad (V,3) f32; added to ``grad`` when given (accumulate)."""
    vertices = np.asarray(vertices, dtype=F32)
    p = np.asarray(proj, dtype=F32).reshape(3, 4)
    sorted_vertex, order = sort_entries(entry_vertex)
    out = np.zeros((len(vertices), 3), dtype=F32)
    with np.errstate(all="ignore"):
        x, y, w = R.project(p, vertices)
        sx, sy = x / w, y / w
        for v in range(len(vertices)):
            begin = np.searchsorted(sorted_vertex, v, side="left")
            end = np.searchsorted(sorted_vertex, v + 1, side="left")
            gx = gy = F32(0.0)
            for e in order[begin:end]:
                gx = gx + entry_grad[e][0]
                gy = gy + entry_grad[e][1]
            if not w[v] > 0:
                continue
            for c in range(3):
                out[v][c] = ((gx * (p[0, c] - sx[v] * p[2, c]))
                             + (gy * (p[1, c] - sy[v] * p[2, c]))) / w[v]
        if grad is not None:
            out = np.asarray(grad, dtype=F32) + out
    return out


def laplacian(values, starts, neighbors, scale, out=None):
    """K34d -> (V,3) f32; added to ``out`` when given (accumulate)."""
    values = np.asarray(values, dtype=F32)
    scale = F32(scale)
    result = np.zeros_like(values)
    with np.errstate(all="ignore"):
        for v in range(len(values)):
            acc = np.zeros(3, dtype=F32)
            for n in neighbors[max(int(starts[v]), 0):min(int(starts[v + 1]), len(neighbors))]:
                if 0 <= n < len(values):
                    acc = acc + (values[v] - values[n])
            result[v] = scale * acc
        if out is not None:
            result = np.asarray(out, dtype=F32) + result
    return result


def geometry_backward(vertices, triangles, proj, eye, width, height, colors, opposite, g_color,
                      g_alpha, grad=None, background=(0, 0, 0)):
    """``mesh.render_mesh_geometry_backward`` for one camera -> (grad, d_color, d_alpha, frame,
    decisions, (entry_vertex, entry_grad))."""
    fr = frame(vertices, triangles, proj, eye, width, height, colors, background=background)
    made = decisions(fr, opposite)
    d_color, d_alpha, entry_vertex, entry_grad = backward(fr, made, g_color, g_alpha)
    grad = vertex_grad(entry_vertex, entry_grad, vertices, proj, grad)
    return grad, d_color, d_alpha, fr, made, (entry_vertex, entry_grad)


# ------------------------------------------------------------------------------- host plumbing
def opposites_brute(triangles, num_vertices):
    """``mesh.edge_opposites`` by loops: the undirected edge of corner 3 f + i is used by exactly
    two corners, of two different triangles -> the other triangle's vertex off the edge, else -1."""
    tri = np.clip(np.asarray(triangles, dtype=np.int64), 0, num_vertices - 1)
    out = np.full(3 * len(tri), -1, dtype=np.int32)

    def key(g, h):
        return tuple(sorted((int(tri[g][(h + 1) % 3]), int(tri[g][(h + 2) % 3]))))

    for f in range(len(tri)):
        for i in range(3):
            users = [(g, h) for g in range(len(tri)) for h in range(3) if key(g, h) == key(f, i)]
            others = [(g, h) for g, h in users if (g, h) != (f, i)]
            if len(users) == 2 and others[0][0] != f:
                out[3 * f + i] = tri[others[0][0]][others[0][1]]
    return out


def neighbors_brute(triangles, num_vertices):
    """``mesh.vertex_neighbors`` by loops -> (starts (V+1,), neighbors) int32."""
    tri = np.clip(np.asarray(triangles, dtype=np.int64), 0, num_vertices - 1)
    rows = [set() for _ in range(num_vertices)]
    for corners in tri:
        for i in range(3):
            a, b = int(corners[i]), int(corners[(i + 1) % 3])
            if a != b:
                rows[a].add(b)
                rows[b].add(a)
    starts = np.zeros(num_vertices + 1, dtype=np.int32)
    starts[1:] = np.cumsum([len(row) for row in rows])
    flat = [n for row in rows for n in sorted(row)]
    return starts, np.array(flat, dtype=np.int32)


# ------------------------------------------------------------------------------- float64 model
def screen64(proj, positions):
    """x / w, y / w of (N,3) positions in float64 -> (N,2) screen coordinates in pixels."""
    p = np.asarray(proj, dtype=np.float64).reshape(3, 4)
    homog = np.asarray(positions, dtype=np.float64) @ p[:, :3].T + p[:, 3]
    return homog[:, :2] / homog[:, 2:3]


def snapped_screen(fr):
    """The snapped screen position of every vertex a drawn triangle uses, X / 256 in float64 ->
    (V,2), NaN where no drawn triangle uses the vertex."""
    state = fr["state"]
    out = np.full((len(fr["vertices"]), 2), np.nan)
    drawn = state["status"] == R.DRAWN
    out[state["ids"][drawn].reshape(-1), 0] = state["X"][drawn].reshape(-1) / 256.0
    out[state["ids"][drawn].reshape(-1), 1] = state["Y"][drawn].reshape(-1) / 256.0
    return out


def crossing64(fr, pair, screen):
    """Where the segment from the centre of pixel a to that of pixel b meets the line through the
    screen points of the pair's edge: t in a + t (b - a), a ratio of two cross products."""
    width = fr["width"]
    corners = fr["state"]["ids"][pair["f"]]
    sj, sk = screen[corners[(pair["edge"] + 1) % 3]], screen[corners[(pair["edge"] + 2) % 3]]
    a = np.array([pair["a"] % width, pair["a"] // width], dtype=np.float64)
    b = np.array([pair["b"] % width, pair["b"] // width], dtype=np.float64)
    along, step = sk - sj, b - a
    return ((sj[0] - a[0]) * along[1] - (sj[1] - a[1]) * along[0]) \
        / (step[0] * along[1] - step[1] * along[0])


def image64(fr, made, screen):
    """The antialiased (H W,4) image in float64 with the decisions frozen: K31's colours and alpha
    stay, every active pair blends its frozen target by t - 1/2 (target b) or 1/2 - t (target a)."""
    values = channels(fr["color"], fr["alpha"]).astype(np.float64)
    out = values.copy()
    for pair in made:
        if pair is None:
            continue
        t = crossing64(fr, pair, screen)
        weight = t - 0.5 if pair["target"] == pair["b"] else 0.5 - t
        out[pair["target"]] += weight * (values[pair["source"]] - values[pair["target"]])
    return out


def loss64(fr, made, screen, g):
    return float((image64(fr, made, screen) * g).sum())


def weights64(made):
    """(target, source, m) of the active pairs in float64, from the restatement's decisions."""
    return [(pair["target"], pair["source"], float(pair["m"])) for pair in made if pair is not None]


def forward64(made, values):
    """J values: out[t] = in[t] + sum m (in[source] - in[t]) in float64."""
    out = np.array(values, dtype=np.float64)
    for target, source, m in weights64(made):
        out[target] += m * (values[source] - values[target])
    return out


def transpose64(made, g, width, height):
    """J^T g pixel by pixel as K34b gathers it: d[p] = g[p] - sum m g[p] over the pairs p is the
    target of + sum m g[target] over the pairs p is the source of."""
    g = np.asarray(g, dtype=np.float64)
    d = g.copy()
    for p in range(width * height):
        for slot in pairs_of(p, width, height):
            pair = made[slot]
            if pair is None:
                continue
            if pair["target"] == p:
                d[p] -= float(pair["m"]) * g[p]
            else:
                d[p] += float(pair["m"]) * g[pair["target"]]
    return d


# ------------------------------------------------------------------------------- scenes
def half_plane(edge, width=8, height=4, vertical=True, flip=False, z=1.0):
    """A big triangle under R.PIXEL_PROJ whose one edge is the line x = ``edge`` (or y = ``edge``)
    and which covers everything below it -> (vertices (3,3), triangles (1,3)).  ``flip`` reverses
    the winding."""
    far = -64.0
    if vertical:
        points = [(edge, -64.0), (edge, 64.0), (far, 0.0)]
    else:
        points = [(-64.0, edge), (64.0, edge), (0.0, far)]
    order = [0, 2, 1] if flip else [0, 1, 2]
    return R.flat(points, z), np.array([order], dtype=np.int32)
