"""K34 without a GPU: the numpy restatement (tests/mesh_aa_reference.py) held to closed forms, to the
cases the contract names and to a float64 model that shares no arithmetic with it; the host plumbing
against brute-force loops; the refusals; and ``antialias=False`` reaching nothing new."""

import numpy as np
import pytest
import torch

import fourier_feature_nets_amd as ffn
from fourier_feature_nets_amd import build, mesh, ops
from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
from tests import mesh_aa_reference as A
from tests import mesh_raster_reference as R
from tests import stream_order_cases_mesh_aa  # noqa: F401  (adds K34's stream-order cases)

U = 2.0 ** -24                      # the unit roundoff of f32


def opposites(triangles, num_vertices):
    return ffn.edge_opposites(triangles, num_vertices, "cpu").numpy()


def flat_frame(vertices, triangles, width, height, colors=None, background=(0, 0, 0)):
    colors = R.grey(vertices) if colors is None else colors
    fr = A.frame(vertices, triangles, R.PIXEL_PROJ, R.ORIGIN, width, height, colors,
                 background=background)
    opposite = opposites(triangles, len(vertices))
    return fr, opposite, A.decisions(fr, opposite)


# ------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("vertical", [True, False])
def test_a_half_plane_edge_gives_the_covered_length(vertical, flip):
    """Alpha 1 left of (above) an axis-parallel edge at x_e = j / 256: every input is a multiple
    of 1/256 px, so alpha = E / D is exact in f32 and so is every blend.  The sum of out_alpha
    over the row (column) is the covered length x_e + 0.5 for every j across two pixels; at
    k + 0.25 pixel k holds 0.75, at k + 0.75 pixel k + 1 holds 0.25, at k + 0.5 nothing changes."""
    width, height, k = (8, 3, 3) if vertical else (3, 8, 3)
    for j in range(256 * k, 256 * (k + 2) + 1):
        edge = j / 256.0
        vertices, triangles = A.half_plane(edge, vertical=vertical, flip=flip)
        fr, _, made = flat_frame(vertices, triangles, width, height)
        _, out_alpha = A.forward(fr, made)
        image = out_alpha.reshape(height, width)
        lines = image if vertical else image.T
        for line in lines:
            assert float(line.astype(np.float64).sum()) == edge + 0.5, (j, line)
        at = int(np.floor(edge))
        frac = edge - at
        if frac == 0.25:
            assert (lines[:, at] == np.float32(0.75)).all()
        if frac == 0.75:
            assert (lines[:, at + 1] == np.float32(0.25)).all()
        if frac == 0.5:
            assert np.array_equal(out_alpha, fr["alpha"])
            assert np.array_equal(A.forward(fr, made)[0], fr["color"])


def test_an_empty_image_and_a_pixel_in_no_pair_come_back_bit_for_bit():
    vertices, triangles = R.flat([(-30, -30), (-20, -30), (-25, -12)]), np.array([[0, 1, 2]], np.int32)
    fr, _, made = flat_frame(vertices, triangles, 7, 5, background=(0.25, 0.5, 0.75))
    assert all(pair is None for pair in made)
    color, alpha = A.forward(fr, made)
    assert np.array_equal(color, fr["color"]) and np.array_equal(alpha, fr["alpha"])
    vertices, triangles = R.quad_scene()
    fr, _, made = flat_frame(vertices, triangles, 14, 12)
    color, alpha = A.forward(fr, made)
    touched = {p for pair in made if pair is not None for p in (pair["target"],)}
    for p in range(14 * 12):
        if p not in touched:
            assert np.array_equal(color[p], fr["color"][p]) and alpha[p] == fr["alpha"][p]


def test_a_quad_changes_on_its_outline_only():
    """Two triangles that share the diagonal: no pair across the diagonal is active, and a pixel
    changes only if it or a 4-neighbour of it is uncovered."""
    vertices, triangles = R.quad_scene()
    width, height = 14, 12
    fr, opposite, made = flat_frame(vertices, triangles, width, height)
    assert sorted(opposite.tolist()) == [-1, -1, -1, -1, 1, 3]
    ids = fr["ids"]
    across = 0
    for p in range(width * height):
        for axis, q, exists in ((0, p + 1, p % width + 1 < width),
                                (1, p + width, p // width + 1 < height)):
            if exists and ids[p] >= 0 and ids[q] >= 0 and ids[p] != ids[q]:
                across += 1
                assert made[2 * p + axis] is None
    assert across > 5
    color, alpha = A.forward(fr, made)
    changed = np.flatnonzero((alpha != fr["alpha"]) | (color != fr["color"]).any(1))
    assert len(changed) > 10
    covered = (ids >= 0).reshape(height, width)
    padded = np.pad(covered, 1, constant_values=False)
    inner = (padded[1:-1, 1:-1] & padded[:-2, 1:-1] & padded[2:, 1:-1] & padded[1:-1, :-2]
             & padded[1:-1, 2:]).reshape(-1)
    outer = ~(padded[1:-1, 1:-1] | padded[:-2, 1:-1] | padded[2:, 1:-1] | padded[1:-1, :-2]
              | padded[1:-1, 2:]).reshape(-1)
    assert not inner[changed].any() and not outer[changed].any()


def _shared_edge_scene(third, z_third=1.0, extra=None):
    """Triangle 0 right of the vertical edge (4,4)-(4,12), triangle 1 on the same edge with its third
    vertex at ``third`` -> (vertices, triangles)."""
    points = [(4, 4), (4, 12), (12, 8)]
    vertices = np.concatenate([R.flat(points), R.flat([third], z_third)])
    triangles = [[0, 1, 2], [1, 0, 3]]
    if extra is not None:
        vertices = np.concatenate([vertices, R.flat([extra], 4.0)])
        triangles.append([0, 1, 4])
    return vertices.astype(np.float32), np.array(triangles, dtype=np.int32)


def _pairs_across_x(made, width, left, rows):
    return [made[2 * (y * width + left)] for y in rows]


def test_a_continuing_surface_is_no_silhouette_and_a_fold_is():
    width, height = 16, 16
    rows = range(6, 11)
    flat_v, flat_t = _shared_edge_scene((-4, 8))
    _, _, made = flat_frame(flat_v, flat_t, width, height)
    assert all(pair is None for pair in _pairs_across_x(made, width, 3, rows))
    # folded over: the neighbour's third vertex lies on triangle 0's own side, farther away
    fold_v, fold_t = _shared_edge_scene((10, 8), 2.0)
    fr, opposite, made = flat_frame(fold_v, fold_t, width, height)
    assert opposite[2] == 3                      # edge 2 of triangle 0 joins its corners 0 and 1
    for pair in _pairs_across_x(made, width, 3, rows):
        assert pair is not None and pair["f"] == 0 and pair["edge"] == 2
        assert pair["alpha"] == 0 and pair["target"] == pair["a"]


def test_boundary_and_non_manifold_edges_are_silhouettes():
    width, height = 16, 16
    rows = range(6, 11)
    vertices, triangles = _shared_edge_scene((-4, 8), extra=(-3, 9))
    fr, opposite, made = flat_frame(vertices, triangles, width, height)
    # three triangles on the edge: nobody has a single neighbour
    assert opposite[2] == -1 and opposite[3 + 2] == -1 and opposite[6 + 2] == -1
    for pair in _pairs_across_x(made, width, 3, rows):
        assert pair is not None and pair["edge"] == 2 and pair["f"] in (0, 1)
    # an open mesh: one triangle, every edge a boundary
    one_v, one_t = R.flat([(4, 4), (4, 12), (12, 8)]), np.array([[0, 1, 2]], np.int32)
    _, opposite, made = flat_frame(one_v, one_t, width, height)
    assert (opposite == -1).all()
    assert all(pair is not None for pair in _pairs_across_x(made, width, 3, rows))


def test_a_neighbour_behind_the_camera_fails_the_attempt():
    width, height = 16, 16
    vertices, triangles = _shared_edge_scene((10, 8), -1.0)
    fr, opposite, made = flat_frame(vertices, triangles, width, height)
    assert fr["state"]["status"][1] == R.CLIPPED and opposite[2] == 3
    assert all(pair is None for pair in _pairs_across_x(made, width, 3, range(6, 11)))
    # triangle 0's other edges are boundaries and stay silhouettes
    assert sum(pair is not None and pair["edge"] != 2 for pair in made) > 4


def test_a_slanted_near_triangle_hands_the_pair_to_the_far_one():
    """Triangle 0 recedes with x and covers both centres; it wins pixel (8, y) and loses (9, y) to
    triangle 1, whose edge x = 8.5 lies between them: the first attempt (from the nearer key, triangle
    0) fails because it covers both centres, the second one, from the far pixel, decides."""
    def at(x, y, z):
        return [x * z, y * z, z]
    vertices = np.array([at(0, 0, 1), at(20, 0, 3), at(0, 20, 1),
                         at(8.5, -30, 1.4), at(40, 8, 1.4), at(8.5, 40, 1.4)], dtype=np.float32)
    triangles = np.array([[0, 1, 2], [3, 4, 5]], dtype=np.int32)
    width, height = 16, 8
    fr, _, made = flat_frame(vertices, triangles, width, height)
    y = 3
    p, q = y * width + 8, y * width + 9
    assert fr["ids"][p] == 0 and fr["ids"][q] == 1 and int(fr["zbuf"][p]) < int(fr["zbuf"][q])
    pair = made[2 * p]
    assert pair is not None and pair["f"] == 1 and pair["a"] == q and pair["b"] == p
    assert pair["alpha"] == np.float32(0.5) and pair["m"] == 0


# ------------------------------------------------------------------------------- float64 model
SCENES = [(401, 10, 24, 20), (402, 14, 21, 17), (403, 12, 33, 13)]


def _perspective(seed, count, width, height):
    vertices, triangles, colors, _ = R.scene(seed, count)
    cam = R.camera(width, height)
    proj = projection_matrices([cam])[0]
    eye = eye_positions([cam], (0.0, 0.0, 0.0))[0]
    rng = np.random.default_rng(seed + 1)
    g_color = rng.uniform(-1, 1, (width * height, 3)).astype(np.float32)
    g_alpha = rng.uniform(-1, 1, width * height).astype(np.float32)
    opposite = opposites(triangles, len(vertices))
    out = A.geometry_backward(vertices, triangles, proj, eye, width, height, colors, opposite,
                              g_color, g_alpha)
    return vertices, triangles, proj, A.channels(g_color, g_alpha).astype(np.float64), out


def _pair_terms(fr, pair, g):
    """What the budget of one pair's entries needs, in float64 -> (R, C, D in px, c_j, c_k)."""
    values = A.channels(fr["color"], fr["alpha"]).astype(np.float64)
    t = pair["target"]
    g_abs = float((np.abs(g[t]) * np.abs(values[pair["source"]] - values[t])).sum())
    d = float(pair["d"])
    width = fr["width"]
    a = np.array([pair["a"] % width, pair["a"] // width], dtype=np.float64) * 256
    b = np.array([pair["b"] % width, pair["b"] // width], dtype=np.float64) * 256
    crossing = a + float(pair["alpha"]) * (b - a)
    state, f = fr["state"], pair["f"]
    j, k = (pair["edge"] + 1) % 3, (pair["edge"] + 2) % 3
    vj = np.array([state["X"][f][j], state["Y"][f][j]], dtype=np.float64)
    vk = np.array([state["X"][f][k], state["Y"][f][k]], dtype=np.float64)
    return 256 * g_abs / d, np.abs(crossing).max(), d / 65536.0, crossing - vj, crossing - vk


def _entry_budget(fr, pair, g, step):
    """The bound on |f32 entry - float64 derivative| for the two entries of ``pair`` -> (2,2).

    Counting roundings, with u = 2^-24, Gabs = sum_c |g_c| |delta_c| and R = 256 Gabs / D:
      G:      one rounded subtraction per delta, one product per channel and three adds, each at
              most u of a partial sum bounded by Gabs: |err G| <= 6 u Gabs;
      r256:   the conversion of D, one division, an exact scaling: |err r256| <= 9 u R (with G's);
      alpha:  two conversions and a division: 3 u alpha, alpha <= 1;  alpha * 256 is exact;
      C:      one add, u |C|;   c = C - V: one subtraction, u |c| (V and Q are integers below
              2^24, exact as floats): |err c| <= u (768 + |C| + |c|), in 1/256 px;
      entry:  one product: |err| <= R u (768 + |C| + |c|) + 9 u R |c| + u R |c|
                                 = u R (768 + |C| + 11 |c|).
    Doubled for the second-order terms.  The model's central difference of alpha -- a ratio of
    two functions linear in the moved coordinate, whose denominator D (in px^2 per px) changes by
    at most 1 per px -- is off by the factor 1 / (1 - (h / D)^2) exactly: the term
    2 (h / D)^2 |entry| is added for it (D in px, the edge's extent across the pair)."""
    scale, crossing, d_px, cj, ck = _pair_terms(fr, pair, g)
    out = np.empty((2, 2))
    for row, c in enumerate((cj, ck)):                  # entry 0 uses c_j, entry 1 uses c_k
        for col in range(2):
            size = abs(c[1 - col])
            # (scale * size bounds |entry|: C, c in 1/256 px, D in their squares, the entry per px)
            out[row, col] = 2 * U * scale * (768 + crossing + 11 * size) \
                + 2 * (step / d_px) ** 2 * scale * size
    return out


def _pair_loss64(fr, pair, screen, g):
    values = A.channels(fr["color"], fr["alpha"]).astype(np.float64)
    t = A.crossing64(fr, pair, screen)
    weight = t - 0.5 if pair["target"] == pair["b"] else 0.5 - t
    return weight * float((g[pair["target"]] * (values[pair["source"]] - values[pair["target"]])).sum())


@pytest.mark.parametrize("seed,count,width,height", SCENES)
def test_pair_gradients_are_the_central_differences_of_the_model(seed, count, width, height):
    """Every entry K34b's restatement writes, against the central difference (h = 1e-6 px) of the
    float64 model of that pair alone in the screen position of the entry's vertex, at the snapped
    positions and with the decisions frozen, within ``_entry_budget`` (derived there).  Worst use of
    the budget observed: 0.245 (seed 401), 0.220 (402), 0.192 (403)."""
    _, _, _, g, (_, _, _, fr, made, (entry_vertex, entry_grad)) = _perspective(seed, count, width,
                                                                             height)
    screen = A.snapped_screen(fr)
    step = 1e-6
    worst, seen = 0.0, 0
    for slot, pair in enumerate(made):
        if pair is None:
            continue
        budget = _entry_budget(fr, pair, g, step)
        for row in range(2):
            v = entry_vertex[2 * slot + row]
            for col in range(2):
                moved = screen.copy()
                moved[v, col] += step
                up = _pair_loss64(fr, pair, moved, g)
                moved[v, col] -= 2 * step
                down = _pair_loss64(fr, pair, moved, g)
                want = (up - down) / (2 * step)
                got = float(entry_grad[2 * slot + row][col])
                # the roundoff of the difference itself: two losses of this size over 2 h
                noise = 4 * np.finfo(np.float64).eps * max(abs(up), abs(down)) / step
                use = abs(got - want) / (budget[row, col] + noise)
                worst = max(worst, use)
                seen += 1
    print("pair gradients: %d entries, worst use of the budget %.3f" % (seen, worst))
    assert seen > 100 and worst <= 1.0


def _vertex_budget(fr, made, g, entry_vertex, entry_grad, vertices, proj, step):
    """The bound on |f32 grad[v][c] - float64 derivative| -> (V,3).

    grad[v][c] = ((gx J0c) + (gy J1c)) / w with J0c = P0c - sx P2c.  With n the entries of v and
    ax = sum |entry_x|: gx carries the entries' own budgets (``_entry_budget`` without the
    central-difference term) and (n - 1) u ax of its n - 1 adds.  x, y, w are three products and
    three adds each, at most 4 u of their absolute sums X, Y, W;  sx = x / w adds u:
    |err sx| <= |sx| u (4 X / |x| + 4 W / |w| + 1).  J0c: a product and a subtraction,
    |err J0c| <= |P2c| |err sx| + u |sx P2c| + u |J0c|.  The term gx J0c: one product; the sum and
    the division by the rounded w: u (2 + 4 W / |w|) of |gx J0c| + |gy J1c|.  Everything / w, and
    doubled for the second-order terms.  The model's difference moves the vertex by h in 3-D;
    the screen moves by at most h (|P0c| + |sx| |P2c|) / w px, and the pairs' central-difference
    term is taken with that step."""
    p = np.asarray(proj, dtype=np.float64).reshape(3, 4)
    pos = np.asarray(vertices, dtype=np.float64)
    terms = np.abs(pos[:, None, :] * p[None, :, :3])
    absolute = terms.sum(2) + np.abs(p[None, :, 3])            # X, Y, W per vertex
    homog = pos @ p[:, :3].T + p[:, 3]
    sx, sy, w = homog[:, 0] / homog[:, 2], homog[:, 1] / homog[:, 2], homog[:, 2]
    cond_w = absolute[:, 2] / np.abs(w)
    err_s = [np.abs(s) * U * (4 * absolute[:, i] / np.abs(homog[:, i]) + 4 * cond_w + 1)
             for i, s in enumerate((sx, sy))]
    count = np.zeros(len(pos))
    total = np.zeros((len(pos), 2))
    own = np.zeros((len(pos), 2))
    steps = np.zeros((len(pos), 2))
    for slot, pair in enumerate(made):
        if pair is None:
            continue
        rounding = _entry_budget(fr, pair, g, 0.0)
        d_px = float(pair["d"]) / 65536.0
        for row in range(2):
            v = entry_vertex[2 * slot + row]
            count[v] += 1
            total[v] += np.abs(entry_grad[2 * slot + row].astype(np.float64))
            own[v] += rounding[row]
            steps[v] += 2 * np.abs(entry_grad[2 * slot + row].astype(np.float64)) / d_px ** 2
    out = np.zeros((len(pos), 3))
    for c in range(3):
        jac = [p[0, c] - sx * p[2, c], p[1, c] - sy * p[2, c]]
        err_jac = [np.abs(p[2, c]) * err_s[i] + U * np.abs((sx, sy)[i] * p[2, c]) + U * np.abs(jac[i])
                   for i in range(2)]
        moved = step * (np.abs(p[0, c]) + np.abs(p[1, c]) + (np.abs(sx) + np.abs(sy)) * np.abs(p[2, c])) \
            / np.abs(w)
        bound = np.zeros(len(pos))
        size = np.zeros(len(pos))
        for i in range(2):
            bound += (own[:, i] + np.maximum(count - 1, 0) * U * total[:, i]) * np.abs(jac[i]) \
                + total[:, i] * err_jac[i] + U * total[:, i] * np.abs(jac[i]) \
                + steps[:, i] * moved ** 2 * np.abs(jac[i])
            size += total[:, i] * np.abs(jac[i])
        bound += U * (2 + 4 * cond_w) * size
        # the projection's own curvature under the central difference: (h |P2| / w)^2 of the size
        bound += 4 * (step * np.abs(p[2, :3]).sum() / np.abs(w)) ** 2 * size
        out[:, c] = 2 * bound / np.abs(w)
    return out


@pytest.mark.parametrize("seed,count,width,height", SCENES)
def test_the_vertex_gradient_is_the_central_difference_of_the_model(seed, count, width, height):
    """K34c's restatement against central differences (h = 1e-6 scene units) of the float64 model
    in the 3-D positions: the screen position of a vertex is its snapped one plus what the float64
    projection moves by (the snap passed straight through), decisions frozen.  Within
    ``_vertex_budget`` (derived there).  Worst use of the budget observed: 0.031 (seed 401), 0.032
    (402), 0.040 (403)."""
    vertices, _, proj, g, (grad, _, _, fr, made, (entry_vertex, entry_grad)) = _perspective(
        seed, count, width, height)
    step = 1e-6
    budget = _vertex_budget(fr, made, g, entry_vertex, entry_grad, vertices, proj, step)
    base = A.snapped_screen(fr)
    pos = vertices.astype(np.float64)
    origin = A.screen64(proj, pos)
    used = sorted(set(entry_vertex[entry_vertex < len(vertices)].tolist()))
    assert len(used) > 10
    worst = 0.0
    for v in used:
        for c in range(3):
            values = []
            for sign in (1, -1):
                moved = pos[v].copy()
                moved[c] += sign * step
                screen = base.copy()
                screen[v] = base[v] + (A.screen64(proj, moved[None])[0] - origin[v])
                values.append(A.loss64(fr, made, screen, g))
            want = (values[0] - values[1]) / (2 * step)
            noise = 4 * np.finfo(np.float64).eps * max(abs(values[0]), abs(values[1])) / step
            worst = max(worst, abs(float(grad[v][c]) - want) / (budget[v, c] + noise))
    untouched = np.setdiff1d(np.arange(len(vertices)), used)
    assert not grad[untouched].any()
    print("vertex gradient: %d vertices, worst use of the budget %.3f" % (len(used), worst))
    assert worst <= 1.0


@pytest.mark.parametrize("seed,count,width,height", SCENES)
def test_adjoint_identity_of_the_image_transpose(seed, count, width, height):
    """<J delta, g> == <delta, J^T g> in float64 on the restatement's decisions, J^T gathered pixel
    by pixel as K34b gathers it; and the f32 restatement's d is J^T g to f32 roundoff."""
    _, _, _, g, (_, d_color, d_alpha, fr, made, _) = _perspective(seed, count, width, height)
    rng = np.random.default_rng(seed + 2)
    delta = rng.uniform(-1, 1, g.shape)
    left = float((A.forward64(made, delta) * g).sum())
    back = A.transpose64(made, g, width, height)
    right = float((delta * back).sum())
    assert abs(left - right) <= 1e-12 * (np.abs(delta).sum() + 1)
    # at most four pairs per pixel, two roundings each, on values below 1 + 4 * 0.5 * 1
    assert np.abs(A.channels(d_color, d_alpha) - back).max() <= 8 * U * 3
    assert sum(pair is not None for pair in made) > 50


# ------------------------------------------------------------------------------- K34d and plumbing
def test_the_laplacian_of_a_path_and_of_a_tetrahedron():
    n = 7
    x = np.stack([np.arange(n) ** 2, 3 * np.arange(n), np.ones(n)], 1).astype(np.float32)
    starts = np.concatenate([[0], np.cumsum([1] + [2] * (n - 2) + [1])]).astype(np.int32)
    neighbors = np.array([1] + sum([[i - 1, i + 1] for i in range(1, n - 1)], []) + [n - 2],
                         dtype=np.int32)
    got = A.laplacian(x, starts, neighbors, 0.5)
    want = np.zeros_like(x)
    want[1:-1] = 2 * x[1:-1] - x[:-2] - x[2:]
    want[0], want[-1] = x[0] - x[1], x[-1] - x[-2]
    assert np.array_equal(got, np.float32(0.5) * want)       # small integers: exact
    assert (got[1:-1, 0] == -1).all() and not got[1:-1, 1:].any()
    tetra = np.array([[0, 1, 2], [0, 3, 1], [1, 3, 2], [0, 2, 3]], dtype=np.int32)
    starts, neighbors = [t.numpy() for t in ffn.vertex_neighbors(tetra, 4, "cpu")]
    assert starts.tolist() == [0, 3, 6, 9, 12]
    x = np.array([[1, 0, 0], [0, 2, 0], [0, 0, 4], [8, 8, 8]], dtype=np.float32)
    got = A.laplacian(x, starts, neighbors, 1.0)
    assert np.array_equal(got, 4 * x - x.sum(0))
    again = A.laplacian(x, starts, neighbors, 2.0, out=got)
    assert np.array_equal(again, 3 * (4 * x - x.sum(0)))
    # an id outside 0 .. V - 1 is skipped
    assert np.array_equal(A.laplacian(x, np.array([0, 2, 2, 2, 2], np.int32),
                                      np.array([7, 1], np.int32), 1.0)[0], x[0] - x[1])


def _meshes():
    rng = np.random.default_rng(7)
    torus = ffn.procedural_torus(6, 5, 8)
    fan = np.array([[0, i, i + 1] for i in range(1, 9)], dtype=np.int32)
    return [("quad", R.quad_scene()[1], 4), ("torus", np.asarray(torus[1]), len(torus[0])),
            ("fan", fan, 11), ("random", rng.integers(0, 9, (20, 3)).astype(np.int32), 9),
            ("degenerate", np.array([[0, 0, 1], [1, 0, 2], [2, 2, 2], [0, 1, 2], [5, -3, 99]],
                                    np.int32), 6)]


@pytest.mark.parametrize("name,triangles,num_vertices", _meshes(), ids=[m[0] for m in _meshes()])
def test_the_plumbing_is_the_brute_force_loops(name, triangles, num_vertices):
    got = ffn.edge_opposites(triangles, num_vertices, "cpu")
    assert got.dtype == torch.int32 and got.shape == (3 * len(triangles),)
    assert np.array_equal(got.numpy(), A.opposites_brute(triangles, num_vertices))
    starts, neighbors = ffn.vertex_neighbors(torch.from_numpy(triangles), num_vertices, "cpu")
    want_starts, want_neighbors = A.neighbors_brute(triangles, num_vertices)
    assert starts.dtype == torch.int32 and neighbors.dtype == torch.int32
    assert np.array_equal(starts.numpy(), want_starts)
    assert np.array_equal(neighbors.numpy(), want_neighbors)
    if name == "torus":
        assert (got.numpy() >= 0).sum() > len(triangles)     # (its UV seams are boundaries)


def test_the_plumbing_refuses_bad_arguments():
    for function in (ffn.edge_opposites, ffn.vertex_neighbors):
        for bad in (np.zeros((2, 4), np.int32), np.zeros((2, 3), np.float32), np.zeros((0, 3), np.int32)):
            with pytest.raises(ValueError, match="triangles"):
                function(bad, 4, "cpu")
        with pytest.raises(ValueError, match="num_vertices"):
            function(np.zeros((2, 3), np.int32), 0, "cpu")


# ------------------------------------------------------------------------------- host
def _fake_raster(record=False):
    def fake(vertices, triangles, proj, eye, width, height, *rest):
        n = width * height
        out = (torch.zeros((n, 3)), torch.zeros(n), torch.zeros(n),
               torch.full((n,), -1, dtype=torch.int32),
               torch.zeros(len(triangles), dtype=torch.uint8), 0)
        if record:
            return (torch.zeros((len(triangles), 16), dtype=torch.int32),) + out \
                + (torch.full((n,), -1, dtype=torch.int64),)
        return out
    return fake


def test_antialias_false_never_reaches_the_new_ops(monkeypatch):
    def boom(*args, **kwargs):
        raise AssertionError("K34 was reached")
    for name in ("mesh_aa_forward", "mesh_aa_backward", "mesh_aa_vertex_grad", "mesh_laplacian"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(mesh, "edge_opposites", boom)
    monkeypatch.setattr(mesh, "_rasterize_z", boom)
    monkeypatch.setattr(mesh, "rasterize_mesh", _fake_raster())
    vertices, triangles = R.quad_scene()
    cam = R.camera(6, 5)
    out, report = ffn.render_mesh(vertices, triangles, cam, colors=R.grey(vertices), device="cpu")
    assert out.alpha.shape == (30,) and report["drawn"] == 2
    out, _ = ffn.render_mesh(vertices, triangles, cam, colors=R.grey(vertices), device="cpu",
                             antialias=False, supersample=2)
    assert out.alpha.shape == (30,)
    # and True does reach them, after K31, on the sub-pixel image
    seen = {}
    monkeypatch.undo()
    monkeypatch.setattr(mesh, "_rasterize_z", _fake_raster(record=True))

    def forward(record, zbuf, ids, opposite, vertices, proj, color, alpha, width, height):
        seen.update(width=width, height=height, opposite=tuple(opposite.shape))
        return color + 0.5, alpha + 0.25
    monkeypatch.setattr(ops, "mesh_aa_forward", forward)
    out, _ = ffn.render_mesh(vertices, triangles, cam, colors=R.grey(vertices), device="cpu",
                             antialias=True, supersample=2)
    assert seen == dict(width=12, height=10, opposite=(6,))
    assert (out.alpha == 0.25).all() and (out.color == 0.5).all()


def _frame_args(width=6, height=5, faces=2, num_vertices=4):
    n = width * height
    return dict(record=torch.zeros((faces, 16), dtype=torch.int32),
                zbuf=torch.zeros(n, dtype=torch.int64), ids=torch.zeros(n, dtype=torch.int32),
                opposite=torch.zeros(3 * faces, dtype=torch.int32),
                vertices=torch.zeros((num_vertices, 3)), proj=np.eye(4, dtype=np.float32)[:3],
                color=torch.zeros((n, 3)), alpha=torch.zeros(n), width=width, height=height)


def _refused(name, function, args, **change):
    with pytest.raises(ValueError, match=name):
        function(**dict(args, **change))


def test_the_ops_refuse_by_name():
    args = _frame_args()
    ops.mesh_aa_forward_check(**args)
    forward = ops.mesh_aa_forward_check
    _refused("record", forward, args, record=args["record"][:, :12])
    _refused("zbuf", forward, args, zbuf=args["zbuf"].to(torch.int32))
    _refused("ids", forward, args, ids=args["ids"][:-1])
    _refused("opposite", forward, args, opposite=args["opposite"][:-1])
    _refused("vertices", forward, args, vertices=args["vertices"].double())
    _refused("color", forward, args, color=args["color"][:, :2])
    _refused("alpha", forward, args, alpha=args["alpha"].reshape(-1, 1))
    _refused("proj", forward, args, proj=np.eye(4))
    _refused("proj", forward, args, proj=np.full((3, 4), np.nan))
    _refused("width", forward, args, width=0)
    back = dict(args, triangles=torch.zeros((2, 3), dtype=torch.int32),
                g_color=torch.zeros((30, 3)), g_alpha=torch.zeros(30))
    ops.mesh_aa_backward_check(**back)
    _refused("triangles", ops.mesh_aa_backward_check, back, triangles=back["triangles"][:1])
    _refused("g_color", ops.mesh_aa_backward_check, back, g_color=back["g_color"][:-1])
    _refused("g_alpha", ops.mesh_aa_backward_check, back, g_alpha=back["g_alpha"].double())
    vertex = dict(sorted_vertex=torch.zeros(120, dtype=torch.int32),
                  order=torch.zeros(120, dtype=torch.int32), entry_grad=torch.zeros((120, 2)),
                  vertices=torch.zeros((4, 3)), proj=args["proj"])
    ops.mesh_aa_vertex_grad_check(**vertex)
    check = ops.mesh_aa_vertex_grad_check
    _refused("entry_grad", check, vertex, entry_grad=torch.zeros((118, 2)),
             sorted_vertex=torch.zeros(118, dtype=torch.int32), order=torch.zeros(118, dtype=torch.int32))
    _refused("sorted_vertex", check, vertex, sorted_vertex=vertex["sorted_vertex"].long())
    _refused("order", check, vertex, order=vertex["order"][:-4])
    _refused("grad", check, vertex, grad=torch.zeros((5, 3)))
    _refused("accumulate", check, vertex, accumulate=True)
    lap = dict(values=torch.zeros((4, 3)), neighbor_starts=torch.zeros(5, dtype=torch.int32),
               neighbors=torch.zeros(6, dtype=torch.int32), scale=1.0)
    assert ops.mesh_laplacian_check(**lap) == 1.0
    _refused("values", ops.mesh_laplacian_check, lap, values=torch.zeros((4, 2)))
    _refused("neighbor_starts", ops.mesh_laplacian_check, lap, neighbor_starts=lap["neighbor_starts"][:-1])
    _refused("neighbors", ops.mesh_laplacian_check, lap, neighbors=lap["neighbors"].long())
    _refused("scale", ops.mesh_laplacian_check, lap, scale=float("nan"))
    _refused("out", ops.mesh_laplacian_check, lap, out=torch.zeros((3, 3)))
    _refused("accumulate", ops.mesh_laplacian_check, lap, accumulate=True)


def test_the_host_functions_refuse_before_the_device(monkeypatch):
    def boom(*args, **kwargs):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mesh, "_rasterize_z", boom)
    monkeypatch.setattr(mesh, "_mesh_on", boom)
    vertices, triangles = R.quad_scene()
    colors = R.grey(vertices)
    cam = R.camera(6, 5)
    back = ffn.render_mesh_geometry_backward
    good = (np.zeros((30, 3), np.float32), np.zeros(30, np.float32))
    with pytest.raises(ValueError, match="vertices"):
        back(vertices[:, :2], triangles, cam, colors, *good)
    with pytest.raises(ValueError, match="colors"):
        back(vertices, triangles, cam, None, *good)
    with pytest.raises(ValueError, match="d_color"):
        back(vertices, triangles, cam, colors, good[0][:-1], good[1])
    with pytest.raises(ValueError, match="d_alpha"):
        back(vertices, triangles, cam, colors, good[0], good[1][:-1])
    with pytest.raises(ValueError, match="accumulate"):
        back(vertices, triangles, cam, colors, *good, accumulate=True)
    with pytest.raises(ValueError, match="background"):
        back(vertices, triangles, cam, colors, *good, background=(0, 0))
    with pytest.raises(ValueError, match="triangles"):
        back(vertices, triangles + 9, cam, colors, *good)

    class Data:
        images = np.zeros((2, 5, 6, 4), np.uint8)
        cameras = [cam, cam]
        color_space = "RGB"
    fit = ffn.fit_mesh_geometry
    with pytest.raises(ValueError, match="colors"):
        fit(vertices, triangles, None, Data())
    with pytest.raises(ValueError, match="learning_rate"):
        fit(vertices, triangles, colors, Data(), learning_rate=0.0)
    with pytest.raises(ValueError, match="num_steps"):
        fit(vertices, triangles, colors, Data(), num_steps=-1)
    with pytest.raises(ValueError, match="alpha_weight"):
        fit(vertices, triangles, colors, Data(), alpha_weight=-1.0)
    with pytest.raises(ValueError, match="laplacian_weight"):
        fit(vertices, triangles, colors, Data(), laplacian_weight=float("nan"))
    with pytest.raises(ValueError, match="max_displacement"):
        fit(vertices, triangles, colors, Data(), max_displacement=0.0)
    with pytest.raises(ValueError, match="train_dataset"):
        fit(vertices, triangles, colors, object())
    with pytest.raises(ValueError, match="triangles"):
        fit(vertices, triangles + 9, colors, Data())


def test_the_new_names_are_built_declared_and_exported():
    assert build.SOURCES["mesh_aa.hip"] == ["-ffp-contract=off"]
    from fourier_feature_nets_amd import _lib
    declared = set(_lib.declared_symbols())
    for name in ("ffn_mesh_aa_forward", "ffn_mesh_aa_backward", "ffn_mesh_aa_vertex_grad",
                 "ffn_mesh_laplacian"):
        assert name in declared
    import fourier_feature_nets as alias
    for name in ("edge_opposites", "vertex_neighbors", "render_mesh_geometry_backward",
                 "fit_mesh_geometry"):
        assert name in ffn.__all__ and getattr(alias, name) is getattr(mesh, name)


def test_the_stream_order_cases_are_registered():
    from tests.stream_order_cases import CASES
    reached = {entry for case in CASES for entry in case.reaches}
    for name in ("mesh_aa_forward", "mesh_aa_backward", "mesh_aa_vertex_grad", "mesh_laplacian"):
        assert "ffn_" + name in reached
