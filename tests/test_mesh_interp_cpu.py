"""K35 without a GPU: the numpy restatement (tests/mesh_interp_reference.py) held to central
differences of a float64 model that shares no code with it, within budgets counted from the f32
roundings of the contract; to closed forms; to the case the feature exists for (a visible vertex on
no outline); and the plumbing: the names, ``interior=False`` reaching nothing new, the refusals."""

import numpy as np
import pytest
import torch

import fourier_feature_nets_amd as ffn
from fourier_feature_nets_amd import build, mesh, ops
from fourier_feature_nets_amd.cameras import eye_positions, projection_matrices
from tests import mesh_aa_reference as A
from tests import mesh_interp_reference as I
from tests import mesh_raster_reference as R
from tests import refusal_cases_mesh_interp  # noqa: F401  (adds K35's refusal rows)
from tests import stream_order_cases_mesh_interp  # noqa: F401  (adds K35's stream-order cases)

U = 2.0 ** -24                      # the unit roundoff of f32
EPS = np.finfo(np.float64).eps
STEP = 1e-6


# ------------------------------------------------------------------------------- the budget
def _pixel_budget(state, f, colors, px, py, g, step):
    """Per selected pixel of triangle ``f`` -> (bound (n,9), size (n,9)): the bound on |f32 term -
    real term| and a bound on |real term|, both in float64 from the exact integers of the record.

    Counting roundings, u = 2^-24, every bound to first order (the caller doubles the sum):
      lambda_i  two conversions and a division: 3 u;   q_i = lambda_i / w_i: 4 u
      depth_w   the q_i are >= 0 at a covered pixel, two adds: 6 u; the reciprocal: 7 u
      b_i       q_i depth_w: 12 u, and sum b_i = 1
      C_ch      three products, two adds of terms bounded by Cabs_ch = sum_i |c_i| b_i: 15 u Cabs_ch
      c_i - C   one subtraction: 15 u Cabs_ch + u |c_i - C|
      a_i       three products, two adds: sum_ch |g_ch| (15 u Cabs_ch + 4 u |c_i - C|_ch)
      r_i       (a_i depth_w) / w_i, s_i = depth_w / w_i: 7 u + 2 u more of Aabs_i =
                sum_ch |g_ch| |c_i - C|_ch:  err r_i = s_i sum_ch |g_ch| (15 u Cabs_ch + 13 u |c_i - C|_ch),
                |r_i| <= Rabs_i = s_i Aabs_i
      n_i       dx_i is an integer below 2^24 and 256 dx_i is exact; the conversion of |A| and the
                division: 2 u
      G         three products, two adds: err G = sum_i |n_i| (err r_i + 5 u Rabs_i),
                |G| <= Gabs = sum_i |n_i| Rabs_i
      t         -(lambda_j G): lambda_j (err G + 4 u Gabs), |t| <= lambda_j Gabs;
                -(r_j q_j):    q_j (err r_j + 5 u Rabs_j), |t| <= q_j Rabs_j.
    The model's central difference: with the ids frozen the colour of a pixel is (N0 + N1 t) /
    (D0 + D1 t) along any line of one corner's screen position (the area cancels in sum c q / sum
    q) and in one corner's w, and the central difference of such a function is its derivative times
    1 / (1 - (h D1 / D0)^2) exactly.  |D1 / D0| <= 3 rho / alt in the screen (alt the smallest
    altitude of the triangle in pixels, rho = w_max / w_min) and <= 1 / w_j in w_j: the terms
    2 (3 h rho / alt)^2 |t| and 2 (h / w_j)^2 |t| are added for it."""
    x = state["X"][f].astype(np.float64) / 256.0
    y = state["Y"][f].astype(np.float64) / 256.0
    w = state["w"][f].astype(np.float64)
    c = np.asarray(colors, dtype=np.float64)[state["ids"][f]]
    g = np.abs(np.asarray(g, dtype=np.float64))
    area = (x[1] - x[0]) * (y[2] - y[0]) - (y[1] - y[0]) * (x[2] - x[0])
    sign = -1.0 if area < 0 else 1.0
    lam, normal, longest = [], [], 0.0
    for i in range(3):
        j, k = (i + 1) % 3, (i + 2) % 3
        lam.append(sign * ((x[k] - x[j]) * (py - y[j]) - (y[k] - y[j]) * (px - x[j])) / abs(area))
        normal.append(np.abs([y[k] - y[j], x[k] - x[j]]) / abs(area))
        longest = max(longest, np.hypot(x[k] - x[j], y[k] - y[j]))
    lam = np.stack(lam, -1)                                         # (n,3)
    q = lam / w
    depth = 1.0 / q.sum(-1)
    b = q * depth[:, None]
    c_abs = b @ np.abs(c)                                           # (n,3 channels)
    diff = np.abs(c[None, :, :] - (b @ c)[:, None, :])              # (n, corner, channel)
    a_abs = (g[:, None, :] * diff).sum(-1)                          # (n,3)
    s = depth[:, None] / w
    r_abs = s * a_abs
    err_r = s * (g[:, None, :] * (15 * U * c_abs[:, None, :] + 13 * U * diff)).sum(-1)
    bound, size = np.zeros((len(lam), 9)), np.zeros((len(lam), 9))
    altitude = abs(area) / longest
    rho = w.max() / w.min()
    for axis in range(2):
        n_abs = np.array([normal[i][axis] for i in range(3)])
        g_abs = (r_abs * n_abs).sum(-1)
        err_g = ((err_r + 5 * U * r_abs) * n_abs).sum(-1)
        for j in range(3):
            size[:, 3 * j + axis] = lam[:, j] * g_abs
            bound[:, 3 * j + axis] = lam[:, j] * (err_g + 4 * U * g_abs) \
                + 2 * (3 * step * rho / altitude) ** 2 * size[:, 3 * j + axis]
    for j in range(3):
        size[:, 3 * j + 2] = q[:, j] * r_abs[:, j]
        bound[:, 3 * j + 2] = q[:, j] * (err_r[:, j] + 5 * U * r_abs[:, j]) \
            + 2 * (step / w[j]) ** 2 * size[:, 3 * j + 2]
    return bound, size


def _entry_budget(state, f, ids, colors, d_color, width, height, step):
    """The bound on |f32 face_grads[f] - the float64 derivative| -> (9,), and the sum of the sizes.
    Every term passes the six adds of the fold and one add per segment, D = 6 + ceil(n / 64) in
    all, each at most u of the sum of the sizes (adding a +0 is exact); doubled for the
    second-order terms."""
    n, chosen, px, py, pixel = I.selected(state, f, ids, width, height)
    bound, size = _pixel_budget(state, f, colors, px.astype(np.float64), py.astype(np.float64),
                                np.asarray(d_color)[pixel], step)
    depth = 6 + (n + 63) // 64
    return 2 * (bound.sum(0) + depth * U * size.sum(0)), size.sum(0)


def _vertex_budget(state, ids, colors, d_color, width, height, grads, triangles, vertices, proj,
                   step):
    """The bound on |f32 grad[v][c] - float64 derivative| -> (V,3).

    grad[v][c] = ((gx J0c) + (gy J1c)) / w + gw P2c with J0c = P0c - sx P2c.  With n the corners of
    v and a = sum |entry|: gx, gy, gw carry the entries' own budgets (``_entry_budget``) and
    (n - 1) u a of their n - 1 adds.  x, y, w are three products and three adds each, at most 4 u
    of their absolute sums X, Y, W; sx = x / w adds u: |err sx| <= |sx| u (4 X / |x| + 4 W / |w| +
    1).  J0c: a product and a subtraction, |err J0c| <= |P2c| |err sx| + u |sx P2c| + u |J0c|.
    The term gx J0c: one product; the sum and the division by the rounded w: u (2 + 4 W / |w|) of
    |gx J0c| + |gy J1c|; all of that / w.  gw P2c: one product, and the last add one more u of both
    halves.  Doubled for the second-order terms.  The model's difference moves the vertex by h in
    3-D: the screen moves by at most h (|P0c| + |P1c| + (|sx| + |sy|) |P2c|) / w px and w by
    h |P2c|, the entries' central-difference terms are taken with the larger of the two, and the
    projection's own curvature adds (h |P2| / w)^2 of the size (as for K34c)."""
    p = np.asarray(proj, dtype=np.float64).reshape(3, 4)
    pos = np.asarray(vertices, dtype=np.float64)
    absolute = np.abs(pos[:, None, :] * p[None, :, :3]).sum(2) + np.abs(p[None, :, 3])
    homog = pos @ p[:, :3].T + p[:, 3]
    sx, sy, w = homog[:, 0] / homog[:, 2], homog[:, 1] / homog[:, 2], homog[:, 2]
    cond_w = absolute[:, 2] / np.abs(w)
    err_s = [np.abs(s) * U * (4 * absolute[:, i] / np.abs(homog[:, i]) + 4 * cond_w + 1)
             for i, s in enumerate((sx, sy))]
    moved = step * max(1.0, float(((np.abs(p[0, :3]) + np.abs(p[1, :3])).max()
                                   + (np.abs(sx) + np.abs(sy)).max() * np.abs(p[2, :3]).max())
                                  / np.abs(w).min()), float(np.abs(p[2, :3]).max()))
    count = np.zeros(len(pos))
    total, own = np.zeros((len(pos), 3)), np.zeros((len(pos), 3))
    corners = state["ids"]
    for f in np.unique(ids[ids >= 0]):
        budget, _ = _entry_budget(state, f, ids, colors, d_color, width, height, moved)
        for j in range(3):
            own[corners[f][j]] += budget[3 * j:3 * j + 3]
    for f in range(len(corners)):
        for j in range(3):
            count[corners[f][j]] += 1
            total[corners[f][j]] += np.abs(grads[f][3 * j:3 * j + 3].astype(np.float64))
    summed = own + np.maximum(count - 1, 0)[:, None] * U * total
    out = np.zeros((len(pos), 3))
    for c in range(3):
        jac = [p[0, c] - sx * p[2, c], p[1, c] - sy * p[2, c]]
        err_jac = [np.abs(p[2, c]) * err_s[i] + U * np.abs((sx, sy)[i] * p[2, c])
                   + U * np.abs(jac[i]) for i in range(2)]
        bound, size = np.zeros(len(pos)), np.zeros(len(pos))
        for i in range(2):
            bound += summed[:, i] * np.abs(jac[i]) + total[:, i] * err_jac[i] \
                + U * total[:, i] * np.abs(jac[i])
            size += total[:, i] * np.abs(jac[i])
        bound += U * (2 + 4 * cond_w) * size
        bound += 4 * (step * np.abs(p[2, :3]).sum() / np.abs(w)) ** 2 * size
        first, first_size = bound / np.abs(w), size / np.abs(w)
        second_size = total[:, 2] * abs(p[2, c])
        second = summed[:, 2] * abs(p[2, c]) + U * second_size
        out[:, c] = 2 * (first + second + U * (first_size + second_size))
    return out


# ------------------------------------------------------------------------------- float64 model
SCENES = [(401, 10, 24, 20), (402, 14, 21, 17), (403, 12, 33, 13)]


def _perspective(seed, count, width, height):
    """K34's seeded scenes (colours uniform in 0 .. 1, so of contrast of order 1) -> a namespace."""
    vertices, triangles, colors, _ = R.scene(seed, count)
    cam = R.camera(width, height)
    proj = projection_matrices([cam])[0]
    state = R.setup(vertices, triangles, proj, width, height)
    zbuf = R.draw(state, width, height)
    ids = np.where(zbuf == R.EMPTY, -1, (zbuf & np.uint64(0xFFFFFFFF)).astype(np.int64)).astype(np.int32)
    g = np.random.default_rng(seed + 1).uniform(-1, 1, (width * height, 3)).astype(np.float32)
    grad, grads = I.interior_backward(state, ids, g, colors, vertices, triangles, proj, width,
                                      height)
    return dict(vertices=vertices, triangles=triangles, colors=colors, proj=proj, state=state,
                ids=ids, g=g, grad=grad, grads=grads, width=width, height=height)


_CACHE = {}


def _scene(seed, count, width, height):
    key = (seed, count, width, height)
    if key not in _CACHE:
        _CACHE[key] = _perspective(*key)
    return _CACHE[key]


@pytest.mark.parametrize("seed,count,width,height", SCENES)
def test_face_gradients_are_the_central_differences_of_the_model(seed, count, width, height):
    """Every entry of K35a's restatement against the central difference (h = 1e-6 px, and 1e-6 in
    w) of the float64 model of that triangle's pixels in the screen position and w of the entry's
    corner, at the record's snapped positions and with the ids frozen, within ``_entry_budget``
    (derived there); and for at least half of the entries the budget is below 1e-3 |entry|.
    Worst use of the budget observed: 0.036 (seed 401), 0.037 (402), 0.023 (403); the budget is below
    1e-3 |entry| for 70 of 72, 80 of 81 and 77 of 81 entries."""
    s = _scene(seed, count, width, height)
    state, ids = s["state"], s["ids"]
    worst, seen, informative = 0.0, 0, 0
    for f in np.unique(ids[ids >= 0]):
        _, _, px, py, pixel = I.selected(state, f, ids, width, height)
        points = np.stack([px, py], -1).astype(np.float64)
        corners = np.stack([state["X"][f] / 256.0, state["Y"][f] / 256.0,
                            state["w"][f].astype(np.float64)], -1)           # (3,3): sx, sy, w
        c = s["colors"].astype(np.float64)[state["ids"][f]]
        budget, _ = _entry_budget(state, f, ids, s["colors"], s["g"], width, height, STEP)
        for j in range(3):
            for k in range(3):
                values = []
                for sign in (1, -1):
                    moved = corners.copy()
                    moved[j, k] += sign * STEP
                    values.append(I.triangle_loss64(moved[:, :2], moved[:, 2], c, points,
                                                    s["g"][pixel]))
                want = (values[0] - values[1]) / (2 * STEP)
                noise = 4 * EPS * max(abs(values[0]), abs(values[1])) / STEP
                got = float(s["grads"][f][3 * j + k])
                worst = max(worst, abs(got - want) / (budget[3 * j + k] + noise))
                seen += 1
                informative += budget[3 * j + k] + noise < 1e-3 * abs(got)
    print("face gradients: %d entries, worst use of the budget %.3f, budget below 1e-3 |entry| for "
          "%d" % (seen, worst, informative))
    assert seen >= 45 and worst <= 1.0
    assert 2 * informative >= seen


@pytest.mark.parametrize("seed,count,width,height", SCENES)
def test_the_vertex_gradient_is_the_central_difference_of_the_model(seed, count, width, height):
    """K35b's restatement against central differences (h = 1e-6 scene units) of the float64 model
    in the 3-D positions: a vertex's screen position and w are the record's plus what the float64
    projection moves by (the snap passed straight through), ids frozen.  Within
    ``_vertex_budget`` (derived there), and for at least half of the components the budget is
    below 1e-3 |component|.  Worst use of the budget observed: 0.006 (seed 401), 0.012
    (402), 0.006 (403); informative for 68 of 72, 75 of 81 and 75 of 81 components."""
    s = _scene(seed, count, width, height)
    state, ids = s["state"], s["ids"]
    budget = _vertex_budget(state, ids, s["colors"], s["g"], width, height, s["grads"],
                            s["triangles"], s["vertices"], s["proj"], STEP)
    model = I.Model64(state, ids, s["vertices"], s["proj"], s["colors"], width, s["g"])
    pos = s["vertices"].astype(np.float64)
    used = sorted(set(state["ids"][np.unique(ids[ids >= 0])].reshape(-1).tolist()))
    assert len(used) >= 15
    worst, seen, informative = 0.0, 0, 0
    for v in used:
        touching = set(np.flatnonzero((state["ids"] == v).any(1)).tolist())
        for c in range(3):
            values = []
            for sign in (1, -1):
                moved = pos.copy()
                moved[v, c] += sign * STEP
                values.append(model.loss(moved, touching))
            want = (values[0] - values[1]) / (2 * STEP)
            noise = 4 * EPS * max(abs(values[0]), abs(values[1])) / STEP
            got = float(s["grad"][v][c])
            worst = max(worst, abs(got - want) / (budget[v, c] + noise))
            seen += 1
            informative += budget[v, c] + noise < 1e-3 * abs(got)
    untouched = np.setdiff1d(np.arange(len(pos)), used)
    assert not s["grad"][untouched].any()
    print("vertex gradient: %d components, worst use of the budget %.3f, budget below 1e-3 "
          "|component| for %d" % (seen, worst, informative))
    assert worst <= 1.0
    assert 2 * informative >= seen


# ------------------------------------------------------------------------------- closed forms
@pytest.mark.parametrize("seed,count,width,height", SCENES)
def test_the_position_entries_of_a_triangle_sum_to_minus_g(seed, count, width, height):
    """sum_j lambda_j = 1: moving the whole triangle is moving the sample point, so the three
    position entries sum to -sum_p G_p.  Within the counted roundings: each entry's own budget
    (``_entry_budget`` without the central-difference term) on both sides -- G_p in float64 from
    the model's blend is what the entries' real values sum to exactly."""
    s = _scene(seed, count, width, height)
    state, ids = s["state"], s["ids"]
    checked = 0
    for f in np.unique(ids[ids >= 0]):
        _, _, px, py, pixel = I.selected(state, f, ids, width, height)
        points = np.stack([px, py], -1).astype(np.float64)
        screen = np.stack([state["X"][f] / 256.0, state["Y"][f] / 256.0], -1)
        w = state["w"][f].astype(np.float64)
        c = s["colors"].astype(np.float64)[state["ids"][f]]
        budget, _ = _entry_budget(state, f, ids, s["colors"], s["g"], width, height, STEP)
        for axis in range(2):
            values = []
            for sign in (1, -1):
                shifted = points.copy()
                shifted[:, axis] += sign * STEP
                values.append(I.triangle_loss64(screen, w, c, shifted, s["g"][pixel]))
            total_g = (values[0] - values[1]) / (2 * STEP)
            noise = 4 * EPS * max(abs(values[0]), abs(values[1])) / STEP
            got = sum(float(s["grads"][f][3 * j + axis]) for j in range(3))
            assert abs(got + total_g) <= budget[axis::3][:3].sum() + noise, (f, axis)
            checked += 1
    assert checked >= 10


def test_a_fronto_parallel_triangle_has_an_affine_colour():
    """Equal w: the colour is affine in the pixel, so the entry of corner j at one pixel is
    -lambda_j (grad C)^T g, and the w entries are -r_j q_j with sum_j w_j entry_j = 0 (scaling all
    w alike changes nothing).  Corners on multiples of 1/256 px, under PIXEL_PROJ at z = 2."""
    corners = [(2.25, 1.5), (12.5, 3.0), (5.75, 10.25)]
    vertices, triangles = R.flat(corners, 2.0), np.array([[0, 1, 2]], np.int32)
    colors = np.array([[0.9, 0.1, 0.3], [0.2, 0.8, 0.4], [0.1, 0.3, 0.95]], np.float32)
    width, height = 16, 12
    state = R.setup(vertices, triangles, R.PIXEL_PROJ, width, height)
    ids = A.frame(vertices, triangles, R.PIXEL_PROJ, R.ORIGIN, width, height, colors)["ids"]
    # the affine colour: C(p) = C0 + M p, from the three corners
    base = np.array([[x, y, 1.0] for x, y in corners])
    plane = np.linalg.solve(base, colors.astype(np.float64))               # rows: d/dx, d/dy, 1
    pixels = np.flatnonzero(ids == 0)
    assert len(pixels) > 20
    rng = np.random.default_rng(3)
    for p in pixels[::5]:
        g = np.zeros((width * height, 3), np.float32)
        g[p] = rng.uniform(-1, 1, 3)
        only = np.where(np.arange(width * height) == p, 0, -1).astype(np.int32)
        row = I.face_grads(state, only, g, colors, width, height)[0].astype(np.float64)
        slope = plane[:2] @ g[p].astype(np.float64)                        # (grad C)^T g
        px, py = p % width, p // width
        lam = np.linalg.solve(base.T, np.array([px, py, 1.0]))
        for j in range(3):
            for axis in range(2):
                want = -lam[j] * slope[axis]
                assert abs(row[3 * j + axis] - want) <= 64 * U * np.abs(slope).sum() + 1e-12
        # (2 -(r_j q_j) is exact scaling of w = 2; the sum cancels to roundoff of its terms)
        assert abs(sum(2.0 * row[3 * j + 2] for j in range(3))) <= 64 * U * np.abs(row[2::3]).sum() * 2 + 1e-12


def test_zero_colours_hidden_triangles_and_a_nan_elsewhere():
    """All-zero colours give rows that compare equal to zero; a fully hidden triangle and one off
    the image get nine +0.0f; a NaN in d_color on a pixel the triangle does not win reaches no
    row."""
    width, height = 16, 12
    front = R.flat([(1, 1), (14, 2), (6, 11)], 1.0)
    hidden = R.flat([(4, 3), (9, 4), (6, 8)], 3.0)
    off = R.flat([(-30, -30), (-20, -30), (-25, -12)], 1.0)
    vertices = np.concatenate([front, hidden, off])
    triangles = np.arange(9, dtype=np.int32).reshape(3, 3)
    colors = R.grey(vertices, 9)
    state = R.setup(vertices, triangles, R.PIXEL_PROJ, width, height)
    ids = A.frame(vertices, triangles, R.PIXEL_PROJ, R.ORIGIN, width, height, colors)["ids"]
    assert (ids == 0).sum() > 30 and not (ids == 1).any() and state["status"][2] == R.OFF_IMAGE
    g = np.random.default_rng(4).uniform(-1, 1, (width * height, 3)).astype(np.float32)
    rows = I.face_grads(state, ids, g, colors, width, height)
    assert rows[0].all()
    for f in (1, 2):
        assert np.array_equal(rows[f].view(np.uint32), np.zeros(9, np.uint32))
    zero = I.face_grads(state, ids, g, np.zeros_like(colors), width, height)
    assert (zero == 0).all()
    poisoned = g.copy()
    poisoned[ids != 0] = np.nan
    assert np.array_equal(I.face_grads(state, ids, poisoned, colors, width, height).view(np.uint32),
                          rows.view(np.uint32))


# ------------------------------------------------------------------------------- what it is for
def _convex_scene(width=32, height=28):
    vertices, triangles, centre = I.tetrahedron_with_a_face_vertex()
    cam = R.camera(width, height, yaw=0.0, pitch=0.0)
    proj = projection_matrices([cam])[0]
    eye = eye_positions([cam], (0.0, 0.0, 0.0))[0]
    colors = np.array([[0.9, 0.2, 0.1], [0.1, 0.8, 0.3], [0.2, 0.3, 0.9], [0.5, 0.5, 0.5],
                       [0.95, 0.9, 0.1]], np.float32)
    rng = np.random.default_rng(8)
    g_color = rng.uniform(-1, 1, (width * height, 3)).astype(np.float32)
    g_alpha = rng.uniform(-1, 1, width * height).astype(np.float32)
    return vertices, triangles, centre, cam, proj, eye, colors, g_color, g_alpha


def test_a_visible_vertex_on_no_outline_gets_its_gradient_from_k35():
    """A closed convex mesh seen from one camera: the vertex in the middle of the front face gets
    exactly zero from K34's restatement, and from K35's a gradient that matches the float64 model
    within ``_vertex_budget``."""
    width, height = 32, 28
    vertices, triangles, centre, _, proj, eye, colors, g_color, g_alpha = _convex_scene(width, height)
    opposite = ffn.edge_opposites(triangles, len(vertices), "cpu").numpy()
    grad34, plain, _, fr, made, _ = A.geometry_backward(vertices, triangles, proj, eye, width,
                                                        height, colors, opposite, g_color, g_alpha)
    state, ids = fr["state"], fr["ids"]
    assert sum(pair is not None for pair in made) > 20 and grad34[:3].any()
    assert set(np.unique(ids).tolist()) == {-1, 0, 1, 2}                   # the front face only
    assert np.array_equal(grad34[centre].view(np.uint32), np.zeros(3, np.uint32))
    grad35, grads = I.interior_backward(state, ids, plain, colors, vertices, triangles, proj,
                                        width, height)
    assert np.abs(grad35[centre]).min() > 0
    budget = _vertex_budget(state, ids, colors, plain, width, height, grads, triangles, vertices,
                            proj, STEP)
    model = I.Model64(state, ids, vertices, proj, colors, width, plain)
    pos = vertices.astype(np.float64)
    for c in range(3):
        values = []
        for sign in (1, -1):
            moved = pos.copy()
            moved[centre, c] += sign * STEP
            values.append(model.loss(moved))
        want = (values[0] - values[1]) / (2 * STEP)
        noise = 4 * EPS * max(abs(values[0]), abs(values[1])) / STEP
        assert abs(float(grad35[centre][c]) - want) <= budget[centre, c] + noise
        # (the match means something only if the parent's answer, zero, would not pass it too)
        assert budget[centre, c] + noise < abs(want)
        print("component %d: %.6g, budget %.3g of it" % (c, want, (budget[centre, c] + noise) / abs(want)))


def _fake_frame(fr):
    def fake(vertices, triangles, proj, eye, width, height, colors, **kwargs):
        n = width * height
        return (torch.zeros((len(triangles), 16), dtype=torch.int32), torch.from_numpy(fr["color"]),
                torch.from_numpy(fr["alpha"]), torch.zeros(n), torch.from_numpy(fr["ids"]),
                torch.zeros(len(triangles), dtype=torch.uint8), 0, torch.zeros(n, dtype=torch.int64))
    return fake


def test_through_the_public_function_the_vertex_moves(monkeypatch):
    """``render_mesh_geometry_backward(interior=True)`` with the four kernels replaced by their
    restatements (no GPU here): the vertex on no outline gets K35's gradient added to K34's zero.
    Without ``interior`` in the signature this fails."""
    width, height = 32, 28
    vertices, triangles, centre, cam, proj, eye, colors, g_color, g_alpha = _convex_scene(width, height)
    opposite = ffn.edge_opposites(triangles, len(vertices), "cpu")
    grad34, plain, d_alpha, fr, made, (entry_vertex, entry_grad) = A.geometry_backward(
        vertices, triangles, proj, eye, width, height, colors, opposite.numpy(), g_color, g_alpha)
    state = fr["state"]
    monkeypatch.setattr(mesh, "_rasterize_z", _fake_frame(fr))
    monkeypatch.setattr(mesh, "_mesh_on", lambda v, t, device=None: (
        True, torch.device("cpu"), torch.from_numpy(np.asarray(v, np.float32)),
        torch.from_numpy(np.asarray(t, np.int32))))
    monkeypatch.setattr(ops, "mesh_aa_backward", lambda *a: (
        torch.from_numpy(plain), torch.from_numpy(d_alpha), torch.from_numpy(entry_vertex),
        torch.from_numpy(entry_grad)))
    monkeypatch.setattr(ops, "mesh_aa_vertex_grad", lambda sv, order, eg, v, p, grad, accumulate:
                        torch.from_numpy(grad34.copy()))
    seen = []

    def face(record, ids, d_color, cols, tri, w, h):
        seen.append("a")
        assert np.array_equal(d_color.numpy(), plain) and (w, h) == (width, height)
        return torch.from_numpy(I.face_grads(state, ids.numpy(), d_color.numpy(), cols.numpy(), w, h))

    def vertex(face_grads, order, starts, v, p, grad, accumulate):
        seen.append("b")
        assert accumulate and grad is not None
        want_order, want_starts = I.adjacency(triangles, len(vertices))
        assert np.array_equal(order.numpy(), want_order) and np.array_equal(starts.numpy(), want_starts)
        grad.copy_(torch.from_numpy(I.vertex_grad(face_grads.numpy(), order.numpy(), starts.numpy(),
                                                  v.numpy(), p, grad.numpy())))
        return grad
    monkeypatch.setattr(ops, "mesh_interp_face_grads", face)
    monkeypatch.setattr(ops, "mesh_interp_vertex_grad", vertex)
    plain_only, _ = ffn.render_mesh_geometry_backward(vertices, triangles, cam, colors, g_color,
                                                      g_alpha, opposites=opposite)
    assert seen == [] and not plain_only[centre].any()
    got, got_plain = ffn.render_mesh_geometry_backward(vertices, triangles, cam, colors, g_color,
                                                       g_alpha, opposites=opposite, interior=True)
    assert seen == ["a", "b"] and np.array_equal(got_plain, plain)
    want, _ = I.interior_backward(state, fr["ids"], plain, colors, vertices, triangles, proj, width,
                                  height, grad34)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(got[centre]).min() > 0


# ------------------------------------------------------------------------------- plumbing
def test_the_new_names_are_built_declared_and_reachable():
    assert build.SOURCES["mesh_interp_grad.hip"] == ["-ffp-contract=off"]
    from fourier_feature_nets_amd import _lib
    declared = set(_lib.declared_symbols())
    assert {"ffn_mesh_interp_face_grads", "ffn_mesh_interp_vertex_grad"} <= declared
    assert _lib.ABI_VERSION == 3
    for name in ("mesh_interp_face_grads", "mesh_interp_vertex_grad"):
        assert callable(getattr(ops, name)) and callable(getattr(ops, name + "_check"))
    import inspect
    for function in (ffn.render_mesh_geometry_backward, ffn.fit_mesh_geometry):
        assert inspect.signature(function).parameters["interior"].default is False
    names = list(inspect.signature(ffn.render_mesh_geometry_backward).parameters)
    assert names[-2:] == ["interior", "adjacency"]
    assert list(inspect.signature(ffn.fit_mesh_geometry).parameters)[-1] == "interior"


def test_interior_false_never_reaches_the_new_ops(monkeypatch):
    from fourier_feature_nets_amd import _lib
    called = []

    def call(name, *args):
        called.append(name)
        raise RuntimeError("stop at " + name)
    monkeypatch.setattr(_lib, "call", call)

    def boom(*args, **kwargs):
        raise AssertionError("K35 was reached")
    for name in ("mesh_interp_face_grads", "mesh_interp_vertex_grad"):
        monkeypatch.setattr(ops, name, boom)
    monkeypatch.setattr(mesh, "vertex_adjacency", boom)
    monkeypatch.setattr(mesh, "_interior_backward", boom)
    width, height = 32, 28
    vertices, triangles, _, cam, proj, eye, colors, g_color, g_alpha = _convex_scene(width, height)
    fr = A.frame(vertices, triangles, proj, eye, width, height, colors)
    monkeypatch.setattr(mesh, "_rasterize_z", _fake_frame(fr))
    monkeypatch.setattr(mesh, "_mesh_on", lambda v, t, device=None: (
        True, torch.device("cpu"), torch.from_numpy(np.asarray(v, np.float32)),
        torch.from_numpy(np.asarray(t, np.int32))))
    monkeypatch.setattr(ops, "mesh_aa_backward", lambda *a: (
        torch.zeros((width * height, 3)), torch.zeros(width * height),
        torch.full((4 * width * height,), 5, dtype=torch.int32), torch.zeros((4 * width * height, 2))))
    monkeypatch.setattr(ops, "mesh_aa_vertex_grad",
                        lambda sv, order, eg, v, p, grad, accumulate: torch.zeros((5, 3)))
    grad, _ = ffn.render_mesh_geometry_backward(vertices, triangles, cam, colors, g_color, g_alpha,
                                                opposites=torch.zeros(18, dtype=torch.int32))
    assert grad.shape == (5, 3) and called == []
    # and True does reach them, after K34c
    monkeypatch.setattr(mesh, "vertex_adjacency", lambda t, n, d: ("order", "starts"))
    reached = []
    monkeypatch.setattr(mesh, "_interior_backward", lambda *a: reached.append(a[1]))
    ffn.render_mesh_geometry_backward(vertices, triangles, cam, colors, g_color, g_alpha,
                                      opposites=torch.zeros(18, dtype=torch.int32), interior=True)
    assert reached == [("order", "starts")]


def _refused(name, function, args, **change):
    with pytest.raises(ValueError, match=name) as error:
        function(**dict(args, **change))
    return str(error.value)


def test_the_ops_refuse_by_name():
    n = 30
    face = dict(record=torch.zeros((2, 16), dtype=torch.int32), ids=torch.zeros(n, dtype=torch.int32),
                d_color=torch.zeros((n, 3)), colors=torch.zeros((4, 3)),
                triangles=torch.zeros((2, 3), dtype=torch.int32), width=6, height=5)
    check = ops.mesh_interp_face_grads_check
    check(**face)
    assert "mesh_interp_face_grads" in _refused("record", check, face, record=face["record"][:1])
    _refused("record", check, face, record=face["record"][:, :12])
    _refused("ids", check, face, ids=face["ids"][:-1])
    _refused("d_color", check, face, d_color=face["d_color"].double())
    _refused("colors", check, face, colors=face["colors"][:, :2])
    _refused("colors", check, face, colors=face["colors"][:0])
    _refused("triangles", check, face, triangles=face["triangles"].long())
    _refused("width", check, face, width=0)
    vertex = dict(face_grads=torch.zeros((2, 9)), corner_order=torch.zeros(6, dtype=torch.int32),
                  vertex_starts=torch.zeros(5, dtype=torch.int32), vertices=torch.zeros((4, 3)),
                  proj=np.eye(4, dtype=np.float32)[:3])
    check = ops.mesh_interp_vertex_grad_check
    check(**vertex)
    assert "mesh_interp_vertex_grad" in _refused("face_grads", check, vertex,
                                                 face_grads=torch.zeros((2, 12)))
    _refused("corner_order", check, vertex, corner_order=vertex["corner_order"][:-1])
    _refused("vertex_starts", check, vertex, vertex_starts=vertex["vertex_starts"][:-1])
    _refused("vertices", check, vertex, vertices=vertex["vertices"].double())
    _refused("proj", check, vertex, proj=np.eye(4))
    _refused("proj", check, vertex, proj=np.full((3, 4), np.nan))
    _refused("grad", check, vertex, grad=torch.zeros((5, 3)))
    _refused("accumulate", check, vertex, accumulate=True)
    # the wrappers themselves: the checks come before the first launch
    from tests import refusal_cases as rc
    for name, args in (("mesh_interp_face_grads", face), ("mesh_interp_vertex_grad", vertex)):
        with pytest.MonkeyPatch.context() as patch:
            hook = rc.Hook().install(patch)
            bad = dict(args)
            bad[sorted(k for k, v in args.items() if torch.is_tensor(v))[0]] = None
            with pytest.raises(ValueError, match=name):
                getattr(ops, name)(**bad)
            assert hook.seen == []


def test_the_host_functions_refuse_before_the_device(monkeypatch):
    def boom(*args, **kwargs):
        raise AssertionError("the device was reached")
    monkeypatch.setattr(mesh, "_rasterize_z", boom)
    monkeypatch.setattr(mesh, "_mesh_on", boom)
    monkeypatch.setattr(mesh, "vertex_adjacency", boom)
    vertices, triangles = R.quad_scene()
    colors = R.grey(vertices)
    cam = R.camera(6, 5)
    good = (np.zeros((30, 3), np.float32), np.zeros(30, np.float32))
    back = ffn.render_mesh_geometry_backward
    with pytest.raises(ValueError, match="colors"):
        back(vertices, triangles, cam, None, *good, interior=True)
    with pytest.raises(ValueError, match="d_color"):
        back(vertices, triangles, cam, colors, good[0][:-1], good[1], interior=True)
    with pytest.raises(ValueError, match="triangles"):
        back(vertices, triangles + 9, cam, colors, *good, interior=True)

    class Data:
        images = np.zeros((2, 5, 6, 4), np.uint8)
        cameras = [cam, cam]
        color_space = "RGB"
    with pytest.raises(ValueError, match="learning_rate"):
        ffn.fit_mesh_geometry(vertices, triangles, colors, Data(), learning_rate=0.0, interior=True)
    with pytest.raises(ValueError, match="triangles"):
        ffn.fit_mesh_geometry(vertices, triangles + 9, colors, Data(), interior=True)


def test_the_script_has_the_flag():
    from scripts import fit_mesh
    parser = fit_mesh.build_parser()
    assert parser.parse_args(["a", "b", "c"]).interior is False
    assert parser.parse_args(["a", "b", "c", "--interior"]).interior is True


def test_the_cases_and_rows_are_registered():
    from tests import refusal_cases as rc
    from tests.stream_order_cases import CASES
    reached = {entry for case in CASES for entry in case.reaches}
    for name in ("mesh_interp_face_grads", "mesh_interp_vertex_grad"):
        assert "ffn_" + name in reached
        assert name in rc.ROWS and name in rc.subjects()
        assert not rc.ROWS[name].gpu_only and not rc.ROWS[name].marked
    assert not [key for key in rc.ACCEPTED if key[0].startswith("mesh_interp")]
    assert not [key for key in rc.BY_VALUE_ONLY if key[0].startswith("mesh_interp")]
